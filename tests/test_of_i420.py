"""CPU side of DVC_FLAG_OUT_I420 on the optical-flow path: the Python surface
refuses unknown output formats before it touches the library, the documents
name the flag for OF, and the mask video a Y4M sink writes reads back (the OF
driver's second pass opens it)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_out_format_checked_before_any_library_call(monkeypatch):
    import dvc_amd
    from dvc_amd import _native

    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_native, "lib", no_lib)
    with pytest.raises(ValueError, match="NV12"):
        dvc_amd.OFWorker(64, 32, out_format="NV12")
    with pytest.raises(ValueError, match="NV12"):
        _native.OFCompressor(64, 32, out_format="NV12")


def test_documents_name_the_flag_for_of():
    hdr = open(os.path.join(ROOT, "include", "dvc.h")).read()
    flag = re.search(r"#define DVC_FLAG_OUT_I420.*?\*/", hdr, re.S).group(0)
    assert "dvc_of_create" in flag and "dvc_ofc_create" in flag
    params = re.search(r"uint32_t flags;\s*/\*[^/]*DVC_FLAG_KEEP_PLANES.*?\*/", hdr, re.S).group(0)
    assert "DVC_FLAG_OUT_I420" in params
    ofc = hdr[hdr.index("typedef struct dvc_ofc dvc_ofc;") - 1500:hdr.index("typedef struct dvc_ofc dvc_ofc;")]
    assert "DVC_FLAG_OUT_I420" in ofc
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("Encoder-ready outputs"):]
    sec = sec[:3000]
    assert "dvc_of_create" in sec and "dvc_ofc_create" in sec and "DVC_FLAG_OUT_I420" in sec


def test_y4m_mono_reads_back(tmp_path):
    from dvc_amd import video_io
    W, H = 10, 6
    frames = [((np.arange(W * H) * k) % 256).astype(np.uint8).reshape(H, W) for k in (1, 7, 13)]
    w = video_io.open_sink(str(tmp_path / "mask.y4m"), 25, (W, H), is_color=False)
    for f in frames:
        w.write(f)
    w.release()
    cap = video_io.open_source(str(tmp_path / "mask.y4m"))
    assert cap.isOpened() and cap.pixel_format == "GRAY"
    assert cap.get(video_io.CAP_PROP_FRAME_COUNT) == 3 and cap.get(video_io.CAP_PROP_FPS) == 25.0
    for f in frames:
        ok, g = cap.read()
        assert ok and g.shape == (H, W) and np.array_equal(g, f)
    assert cap.read() == (False, None)
    cap.release()
