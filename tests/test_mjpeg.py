"""CPU tests of the Motion-JPEG output path (DESIGN.md "Motion-JPEG stream"):
the constant header dvc_jpeg_header returns (host only), the stream format
checked with a decoder that is not ours (Pillow / libjpeg-turbo on the
reference stream of tests/mjpeg_ref.py), and the MP4 muxer and reader around
an encoder stub that returns the reference stream (the real encoder is a GPU
kernel chain: tests/test_mjpeg_gpu.py)."""
import ctypes
import io
import os
import struct
import sys

import numpy as np
import pytest

from tests import mjpeg_cases as C
from tests import mjpeg_ref as R

from PIL import Image  # noqa: E402  (the independent decoder: libjpeg-turbo)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fmt,W,H,q", [(R.FMT_BGR, 70, 37, 90), (R.FMT_GRAY, 70, 37, 50), (R.FMT_BGR, 1920, 1080, 75),
                                       (R.FMT_BGR, 1, 1, 1), (R.FMT_GRAY, 9, 8, 100)])
def test_header_parses_and_tables_are_complete(fmt, W, H, q):
    info = R.parse_header(R.header_bytes(W, H, fmt, q))
    assert info["order"] == ["SOI", "APP0", "DQT", "DQT", "SOF0", "DHT", "DHT", "DRI", "SOS"]
    assert info["jfif"][:5] == b"JFIF\0"
    assert (info["W"], info["H"]) == (W, H)                      # SOF0 carries the true size
    gray = fmt == R.FMT_GRAY
    assert [c[1:] for c in info["comps"]] == ([(1, 1, 0)] if gray else [(2, 2, 0), (1, 1, 1), (1, 1, 1)])
    assert info["dri"] == -(-W // (8 if gray else 16))           # one MCU row
    assert [(td, ta) for _, td, ta in info["scan"]] == [(0, 0)] * len(info["comps"])
    for t in (0, 1):
        assert info["q"][t].min() >= 1 and info["q"][t].max() <= 255
        if q == 100:
            assert (info["q"][t] == 1).all()
    dc, ac = info["huff"][(0, 0)], info["huff"][(1, 0)]
    assert sorted(dc) == list(range(12))
    assert sorted(ac) == sorted([0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)])
    for table in (dc, ac):
        assert all(1 <= ln <= 16 for _, ln in table.values())
        assert all(code != (1 << ln) - 1 for code, ln in table.values())       # no code is all ones
        assert sum(2.0 ** -ln for _, ln in table.values()) < 1.0
        assert len({(code, ln) for code, ln in table.values()}) == len(table)


def test_quality_scales_the_quantiser_ijg_style():
    base = R.parse_header(R.header_bytes(16, 16, R.FMT_BGR, 50))["q"]      # s = 100: the base tables
    for q in (1, 20, 49, 75, 90):
        s = 5000 // q if q < 50 else 200 - 2 * q
        got = R.parse_header(R.header_bytes(16, 16, R.FMT_BGR, q))["q"]
        for t in (0, 1):
            assert np.array_equal(got[t], np.clip((base[t] * s + 50) // 100, 1, 255))


def test_header_and_bound_argument_checks():
    from dvc_amd import _native as N
    L, h, n = N.lib(), ctypes.c_void_p(), ctypes.c_size_t()
    for args in ((0, 8, 0, 75), (8, 8, 0, 0), (8, 8, 0, 101), (8, 8, 7, 75), (8, 8, 1, 75), (70000, 8, 0, 75)):
        assert L.dvc_jpeg_create(*args, 1, -1, None, 0, ctypes.byref(h)) < 0
    assert L.dvc_jpeg_bound(8, 8, 1, ctypes.byref(n)) < 0
    N.check(L.dvc_jpeg_create(64, 48, 0, 75, 1, -1, None, 0, ctypes.byref(h)))
    N.check(L.dvc_jpeg_header(h, None, 0, ctypes.byref(n)))
    small = (ctypes.c_uint8 * 16)()
    assert L.dvc_jpeg_header(h, small, 16, ctypes.byref(n)) == N.DVC_E_NOMEM and n.value > 16
    out, sizes = (ctypes.c_uint8 * 64)(), (ctypes.c_uint32 * 1)()
    assert L.dvc_jpeg_encode(h, out, 192, 0, 1, out, 64, sizes) == N.DVC_E_STATE   # host-only handle
    L.dvc_jpeg_destroy(h)


def _decode(jpeg, size):
    im = Image.open(io.BytesIO(jpeg))
    im.draft("YCbCr", size)
    a = np.asarray(im)
    assert im.mode == "YCbCr"
    return a.astype(np.int64)


def _check_plane(got, want, what):
    want = np.rint(np.clip(want, 0, 255))
    assert got.shape == want.shape, what
    d = np.abs(got - want)
    print(f"{what}: max |diff| {d.max():.0f}, {100 * np.mean(d > 0):.2f} % of samples differ")
    assert d.max() <= 1, what                  # IEEE-1180 accuracy of libjpeg's inverse DCT
    assert np.mean(d > 0) <= 0.05, what


@pytest.mark.parametrize("name", list(C.CASES))
def test_independent_decoder_reads_the_reference_stream(name):
    ref = C.reference(name)
    H, W = C.frame(name).shape[:2]
    _check_plane(_decode(ref["jpeg"], (W, H))[..., 0], ref["Y"], f"{name} luma")
    half = _decode(ref["jpeg"], (W // 2, H // 2))      # chroma at its own size: no upsampling involved
    _check_plane(half[..., 1], ref["Cb"], f"{name} Cb")
    _check_plane(half[..., 2], ref["Cr"], f"{name} Cr")


@pytest.mark.parametrize("name", list(C.EXTRA))
def test_independent_decoder_reads_tiny_frames(name):
    ref = C.reference(name)
    H, W = C.frame(name).shape[:2]
    _check_plane(_decode(ref["jpeg"], (W, H))[..., 0], ref["Y"], f"{name} luma")


def test_independent_decoder_reads_the_gray_stream():
    ref = C.reference(C.GRAY_CASE, 0, True)
    im = Image.open(io.BytesIO(ref["jpeg"]))
    assert im.mode == "L"
    _check_plane(np.asarray(im).astype(np.int64), ref["Y"], "gray")


def test_cases_reach_what_they_are_for():
    zz = [b.reshape(64)[R.ZIGZAG] for b in C.reference("zz63")["levels"][0].reshape(-1, 8, 8)]
    assert all(np.flatnonzero(b).tolist() == [63] for b in zz)                  # 62 zeros: three ZRLs
    dc = C.reference("alt8")["levels"][0][0, :, 0, 0]
    assert abs(int(dc[1]) - int(dc[0])) == 2040                                 # DC size 11
    assert sum(C.reference(n)["stuffed"] for n in C.CASES) > 0                   # stuffed 0xFF bytes exist
    assert C.reference("rst_wrap32x160")["stream"].count(b"\xff\xd0") >= 2      # RST index wrapped
    assert C.reference("wide1120x32")["info"]["dri"] * 6 == 420
    lv = C.reference("const16")["levels"]
    assert all(not l.reshape(-1, 64)[:, 1:].any() for l in lv)                  # EOB-only blocks
    for n in C.CASES:
        f = C.frame(n)
        b = ctypes.c_size_t()
        from dvc_amd import _native as N
        N.check(N.lib().dvc_jpeg_bound(f.shape[1], f.shape[0], 0, ctypes.byref(b)))
        assert len(C.reference(n)["stream"]) <= b.value


def test_committed_tables_are_what_the_tool_generates():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_jpeg_tables as G
    finally:
        sys.path.pop(0)
    assert open(G.HEADER).read() == G.render()


# ---- muxer, reader, sink selection (an encoder stub returning the reference stream) ----
class RefEncoder:
    def __init__(self, width, height, is_color=True, quality=75, max_batch=8, device=0):
        self.quality = quality
        self.header = R.header_bytes(width, height, R.FMT_BGR if is_color else R.FMT_GRAY, quality)

    def encode(self, frames):
        return [R.encode(f, self.quality)["stream"] for f in frames]


def _boxes(buf, start, end):
    out, p = [], start
    while p < end:
        size, kind = struct.unpack_from(">I4s", buf, p)
        head = 8
        if size == 1:
            size, head = struct.unpack_from(">Q", buf, p + 8)[0], 16
        assert size >= head and p + size <= end, (kind, size)
        out.append((kind.decode("latin1"), p + head, p + size))
        p += size
    return out


def _tree(buf, start, end, containers=("moov", "trak", "mdia", "minf", "dinf", "stbl")):
    return [(k, _tree(buf, a, b) if k in containers else None) for k, a, b in _boxes(buf, start, end)]


def _clip(n=5, W=70, H=37):
    from dvc_amd.synthetic import clip
    return clip(W, H, n, seed=9)


def test_muxer_box_tree_and_sample_table(tmp_path):
    from dvc_amd import video_io
    frames = _clip()
    path = str(tmp_path / "out.mp4")
    w = video_io.Mp4MjpegWriter(path, 29.97, (70, 37), encoder=RefEncoder(70, 37, quality=60), batch=2)
    assert w.isOpened()
    for f in frames:
        w.write(f)
    w.write(np.zeros((10, 10, 3), np.uint8))          # wrong shape: dropped
    w.release()
    buf = open(path, "rb").read()
    assert _tree(buf, 0, len(buf)) == [
        ("ftyp", None), ("mdat", None),
        ("moov", [("mvhd", None), ("trak", [("tkhd", None), ("mdia", [
            ("mdhd", None), ("hdlr", None), ("minf", [("vmhd", None), ("dinf", [("dref", None)]), ("stbl", [
                ("stsd", None), ("stts", None), ("stsc", None), ("stsz", None), ("co64", None)])])])])])]
    top = {k: (a, b) for k, a, b in _boxes(buf, 0, len(buf))}
    moov = dict((k, (a, b)) for k, a, b in _boxes(buf, *top["moov"]))
    trak = dict((k, (a, b)) for k, a, b in _boxes(buf, *moov["trak"]))
    mdia = dict((k, (a, b)) for k, a, b in _boxes(buf, *trak["mdia"]))
    minf = dict((k, (a, b)) for k, a, b in _boxes(buf, *mdia["minf"]))
    stbl = dict((k, (a, b)) for k, a, b in _boxes(buf, *minf["stbl"]))
    assert buf[mdia["hdlr"][0] + 8:mdia["hdlr"][0] + 12] == b"vide"
    timescale, duration = struct.unpack_from(">II", buf, mdia["mdhd"][0] + 12)
    assert (timescale, duration) == (29970, 5 * 1000)
    assert struct.unpack_from(">III", buf, stbl["stts"][0] + 4) == (1, 5, 1000)
    (entry,) = _boxes(buf, stbl["stsd"][0] + 8, stbl["stsd"][1])
    assert entry[0] == "mp4v" and struct.unpack_from(">HH", buf, entry[1] + 24) == (70, 37)
    (esds,) = _boxes(buf, entry[1] + 78, entry[2])
    assert esds[0] == "esds"
    d = buf[esds[1] + 4:esds[2]]
    assert d[0] == 0x03 and d[1] == len(d) - 2 and d[5] == 0x04 and d[6] == 13
    assert d[7] == 0x6C                                 # objectTypeIndication: Visual ISO/IEC 10918-1
    assert d[8] >> 2 == 4                               # streamType: visual
    n = struct.unpack_from(">I", buf, stbl["stsz"][0] + 8)[0]
    sizes = struct.unpack_from(">5I", buf, stbl["stsz"][0] + 12)
    offs = struct.unpack_from(">5Q", buf, stbl["co64"][0] + 8)
    assert n == 5 and struct.unpack_from(">I", buf, stbl["co64"][0] + 4)[0] == 5
    for f, o, s in zip(frames, offs, sizes):
        assert top["mdat"][0] <= o and o + s <= top["mdat"][1]
        assert buf[o:o + s] == R.encode(f, 60)["jpeg"]
    assert offs[0] == top["mdat"][0] and offs[-1] + sizes[-1] == top["mdat"][1]


@pytest.mark.parametrize("color", [True, False])
def test_writer_reader_round_trip(tmp_path, color):
    from dvc_amd import video_io
    frames = _clip(4, 64, 48).copy()
    frames[0] = (10, 120, 240)                       # B, G, R: a swapped channel order would be off by 230
    if not color:
        frames = (frames[..., 1] > 100).astype(np.uint8) * 255
    path = str(tmp_path / "v.mp4")
    w = video_io.Mp4MjpegWriter(path, 25, (64, 48), is_color=color, encoder=RefEncoder(64, 48, color, 100), batch=3)
    for f in frames:
        w.write(f)
    w.release()
    cap = video_io.open_source(path)
    assert isinstance(cap, video_io.Mp4MjpegReader) and cap.isOpened()
    assert cap.get(video_io.CAP_PROP_FPS) == 25.0 and cap.get(video_io.CAP_PROP_FRAME_COUNT) == 4
    assert (cap.get(video_io.CAP_PROP_FRAME_WIDTH), cap.get(video_io.CAP_PROP_FRAME_HEIGHT)) == (64, 48)
    for t, f in enumerate(frames):
        ok, got = cap.read()
        assert ok and got.shape == f.shape and got.dtype == np.uint8
        ref = R.encode(f, 100)
        im = Image.open(io.BytesIO(ref["jpeg"]))      # the sample is the reference image, decoded by Pillow
        if color:
            assert np.array_equal(got, np.asarray(im.convert("RGB"))[:, :, ::-1])
            if t == 0:   # constant frame, Q = 1: Y, Cb, Cr each within 1 of exact, so B (= Y + 1.772 Cb') within 4
                assert np.abs(got.astype(int) - f).max() <= 4
        else:
            assert np.array_equal(got, np.asarray(im))
            assert np.abs(got.astype(np.int64) - np.rint(np.clip(ref["Y"], 0, 255))).max() <= 1
    assert cap.read() == (False, None)
    cap.release()


def test_reader_refuses_other_files(tmp_path):
    from dvc_amd import video_io
    p = tmp_path / "x.mp4"
    p.write_bytes(b"\0\0\0\x18ftypmp42" + b"\0" * 64)
    assert not video_io.Mp4MjpegReader(str(p)).isOpened()
    assert not video_io.open_source(str(p)).isOpened()


def test_open_sink_selection(tmp_path, monkeypatch):
    from dvc_amd import _native, video_io
    monkeypatch.setattr(_native, "JpegEncoder", RefEncoder)
    monkeypatch.delenv("DVC_VIDEO_SINK", raising=False)
    w = video_io.open_sink(str(tmp_path / "a.mp4"), 25, (32, 16))
    assert isinstance(w, video_io.NpyStreamWriter)         # the default is unchanged
    w.release()
    monkeypatch.setenv("DVC_VIDEO_SINK", "y4m")
    w = video_io.open_sink(str(tmp_path / "b.mp4"), 25, (32, 16), is_color=False)
    assert isinstance(w, video_io.Y4mWriter)
    w.release()
    monkeypatch.setenv("DVC_VIDEO_SINK", "mjpeg")
    monkeypatch.setenv("DVC_VIDEO_QUALITY", "40")
    w = video_io.open_sink(str(tmp_path / "c.mp4"), 25, (32, 16))
    assert isinstance(w, video_io.Mp4MjpegWriter) and w._enc.quality == 40
    w.write(np.full((16, 32, 3), 99, np.uint8))
    w.release()
    assert open(tmp_path / "c.mp4", "rb").read(12)[4:12] == b"ftypisom"
    assert isinstance(video_io.open_sink(str(tmp_path / "d.npy"), 25, (32, 16)), video_io.NpyStreamWriter)
    assert isinstance(video_io.open_sink(str(tmp_path / "e.y4m"), 25, (32, 16)), video_io.Y4mWriter)
