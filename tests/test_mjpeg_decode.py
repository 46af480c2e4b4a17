"""CPU: the Motion-JPEG decoder's specification against a decoder that is not
ours. tests/mjpeg_dec_ref.py (an independent numpy restatement of DESIGN.md
"Motion-JPEG decoder") equals Pillow byte for byte on the project's own streams
and on Pillow-encoded ones; dvc_jpegd_set_header on a host-only handle accepts
those and refuses what is outside the contract; tools/jpegd_host_check.cc — the
text the GPU kernels compile, built for the host under ASan and UBSan as a
stand-alone program — reproduces the reference and survives the damaged streams
the GPU test then uses."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import mjpeg_dec_cases as D
from tests import mjpeg_dec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("kind,name,gray", D.ids())
def test_reference_decoder_equals_pillow(kind, name, gray, variant):
    jpg = D.stream(kind, name, gray, variant)
    got, pil = D.expected(kind, name, gray, variant), D.pillow(jpg)
    assert got.shape == pil.shape and got.dtype == pil.dtype
    assert np.array_equal(got, pil), f"{np.count_nonzero(got != pil)} bytes differ, " \
        f"first at {tuple(int(v[0]) for v in np.nonzero(got != pil))}"


def _host_handle(N, w=4096, h=4096):
    h_ = ctypes.c_void_p()
    N.check(N.lib().dvc_jpegd_create(w, h, 1, -1, None, 0, ctypes.byref(h_)))
    return h_


def _set_header(N, h, data):
    n, w, hh, fmt = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = N.lib().dvc_jpegd_set_header(h, data, len(data), ctypes.byref(n), ctypes.byref(w), ctypes.byref(hh),
                                      ctypes.byref(fmt))
    return rc, n.value, w.value, hh.value, fmt.value


def test_header_parser_accepts_every_case():
    from dvc_amd import _native as N
    h = _host_handle(N)
    try:
        for kind, name, gray in D.ids():
            jpg = D.stream(kind, name, gray)
            info = R.parse(jpg)
            want = (N.DVC_OK, info["start"], info["W"], info["H"], N.FMT_GRAY if len(info["comps"]) == 1 else N.FMT_BGR)
            assert _set_header(N, h, jpg) == want, name                       # a whole sample
            assert _set_header(N, h, jpg[:info["start"]]) == want, name       # the header alone
    finally:
        N.lib().dvc_jpegd_destroy(h)


def test_header_parser_refuses_what_is_outside_the_contract():
    import io
    from PIL import Image
    from dvc_amd import _native as N
    a = np.random.default_rng(3).integers(0, 256, (37, 70, 3), dtype=np.uint8)

    def pil(**kw):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=75, **kw)
        return buf.getvalue()

    good = pil(subsampling=2)
    h = _host_handle(N)
    try:
        assert _set_header(N, h, good)[0] == N.DVC_OK
        first = _set_header(N, h, good)
        for bad in (pil(progressive=True, subsampling=2), pil(subsampling=0), pil(subsampling=1)):
            assert _set_header(N, h, bad)[0] == N.DVC_E_UNSUPPORTED
        cut = R.parse(good)["start"]
        for n in (0, 1, 2, 3, 20, cut // 2, cut - 1):
            assert _set_header(N, h, good[:n])[0] == N.DVC_E_INVALID, n
        assert _set_header(N, h, b"\x00" + good[1:])[0] == N.DVC_E_INVALID
        assert _set_header(N, h, good) == first
    finally:
        N.lib().dvc_jpegd_destroy(h)
    small = _host_handle(N, 69, 37)                                           # the handle's largest frame
    try:
        assert _set_header(N, small, good)[0] == N.DVC_E_INVALID
    finally:
        N.lib().dvc_jpegd_destroy(small)
    # a host-only handle decodes nothing
    h = _host_handle(N)
    try:
        assert _set_header(N, h, good)[0] == N.DVC_OK
        z = np.zeros(16, np.uint8)
        sizes, st = np.array([4], np.uint32), np.zeros(1, np.int32)
        assert N.lib().dvc_jpegd_decode(h, z.ctypes.data, 16, sizes.ctypes.data, 1, z.ctypes.data, 3 * 70, 0,
                                        st.ctypes.data) == N.DVC_E_STATE
    finally:
        N.lib().dvc_jpegd_destroy(h)


HOST_CASES = [("ref", "noise70x37_q90", False), ("ref", "noise70x37_q90", True), ("pil", "pil70x37_blocks7", None),
              ("pil", "pil33x17_opt", None), ("pil", "pil3x5", None), ("ref", "alt8", False)]


def test_host_program_under_sanitizers(tmp_path):
    """The kernels' serial routines, compiled for the host with ASan and UBSan into
    a stand-alone program: the reference's bytes on six cases, and a clean exit
    with a damaged status on every damaged stream of the GPU test."""
    exe = tmp_path / "jpegd_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), os.path.join(ROOT, "tools", "jpegd_host_check.cc")], check=True)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    for i, (kind, name, gray) in enumerate(HOST_CASES):
        (src / f"good{i}.jpg").write_bytes(D.stream(kind, name, gray))
    for kind in D.DAMAGE:
        hdr, data = D.damaged(kind)
        (src / f"bad_{kind}.jpg").write_bytes(hdr + data[1])
        assert R.parse(hdr + data[0])["W"] == 70
        with pytest.raises(R.Damaged):
            R.decode(hdr + data[1])
    (src / "bad_header.jpg").write_bytes(D.stream("ref", "noise70x37_q90")[:100])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines()}
    for i, (kind, name, gray) in enumerate(HOST_CASES):
        want = D.expected(kind, name, gray)
        assert lines[f"good{i}"] == [want.shape[1], want.shape[0], 3 if want.ndim == 3 else 1, 0]
        got = np.fromfile(dst / f"good{i}.raw", np.uint8).reshape(want.shape)
        assert np.array_equal(got, want), (kind, name, gray)
    for kind in list(D.DAMAGE) + ["header"]:
        assert lines[f"bad_{kind}"][3] == -1 and not (dst / f"bad_{kind}.raw").exists(), kind
