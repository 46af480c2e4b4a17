"""CPU: the camera stream set of the Motion-JPEG decoder (DVC_FLAG_JPEGD_CAMERA).
tests/mjpeg_cam_ref.py (an independent numpy decoder for 4:2:0, 4:2:2 and 4:4:4)
equals Pillow byte for byte on the grid of DESIGN.md "Sizes under test";
dvc_jpegd_set_header accepts and refuses what the header says with and without
the flag; the committed Annex K arrays are libjpeg's default DHT segments;
tools/jpegd_host_check.cc (the text the GPU kernels compile, built for the host
under ASan and UBSan as a stand-alone program, `camera` mode) reproduces the
reference and survives the damaged streams the GPU test then uses; the AVI and
raw-stream readers demux hand-built containers and decode what Pillow decodes."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mjpeg_cam_cases as C
from tests import mjpeg_cam_ref as CR
from tests import mjpeg_dec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sub", ["420", "422", "444"])
@pytest.mark.parametrize("w,h", C.GRID_SIZES)
def test_reference_decoder_equals_pillow(w, h, sub):
    for content, quality, restart, optimize in C.GRID_COMBOS:
        jpg = C.stream(w, h, sub, restart, 0, quality, content, optimize)
        assert CR.sampling(jpg) == {"420": (2, 2), "422": (2, 1), "444": (1, 1)}[sub]
        got, pil = CR.decode(jpg), C.pillow(jpg)
        assert got.shape == pil.shape == (h, w, 3) and got.dtype == pil.dtype
        assert np.array_equal(got, pil), f"{content} q{quality} {restart}: {np.count_nonzero(got != pil)} bytes differ"


def test_reference_decoder_without_dht_equals_pillow():
    for sub in ("420", "422", "444"):
        jpg = C.strip_dht(C.stream(33, 17, sub, "dri7"))
        assert not C.dht_segments(jpg)
        assert np.array_equal(CR.decode(jpg), C.pillow(jpg))
        assert np.array_equal(C.pillow(jpg), C.pillow(C.stream(33, 17, sub, "dri7")))


def _host_handle(N, flags, w=4096, h=4096):
    h_ = ctypes.c_void_p()
    N.check(N.lib().dvc_jpegd_create(w, h, 1, -1, None, flags, ctypes.byref(h_)))
    return h_


def _set_header(N, h, data):
    n, w, hh, fmt = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = N.lib().dvc_jpegd_set_header(h, data, len(data), ctypes.byref(n), ctypes.byref(w), ctypes.byref(hh),
                                      ctypes.byref(fmt))
    return rc, n.value, w.value, hh.value, fmt.value


def test_header_acceptance_with_and_without_the_flag():
    from PIL import Image
    from dvc_amd import _native as N
    assert N.DVC_FLAG_JPEGD_CAMERA == 0x100
    s444, s422, s420 = (C.stream(70, 37, sub) for sub in ("444", "422", "420"))
    nodht = {sub: C.strip_dht(C.stream(70, 37, sub)) for sub in ("420", "422", "444")}
    buf = io.BytesIO()
    Image.fromarray(np.zeros((37, 70, 3), np.uint8)).save(buf, "JPEG", quality=75, subsampling=1, progressive=True)
    progressive = buf.getvalue()
    rgb = C.rgb_stream()
    assert b"Adobe" in rgb[:64] and b"JFIF" not in rgb[:64]
    assert [c[0] for c in R.parse(rgb)["comps"]] == [82, 71, 66]
    cam, plain = _host_handle(N, N.DVC_FLAG_JPEGD_CAMERA), _host_handle(N, 0)
    try:
        for jpg in (s444, s422, s420, *nodht.values(), C.gray_stream(70, 37), C.strip_dht(C.gray_stream(70, 37))):
            start = R.parse(jpg)["start"]
            fmt = N.FMT_GRAY if len(R.parse(jpg)["comps"]) == 1 else N.FMT_BGR
            assert _set_header(N, cam, jpg) == (N.DVC_OK, start, 70, 37, fmt)
            assert _set_header(N, cam, jpg[:start]) == (N.DVC_OK, start, 70, 37, fmt)     # the header alone
        # refused with the flag, at set_header
        for bad in (rgb, progressive, C.patch_sampling(s422, 0x12), C.patch_sampling(s422, 0x41),
                    C.patch_sampling(s422, 0x14), C.patch_sampling(s422, 0x42)):
            assert _set_header(N, cam, bad)[0] == N.DVC_E_UNSUPPORTED
        all22 = bytearray(s420)                                   # every component 2x2
        sof = next(a for m, a, b in C.segments(s420) if m == 0xC0)
        all22[sof + 4 + 10] = all22[sof + 4 + 13] = 0x22
        assert _set_header(N, cam, bytes(all22))[0] == N.DVC_E_UNSUPPORTED
        # RGB by the component ids alone: the Adobe segment removed
        ids_only = bytearray(rgb[:2])
        for m, a, b in C.segments(rgb):
            if m != 0xEE:
                ids_only += rgb[a:b]
        assert b"Adobe" not in ids_only
        assert _set_header(N, cam, bytes(ids_only))[0] == N.DVC_E_UNSUPPORTED
        # a JFIF stream with 4:4:4 is YCbCr whatever else it says
        assert _set_header(N, cam, s444)[0] == N.DVC_OK
        # without the flag: today's statuses
        assert _set_header(N, plain, s420)[0] == N.DVC_OK
        for jpg in (s444, s422, rgb, progressive, nodht["444"], nodht["422"]):
            assert _set_header(N, plain, jpg)[0] == N.DVC_E_UNSUPPORTED
        assert _set_header(N, plain, nodht["420"])[0] == N.DVC_E_INVALID      # "scan names a missing Huffman table"
        assert _set_header(N, plain, C.strip_dht(C.gray_stream(70, 37)))[0] == N.DVC_E_INVALID
    finally:
        N.lib().dvc_jpegd_destroy(cam)
        N.lib().dvc_jpegd_destroy(plain)


def test_camera_handle_refuses_a_frame_past_the_31_bit_bound():
    """3 * up(W,16) * up(H,16) int16 coefficients must stay below 2^31 bytes: 18912 x 18912 passes,
    18928 x 18912 is refused; a default handle (half the buffers) takes both."""
    from dvc_amd import _native as N
    assert 3 * 18912 * 18912 * 2 <= 0x7FFFFFFF < 3 * 18928 * 18912 * 2 and 18912 % 16 == 0 and 18928 % 16 == 0
    for w, flags, want in ((18912, N.DVC_FLAG_JPEGD_CAMERA, N.DVC_OK), (18928, N.DVC_FLAG_JPEGD_CAMERA, N.DVC_E_UNSUPPORTED),
                           (18913, N.DVC_FLAG_JPEGD_CAMERA, N.DVC_E_UNSUPPORTED), (18928, 0, N.DVC_OK)):
        h = ctypes.c_void_p()
        assert N.lib().dvc_jpegd_create(w, 18912, 1, -1, None, flags, ctypes.byref(h)) == want, (w, flags)
        if h:
            N.lib().dvc_jpegd_destroy(h)


def test_annex_k_arrays_are_libjpegs_default_dht_segments():
    text = open(os.path.join(ROOT, "dynamic-video-compression-surveillance_amd", "csrc", "jpeg_std_tables.h")).read()

    def array(name):
        m = re.search(r"%s\[(\d+)\] = \{([^}]*)\}" % name, text)
        vals = [int(v, 0) for v in m.group(2).replace("\n", " ").split(",")]
        assert len(vals) == int(m.group(1))
        return bytes(vals)

    dht = C.dht_segments(C.stream(70, 37, "420"))                # default tables: not optimised
    assert sorted(dht) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for key, name in {(0, 0): "DcLuma", (0, 1): "DcChroma", (1, 0): "AcLuma", (1, 1): "AcChroma"}.items():
        assert dht[key] == (array(f"kJpegStd{name}Bits"), array(f"kJpegStd{name}Vals")), name


HOST_GOOD = [(70, 37, "422", "row"), (70, 37, "444", "dri7"), (33, 17, "422", "dri1"), (33, 17, "444", "none"),
             (3, 5, "422", "none"), (70, 37, "420", "dri7")]


def test_host_program_under_sanitizers_camera_mode(tmp_path):
    """The kernels' serial routines for the camera set, compiled for the host with ASan and
    UBSan into a stand-alone program: the reference's bytes on the good streams (one of them
    without DHT segments), status -1, no output and a clean exit on the damaged ones."""
    exe = tmp_path / "jpegd_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), os.path.join(ROOT, "tools", "jpegd_host_check.cc")], check=True)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    good = [C.stream(*c) for c in HOST_GOOD] + [C.strip_dht(C.stream(70, 37, "422", "dri7"))]
    for i, jpg in enumerate(good):
        (src / f"good{i}.jpg").write_bytes(jpg)
    bad = []
    for sub in ("422", "444"):
        for kind in C.DAMAGE:
            hdr, data = C.damaged(sub, kind)
            (src / f"bad_{sub}_{kind}.jpg").write_bytes(hdr + data[1])
            bad.append(f"bad_{sub}_{kind}")
            with pytest.raises(CR.Damaged):
                CR.decode(hdr + data[1])
    (src / "bad_rgb.jpg").write_bytes(C.rgb_stream())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(src), str(dst), "camera"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines()}
    for i, jpg in enumerate(good):
        want = CR.decode(jpg)
        assert lines[f"good{i}"] == [want.shape[1], want.shape[0], 3, 0], i
        got = np.fromfile(dst / f"good{i}.raw", np.uint8).reshape(want.shape)
        assert np.array_equal(got, want), i
    for name in bad:
        assert lines[name][3] == -1 and not (dst / f"{name}.raw").exists(), name
    assert lines["bad_rgb"][3] == -5 and not (dst / "bad_rgb.raw").exists()
    # without the third argument the program is the default handle's: it refuses the same streams
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines()}
    assert lines["good0"][3] == -5 and lines["good5"][3] == 0 and lines["good6"][3] == -5


def _read_all(r):
    from dvc_amd import video_io
    assert r.isOpened()
    props = [r.get(p) for p in (video_io.CAP_PROP_FPS, video_io.CAP_PROP_FRAME_WIDTH, video_io.CAP_PROP_FRAME_HEIGHT,
                                video_io.CAP_PROP_FRAME_COUNT)]
    frames = []
    while True:
        ok, f = r.read()
        if not ok:
            assert f is None
            break
        frames.append(f)
    assert r.read() == (False, None)
    r.release()
    assert not r.isOpened()
    return frames, props


def test_raw_stream_reader_pillow(tmp_path, monkeypatch):
    from dvc_amd import video_io
    monkeypatch.setenv("DVC_MJPEG_DECODE", "pillow")
    monkeypatch.setenv("DVC_MJPEG_FPS", "12.5")
    samples = [C.stream(70, 37, "422", "row", 0), C.with_app1(C.stream(70, 37, "422", "row", 1)),
               C.stream(70, 37, "444", "none", 2), C.strip_dht(C.stream(70, 37, "422", "dri7", 0))]
    cut = C.stream(70, 37, "422", "row", 2)
    blob = b"\x00\x01junk" + samples[0] + b"--boundary\r\nContent-Type: image/jpeg\r\n\r\n" + samples[1] + \
        samples[2] + b"\xff\x00\xff" + samples[3] + cut[:len(cut) // 2]
    path = tmp_path / "cam.mjpeg"
    path.write_bytes(blob)
    r = video_io.MjpegStreamReader(str(path))
    got = []
    while True:
        ok, s = r.read_sample()
        if not ok:
            break
        got.append(s)
    assert got == samples                                       # the APP1's SOI / EOI split nothing
    r.release()
    frames, props = _read_all(video_io.open_source(str(path)))
    assert props == [12.5, 70.0, 37.0, 4.0] and len(frames) == 4
    for f, s in zip(frames, samples):
        assert np.array_equal(f, C.pillow(s))
    # .mjpg routes too; the default rate is 25; a file without an image does not open
    monkeypatch.delenv("DVC_MJPEG_FPS")
    p2 = tmp_path / "cam.mjpg"
    p2.write_bytes(samples[0])
    r = video_io.open_source(str(p2))
    assert isinstance(r, video_io.MjpegStreamReader) and r.get(video_io.CAP_PROP_FPS) == 25.0
    r.release()
    p3 = tmp_path / "empty.mjpeg"
    p3.write_bytes(b"no image here \xff\xd8\xff")
    assert not video_io.MjpegStreamReader(str(p3)).isOpened()
    # a sample of another size ends the stream
    p4 = tmp_path / "sizes.mjpeg"
    p4.write_bytes(samples[0] + C.stream(33, 17, "422") + samples[0])
    frames, props = _read_all(video_io.MjpegStreamReader(str(p4)))
    assert props[3] == 3.0 and len(frames) == 1


def test_avi_reader_pillow(tmp_path, monkeypatch):
    from dvc_amd import video_io
    monkeypatch.setenv("DVC_MJPEG_DECODE", "pillow")
    samples = [C.strip_dht(C.stream(96, 64, "422", "row", v)) for v in range(6)]
    samples[1] += b"\0" * (1 - len(samples[1]) % 2)             # an odd-sized video chunk (bytes after EOI)
    assert len(samples[1]) % 2 == 1
    path = tmp_path / "cam.avi"
    path.write_bytes(C.avi(samples, 96, 64))
    assert b"idx1" not in path.read_bytes() and b"JUNK" in path.read_bytes()
    r = video_io.AviMjpegReader(str(path))
    got = []
    while True:
        ok, s = r.read_sample()
        if not ok:
            break
        got.append(s)
    r.release()
    assert got == samples
    frames, props = _read_all(video_io.open_source(str(path)))
    assert props == [30000 / 1001, 96.0, 64.0, 6.0] and len(frames) == 6
    for f, s in zip(frames, samples):
        assert np.array_equal(f, C.pillow(s))
    # refused: no MJPG stream, a second RIFF segment, not an AVI
    for name, blob in (("other.avi", C.avi(samples, 96, 64, fourcc=b"H264")), ("big.avi", C.avi(samples, 96, 64, avix=True)),
                       ("not.avi", b"RIFF\x04\0\0\0WAVE")):
        (tmp_path / name).write_bytes(blob)
        assert not video_io.AviMjpegReader(str(tmp_path / name)).isOpened(), name
    # upper-case fourcc, no audio stream (the video stream is 00), no LIST rec
    (tmp_path / "plain.avi").write_bytes(C.avi(samples[:3], 96, 64, 25, 1, b"MJPG", audio=False, rec=False, junk=False))
    frames, props = _read_all(video_io.AviMjpegReader(str(tmp_path / "plain.avi")))
    assert props == [25.0, 96.0, 64.0, 3.0] and len(frames) == 3
