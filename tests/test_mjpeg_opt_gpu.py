"""GPU: dvc_jpeg_encode with DVC_FLAG_JPEG_OPT_HUFFMAN byte for byte against
tests/mjpeg_opt_ref.py — the independent restatement of DESIGN.md "Optimised
Huffman tables" whose streams tests/test_mjpeg_opt.py hands to Pillow — on the
frames of tests/mjpeg_cases.py; the table builder alone on the count vectors
tools/jpeg_huff_host_check.cc has run under the host sanitizers; both decoders
on the optimised samples; and the FD driver writing optimised .mp4 files."""
import ctypes
import io
import os

import numpy as np
import pytest

from tests import mjpeg_cases as C
from tests import mjpeg_opt_ref as O
from tests import mjpeg_ref as R

pytestmark = pytest.mark.gpu


def _handle(N, W, H, fmt, quality, max_batch, stream=None, flags=0):
    h = ctypes.c_void_p()
    N.check(N.lib().dvc_jpeg_create(W, H, fmt, quality, max_batch, 0, stream, flags, ctypes.byref(h)))
    return h


def _stride(N, W, H, fmt):
    b = ctypes.c_size_t()
    N.check(N.lib().dvc_jpeg_bound(W, H, fmt, ctypes.byref(b)))
    return int(b.value) + N.JPEG_OPT_PREFIX_MAX


def _header(N, h):
    n = ctypes.c_size_t()
    N.check(N.lib().dvc_jpeg_header(h, None, 0, ctypes.byref(n)))
    buf = (ctypes.c_uint8 * n.value)()
    N.check(N.lib().dvc_jpeg_header(h, buf, n.value, ctypes.byref(n)))
    return bytes(buf)


def _encode_host(N, frames, quality, max_batch):
    """frames: (n, H, W, 3) or (n, H, W) -> (header, [frame bytes]) through host pointers."""
    f = np.ascontiguousarray(frames)
    n, H, W = f.shape[:3]
    fmt = N.FMT_BGR if f.ndim == 4 else N.FMT_GRAY
    h = _handle(N, W, H, fmt, quality, max_batch, None, N.DVC_FLAG_JPEG_OPT_HUFFMAN)
    stride = _stride(N, W, H, fmt)
    out, sizes = np.full((n, stride), 0xA5, np.uint8), np.zeros(n, np.uint32)
    try:
        header = _header(N, h)
        N.check(N.lib().dvc_jpeg_encode(h, f.ctypes.data, f[0][0].nbytes, f[0].nbytes, n, out.ctypes.data, stride,
                                        sizes.ctypes.data))
    finally:
        N.lib().dvc_jpeg_destroy(h)
    assert all((out[i, int(sizes[i]):] == 0xA5).all() for i in range(n))      # nothing past a frame's bytes
    return header, [out[i, :int(sizes[i])].tobytes() for i in range(n)]


def _same(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} bytes, reference {len(want)}"
    assert got == want, f"{what}: first difference at byte {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)}"


def _check(N, name, variants, max_batch, gray=False, cases=C.ALL):
    frames = np.stack([C.frame(name, v)[..., 1] if gray else C.frame(name, v) for v in variants])
    header, got = _encode_host(N, frames, cases[name][1], max_batch)
    want_header, want = O.encode([C.reference(name, v, gray) for v in variants], max_batch)
    assert header == want_header
    for t in range(len(variants)):
        _same(got[t], want[t], f"{name} frame {t}")
    return got


@pytest.mark.parametrize("name", list(C.ALL))
def test_group_of_one_matches_reference_bytes(gpu_lib, name):
    _check(gpu_lib._native, name, (0,), 1)
    g = O.case_group(name)
    if name == "const16":       # EOB alone in both AC tables: one symbol, a 1-bit code
        assert all(g["counts"][k][0] > 0 and sum(g["counts"][k]) == g["counts"][k][0] for k in (1, 3))
        assert O.code_lengths(g["counts"][1])[:2] == ([1] + [0] * 15, [0])
    if name == "zz63":
        assert g["counts"][1][0xF0] == 12                           # three ZRLs a luma block
    if name == "alt8":
        assert g["counts"][0][11] > 0                               # DC size 11
    if name == "noise16_q100":  # Q = 1 on noise: nearly every luma coefficient is coded and no block ends in EOB
        assert g["counts"][1][0x00] == 0 and sum(g["counts"][1]) > 60 * 4


def test_three_frames_in_two_groups(gpu_lib):
    """max_batch 2: frames 0 and 1 share their tables, frame 2 has its own."""
    got = _check(gpu_lib._native, "mixed130x50_q20", (0, 1, 0), 2)
    a, b = O.case_group("mixed130x50_q20", (0, 1))["prefix"], O.case_group("mixed130x50_q20", (0,))["prefix"]
    assert a != b and got[0].startswith(a) and got[1].startswith(a) and got[2].startswith(b)


@pytest.mark.parametrize("name", [C.GRAY_CASE, "tiny5x3", "wide1120x32"])
def test_gray_matches_reference_bytes(gpu_lib, name):
    got = _check(gpu_lib._native, name, (0, 1), 2, gray=True)
    assert got[0][4] == 0x00 and got[0][:2] == b"\xff\xc4"          # tables 00 and 10 alone
    assert len(O.case_group(name, (0, 1), True)["prefix"]) - 10 == int.from_bytes(got[0][2:4], "big") + 2


def test_dense_segment_takes_a_second_pack_chunk(gpu_lib):
    _check(gpu_lib._native, "dense176x16_q100", (0,), 1, cases=C.SIZE_CASES)
    counts = O.case_group("dense176x16_q100")["counts"]
    assert sum(counts[1]) > 60 * 4 * 11 and counts[1][0x00] == 0       # 66 blocks a segment, nearly every coefficient coded


def test_257_segments(gpu_lib):
    """The histogram's atomics cross 257 workgroups; k_jpeg_gather sums its second trip behind a prefix."""
    _check(gpu_lib._native, "tall16x4112", (0,), 1, cases=C.SIZE_CASES)


@pytest.mark.parametrize("pad", [5, 6])
def test_device_pointers_padded_pitch_caller_stream(gpu_lib, pad):
    import torch
    N = gpu_lib._native
    name, variants = "noise70x37_q90", (0, 1, 0)
    H, W = C.frame(name).shape[:2]
    pitch = 3 * W + pad
    host = np.full((3, H, pitch), 0x5A, np.uint8)
    for t, v in enumerate(variants):
        host[t, :, :3 * W] = C.frame(name, v).reshape(H, 3 * W)
    stride = _stride(N, W, H, N.FMT_BGR)
    s = torch.cuda.Stream()
    h = _handle(N, W, H, N.FMT_BGR, C.CASES[name][1], 2, ctypes.c_void_p(s.cuda_stream),
                N.DVC_FLAG_DEVICE_PTRS | N.DVC_FLAG_JPEG_OPT_HUFFMAN)
    try:
        with torch.cuda.stream(s):
            d_in = torch.from_numpy(host).pin_memory().to("cuda", non_blocking=True)
            d_out = torch.full((3, stride), 0xA5, dtype=torch.uint8, device="cuda")
            d_sizes = torch.zeros(3, dtype=torch.int32, device="cuda")
            N.check(N.lib().dvc_jpeg_encode(h, d_in.data_ptr(), pitch, H * pitch, 3, d_out.data_ptr(), stride,
                                            d_sizes.data_ptr()))
            out = d_out.to("cpu", non_blocking=True)             # copied out on the caller's stream
            sizes = d_sizes.to("cpu", non_blocking=True)
        s.synchronize()
        N.check(N.lib().dvc_jpeg_sync(h))
    finally:
        N.lib().dvc_jpeg_destroy(h)
    out, sizes = out.numpy(), sizes.numpy()
    _, want = O.encode([C.reference(name, v) for v in variants], 2)
    for t in range(3):
        assert int(sizes[t]) == len(want[t])
        _same(out[t, :len(want[t])].tobytes(), want[t], f"frame {t}")
        assert (out[t, len(want[t]):] == 0xA5).all()


def test_overflow_counts_the_prefix(gpu_lib):
    """out_stride one byte short of a frame's prefix + data: DVC_E_NOMEM, the slot untouched, sizes hold the need."""
    import torch
    N = gpu_lib._native
    name = "noise70x37_q90"
    H, W = C.frame(name).shape[:2]
    flat = np.full((H, W, 3), (90, 120, 200), np.uint8)
    frames = np.stack([flat, C.frame(name), flat])
    flat_ref = R.encode(flat, 90)
    _, want = O.encode([flat_ref, C.reference(name), flat_ref], 2)
    stride, guard = len(want[1]) - 1, 64
    assert len(want[0]) < stride and len(want[2]) < stride
    flags = N.DVC_FLAG_JPEG_OPT_HUFFMAN
    h = _handle(N, W, H, N.FMT_BGR, 90, 2, None, flags)
    out, sizes = np.full(3 * stride + guard, 0xA5, np.uint8), np.zeros(3, np.uint32)
    try:
        rc = N.lib().dvc_jpeg_encode(h, frames.ctypes.data, 3 * W, frames[0].nbytes, 3, out.ctypes.data, stride,
                                     sizes.ctypes.data)
        assert rc == N.DVC_E_NOMEM
        assert sizes.tolist() == [len(w) for w in want]
        slots = out[:3 * stride].reshape(3, stride)
        for t in (0, 2):
            assert slots[t, :len(want[t])].tobytes() == want[t] and (slots[t, len(want[t]):] == 0xA5).all()
        assert (slots[1] == 0xA5).all() and (out[3 * stride:] == 0xA5).all()
        sizes[:] = 0                                              # the handle goes on working
        big = np.zeros((3, len(want[1])), np.uint8)
        N.check(N.lib().dvc_jpeg_encode(h, frames.ctypes.data, 3 * W, frames[0].nbytes, 3, big.ctypes.data,
                                        big.shape[1], sizes.ctypes.data))
        assert big[1].tobytes() == want[1]
    finally:
        N.lib().dvc_jpeg_destroy(h)
    h = _handle(N, W, H, N.FMT_BGR, 90, 2, None, flags | N.DVC_FLAG_DEVICE_PTRS)
    try:
        d_in = torch.from_numpy(frames).cuda()
        d_out = torch.full((3 * stride + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        d_sizes = torch.zeros(3, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        N.check(N.lib().dvc_jpeg_encode(h, d_in.data_ptr(), 3 * W, frames[0].nbytes, 3, d_out.data_ptr(), stride,
                                        d_sizes.data_ptr()))
        assert N.lib().dvc_jpeg_sync(h) == N.DVC_E_NOMEM
        assert N.lib().dvc_jpeg_sync(h) == N.DVC_OK               # reported once
        o = d_out.cpu().numpy()
        assert d_sizes.cpu().tolist() == [len(w) for w in want]
        assert (o[stride:2 * stride] == 0xA5).all() and (o[3 * stride:] == 0xA5).all()
        assert o[:len(want[0])].tobytes() == want[0]
    finally:
        N.lib().dvc_jpeg_destroy(h)


@pytest.mark.parametrize("name", list(O.count_vectors()))
def test_table_builder_on_count_vectors(gpu_lib, name):
    """dvc_jpeg_opt_tables: the only way to the paths deeper than 16 and than 32 on the device."""
    N = gpu_lib._native
    nc, counts = O.count_vectors()[name]
    with N.JpegEncoder(16, 16, is_color=nc == 3, optimize=True) as enc:
        _same(enc.tables(counts), O.dht_segment(counts), name)
        _same(enc.tables(counts), O.dht_segment(counts), name + " again")      # and the handle's state is clean


def test_table_builder_refusals(gpu_lib):
    N = gpu_lib._native
    ok = [[0] * 256 for _ in range(4)]
    ok[0][0] = ok[1][0] = 1
    with N.JpegEncoder(16, 16, is_color=True, optimize=True) as enc:
        assert enc.tables(ok) == O.dht_segment(ok)
        for k, s in ((0, 12), (2, 200), (1, 0x0B), (1, 0x10), (3, 0xE0), (1, 0xFF)):
            bad = [list(r) for r in ok]
            bad[k][s] = 1
            with pytest.raises(N.DvcError) as e:
                enc.tables(bad)
            assert e.value.code == N.DVC_E_INVALID, (k, s)
        with pytest.raises(N.DvcError) as e:
            enc.tables([[0] * 256 for _ in range(4)])
        assert e.value.code == N.DVC_E_INVALID
        n = ctypes.c_size_t()
        c = np.asarray(ok, np.uint64)
        N.check(N.lib().dvc_jpeg_opt_tables(enc._h, c.ctypes.data_as(N._PU64), None, 0, ctypes.byref(n)))
        small = (ctypes.c_uint8 * 8)()
        assert n.value == len(O.dht_segment(ok))
        assert N.lib().dvc_jpeg_opt_tables(enc._h, c.ctypes.data_as(N._PU64), small, 8, ctypes.byref(n)) == N.DVC_E_NOMEM
    with N.JpegEncoder(16, 16, is_color=False, optimize=True) as enc:
        bad = [list(r) for r in ok]
        bad[2][0] = 1                                             # a class 1 count on a one-component handle
        with pytest.raises(N.DvcError) as e:
            enc.tables(bad)
        assert e.value.code == N.DVC_E_INVALID
    with N.JpegEncoder(16, 16, is_color=True) as enc:
        with pytest.raises(N.DvcError) as e:
            enc.tables(ok)
        assert e.value.code == N.DVC_E_STATE


def test_handle_without_the_flag_gives_the_fixed_stream(gpu_lib):
    N = gpu_lib._native
    name = "mixed130x50_q20"
    H, W = C.frame(name).shape[:2]
    with N.JpegEncoder(W, H, True, C.ALL[name][1], max_batch=2) as enc:
        got = enc.encode(np.stack([C.frame(name, v) for v in (0, 1, 0)]))
        assert enc.header == C.reference(name)["header"] and enc.bound + N.JPEG_OPT_PREFIX_MAX == _stride(N, W, H, N.FMT_BGR)
    for t, v in enumerate((0, 1, 0)):
        _same(got[t], C.reference(name, v)["stream"], f"frame {t}")


def _pillow_bgr(sample):
    from PIL import Image
    im = Image.open(io.BytesIO(sample))
    return np.asarray(im) if im.mode == "L" else np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


@pytest.mark.parametrize("name,gray", [("mixed130x50_q20", False), ("noise70x37_q90", True)])
def test_both_decoders_read_the_fixed_stream_s_pixels(gpu_lib, name, gray):
    N = gpu_lib._native
    H, W = C.frame(name).shape[:2]
    frames = np.stack([C.frame(name, v)[..., 1] if gray else C.frame(name, v) for v in (0, 1, 0)])
    samples = {}
    for optimize in (False, True):
        with N.JpegEncoder(W, H, not gray, C.ALL[name][1], max_batch=2, optimize=optimize) as enc:
            assert enc.bound == _stride(N, W, H, enc.fmt) - (0 if optimize else N.JPEG_OPT_PREFIX_MAX)
            samples[optimize] = [enc.header + f for f in enc.encode(frames)]
    assert sum(map(len, samples[True])) != sum(map(len, samples[False]))
    with N.JpegDecoder(W, H, max_batch=4) as dec:
        fixed = dec.decode(samples[False])
        opt = dec.decode(samples[True])                            # two headers: the decoder parses twice
    for t in range(3):
        assert fixed[t] is not None and opt[t] is not None and np.array_equal(opt[t], fixed[t]), t
        assert np.array_equal(_pillow_bgr(samples[True][t]), _pillow_bgr(samples[False][t])), t
        assert np.array_equal(opt[t], _pillow_bgr(samples[True][t])), t


def test_fd_driver_writes_optimised_files(gpu_lib, tmp_path, monkeypatch):
    """process_single_video_fd on a Y4M file with DVC_VIDEO_SINK=mjpeg, once with the fixed and once
    with optimised tables: the GPU reader returns the same frames from both, and the compressed
    video of the optimised run is the smaller file."""
    from dvc_amd import video_io
    from dvc_amd.frame_differencing import process_single_video_fd
    from dvc_amd.synthetic import clip
    N = gpu_lib._native
    W, H, n = 320, 192, 12
    src = str(tmp_path / "cam.y4m")
    with open(src, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg\n" % (W, H))
        for fr in N.bgr_to_i420(clip(W, H, n, seed=3)):
            f.write(b"FRAME\n" + fr.tobytes())
    monkeypatch.setenv("DVC_VIDEO_SINK", "mjpeg")
    monkeypatch.setenv("DVC_MJPEG_DECODE", "gpu")

    def frames_of(path):
        r = video_io.Mp4MjpegReader(path, batch=8)
        assert r.isOpened(), path
        out = []
        while True:
            ok, fr = r.read()
            if not ok:
                break
            out.append(fr)
        r.release()
        return out

    for mode in ("fixed", "optimized"):
        monkeypatch.setenv("DVC_VIDEO_HUFFMAN", mode)
        process_single_video_fd(src, str(tmp_path / mode))
    for name in ("dilated_motion_mask_video.mp4", "compressed_final_video.mp4"):
        a, b = (frames_of(str(tmp_path / mode / "cam" / name)) for mode in ("fixed", "optimized"))
        assert len(a) == len(b) == n - 1, name
        for t in range(n - 1):
            assert np.array_equal(a[t], b[t]), f"{name} frame {t}"
    sizes = {mode: os.path.getsize(tmp_path / mode / "cam" / "compressed_final_video.mp4") for mode in ("fixed", "optimized")}
    print("compressed_final_video.mp4:", sizes)
    assert sizes["optimized"] < sizes["fixed"]
