"""GPU: dvc_jpeg_encode byte for byte against tests/mjpeg_ref.py — an
independent numpy restatement of DESIGN.md "Motion-JPEG stream" whose streams
tests/test_mjpeg.py hands to a decoder that is not ours — on the frames of
tests/mjpeg_cases.py, and the drop-in drivers writing real .mp4 files."""
import ctypes
import io
import os

import numpy as np
import pytest

from tests import mjpeg_cases as C

pytestmark = pytest.mark.gpu


def _handle(N, W, H, fmt, quality, max_batch=2, stream=None, flags=0):
    h = ctypes.c_void_p()
    N.check(N.lib().dvc_jpeg_create(W, H, fmt, quality, max_batch, 0, stream, flags, ctypes.byref(h)))
    return h


def _bound(N, W, H, fmt):
    b = ctypes.c_size_t()
    N.check(N.lib().dvc_jpeg_bound(W, H, fmt, ctypes.byref(b)))
    return int(b.value)


def _encode_host(N, frames, quality, max_batch=2):
    """frames: (n, H, W, 3) or (n, H, W) -> ([stream bytes], sizes) through host pointers."""
    f = np.ascontiguousarray(frames)
    n, H, W = f.shape[:3]
    fmt = N.FMT_BGR if f.ndim == 4 else N.FMT_GRAY
    h = _handle(N, W, H, fmt, quality, max_batch)
    stride = _bound(N, W, H, fmt)
    out, sizes = np.full((n, stride), 0xA5, np.uint8), np.zeros(n, np.uint32)
    try:
        N.check(N.lib().dvc_jpeg_encode(h, f.ctypes.data, f[0][0].nbytes, f[0].nbytes, n, out.ctypes.data, stride,
                                        sizes.ctypes.data))
    finally:
        N.lib().dvc_jpeg_destroy(h)
    assert all((out[i, int(sizes[i]):] == 0xA5).all() for i in range(n))      # nothing past a frame's bytes
    return [out[i, :int(sizes[i])].tobytes() for i in range(n)], sizes


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", list(C.ALL))
def test_encode_matches_reference_bytes(gpu_lib, name, n):
    N = gpu_lib._native
    variants = [0, 1, 0][:n]                                     # max_batch 2: a call of 3 splits
    frames = np.stack([C.frame(name, v) for v in variants])
    got, sizes = _encode_host(N, frames, C.ALL[name][1])
    for t, v in enumerate(variants):
        ref = C.reference(name, v)["stream"]
        assert int(sizes[t]) == len(ref), f"{name} frame {t}: {sizes[t]} bytes, reference {len(ref)}"
        assert got[t] == ref, f"{name} frame {t}: first difference at byte " \
            f"{next(i for i, (a, b) in enumerate(zip(got[t], ref)) if a != b)}"


@pytest.mark.parametrize("name", [C.GRAY_CASE, "wide1120x32", "tiny5x3"])   # 9, 140 (three LDS chunks) and 1 block a row
def test_encode_gray_matches_reference_bytes(gpu_lib, name):
    N = gpu_lib._native
    frames = np.stack([C.frame(name, v)[..., 1] for v in (0, 1, 0)])
    got, sizes = _encode_host(N, frames, C.ALL[name][1])
    for t, v in enumerate((0, 1, 0)):
        ref = C.reference(name, v, True)["stream"]
        assert int(sizes[t]) == len(ref) and got[t] == ref


@pytest.mark.parametrize("pad", [5, 6])       # 3 * 70 + 5: unaligned rows; + 6 = 216: aligned dword loads
def test_encode_device_pointers_padded_pitch_caller_stream(gpu_lib, pad):
    import torch
    N = gpu_lib._native
    name, variants = "noise70x37_q90", (0, 1, 0)
    H, W = C.frame(name).shape[:2]
    pitch = 3 * W + pad
    host = np.full((3, H, pitch), 0x5A, np.uint8)
    for t, v in enumerate(variants):
        host[t, :, :3 * W] = C.frame(name, v).reshape(H, 3 * W)
    stride = _bound(N, W, H, N.FMT_BGR)
    s = torch.cuda.Stream()
    h = _handle(N, W, H, N.FMT_BGR, C.CASES[name][1], 2, ctypes.c_void_p(s.cuda_stream), N.DVC_FLAG_DEVICE_PTRS)
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
    for t, v in enumerate(variants):
        ref = C.reference(name, v)["stream"]
        assert int(sizes[t]) == len(ref) and out[t, :len(ref)].tobytes() == ref
        assert (out[t, len(ref):] == 0xA5).all()


def test_overflow_reports_needed_sizes_and_writes_nothing_past_a_slot(gpu_lib):
    import torch
    N = gpu_lib._native
    name = "noise70x37_q90"
    H, W = C.frame(name).shape[:2]
    flat = np.full((H, W, 3), (90, 120, 200), np.uint8)
    frames = np.stack([flat, C.frame(name), flat])
    ref_flat = _encode_host(N, flat[None], 90)[0][0]
    refs = [ref_flat, C.reference(name)["stream"], ref_flat]
    stride, guard = len(refs[1]) - 1, 64                          # one byte short for the noise frame
    assert len(ref_flat) < stride
    h = _handle(N, W, H, N.FMT_BGR, 90)
    out, sizes = np.full(3 * stride + guard, 0xA5, np.uint8), np.zeros(3, np.uint32)
    try:
        rc = N.lib().dvc_jpeg_encode(h, frames.ctypes.data, 3 * W, frames[0].nbytes, 3, out.ctypes.data, stride,
                                     sizes.ctypes.data)
        assert rc == N.DVC_E_NOMEM
        assert sizes.tolist() == [len(r) for r in refs]           # the needed lengths
        slots = out[:3 * stride].reshape(3, stride)
        for t in (0, 2):                                          # the frames that fit are written
            assert slots[t, :len(refs[t])].tobytes() == refs[t] and (slots[t, len(refs[t]):] == 0xA5).all()
        assert (slots[1] == 0xA5).all() and (out[3 * stride:] == 0xA5).all()
        # the handle goes on working
        sizes[:] = 0
        big = np.zeros((3, len(refs[1])), np.uint8)
        N.check(N.lib().dvc_jpeg_encode(h, frames.ctypes.data, 3 * W, frames[0].nbytes, 3, big.ctypes.data,
                                        big.shape[1], sizes.ctypes.data))
        assert big[1].tobytes() == refs[1]
    finally:
        N.lib().dvc_jpeg_destroy(h)
    # device pointers: the call is asynchronous, the next dvc_jpeg_sync reports it
    h = _handle(N, W, H, N.FMT_BGR, 90, 2, None, N.DVC_FLAG_DEVICE_PTRS)
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
        assert d_sizes.cpu().tolist() == [len(r) for r in refs]
        assert (o[stride:2 * stride] == 0xA5).all() and (o[3 * stride:] == 0xA5).all()
        assert o[:len(refs[0])].tobytes() == refs[0]
    finally:
        N.lib().dvc_jpeg_destroy(h)


def _samples(path):
    from dvc_amd import video_io
    r = video_io.Mp4MjpegReader(path)
    assert r.isOpened(), path
    out = []
    while True:
        ok, data = r.read_sample()
        if not ok:
            break
        out.append(data)
    fps, size = r.get(video_io.CAP_PROP_FPS), (int(r.W), int(r.H))
    r.release()
    return out, fps, size


def test_drop_in_drivers_write_real_mp4(gpu_lib, tmp_path, monkeypatch):
    """The FD and OF drivers with DVC_VIDEO_SINK=mjpeg on a 64x48 synthetic clip:
    .mp4 files whose every sample Pillow decodes, the right frame counts, files
    smaller than their raw frames, and a reduction performance_analysis can report."""
    from PIL import Image
    from dvc_amd import performance_analysis as pa
    from dvc_amd.frame_differencing import process_single_video_fd
    from dvc_amd.motion_compression_opt import process_single_video_of
    monkeypatch.setenv("DVC_VIDEO_SINK", "mjpeg")
    n, W, H = 12, 64, 48
    src = f"synthetic://{W}x{H}?frames={n}&seed=3&fps=25"
    fd_dir, of_dir = tmp_path / "fd", tmp_path / "of"
    process_single_video_fd(src, str(fd_dir))
    process_single_video_of(src, str(of_dir))
    files = [(fd_dir / f"{W}x{H}" / "dilated_motion_mask_video.mp4", "RGB"),
             (fd_dir / f"{W}x{H}" / "compressed_final_video.mp4", "RGB"),
             (of_dir / f"{W}x{H}" / "overlay.mp4", "RGB"), (of_dir / f"{W}x{H}" / "mask.mp4", "L"),
             (of_dir / f"{W}x{H}" / "compressed.mp4", "RGB")]
    for path, mode in files:
        samples, fps, size = _samples(str(path))
        assert len(samples) == n - 1 and fps == 25.0 and size == (W, H), path
        for s in samples:
            im = Image.open(io.BytesIO(s))
            im.load()
            assert im.size == (W, H) and im.convert(mode).mode == mode and (mode != "L" or im.mode == "L")
        raw = (n - 1) * W * H * (3 if mode == "RGB" else 1)
        assert os.path.getsize(path) < raw, path
    for d in (fd_dir, of_dir):
        rows = pa.collect(str(d))
        assert len(rows) == 1 and rows[0]["original_size_bytes"] > 0 and rows[0]["compressed_size_bytes"] > 0
        assert rows[0]["reduction_percentage"] != 0
        assert rows[0]["video_duration_seconds"] == pytest.approx((n - 1) / 25.0)
