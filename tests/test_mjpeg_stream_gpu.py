"""GPU: dvc_jpeg_encode_stream (include/dvc_jpeg_stream.h) — complete samples back
to back — against dvc_jpeg_encode of a second handle with the same parameters:
every sample is that handle's header followed by its bytes for the frame, in
both Huffman modes, with device pointers on a caller's stream and with host
pointers, across launch groups, at any byte alignment, and at a ``cap`` on
either side of the last sample's end. Frames are those of tests/mjpeg_cases.py.
The offset arithmetic alone runs under the host sanitizers in
tests/test_mjpeg_stream.py."""
import ctypes

import numpy as np
import pytest

from tests import mjpeg_cases as C

pytestmark = pytest.mark.gpu

FILL = 0xA5


def five_frames():
    """Five different 70x37 colour frames: noise and crops of the 130x50 surveillance frame."""
    noise, mixed = "noise70x37_q90", "mixed130x50_q20"
    return np.stack([C.frame(noise, 0), C.frame(mixed, 0)[:37, :70], C.frame(noise, 1), C.frame(mixed, 1)[:37, :70],
                     C.frame(mixed, 0)[13:, 60:]])


def _reference(N, frames, quality, max_batch, optimize):
    """[header + frame bytes] from dvc_jpeg_encode on a handle of its own."""
    with N.JpegEncoder(frames.shape[2], frames.shape[1], frames.ndim == 4, quality, max_batch, 0, optimize) as enc:
        return [enc.header + b for b in enc.encode(frames)]


def _padded(frames, pitch):
    n, H = frames.shape[:2]
    rows = frames.reshape(n, H, -1)
    out = np.full((n, H, pitch), 0x5A, np.uint8)
    out[:, :, :rows.shape[2]] = rows
    return out


def _stream(N, frames, quality, max_batch, optimize, mode, cap=None, guard=0, pitch=0, enc=None):
    """Run encode_stream; (out bytes incl. guard, offsets, DvcError code or 0). mode: "device"
    (torch tensors, the caller's stream) or "host" (numpy)."""
    import torch
    n = frames.shape[0]
    src = _padded(frames, pitch) if pitch else np.array(frames)
    W, H, color = frames.shape[2], frames.shape[1], frames.ndim == 4
    if cap is None:
        cap = n * (N.JpegEncoder(W, H, color, quality, 1, -1, optimize).bound + 1024)
    code = 0
    if mode == "host":
        e = enc or N.JpegEncoder(W, H, color, quality, max_batch, 0, optimize)
        out, offs = np.full(cap + guard, FILL, np.uint8), np.full(n + 1, 2 ** 64 - 1, np.uint64)
        try:
            e.encode_stream(src, out[:cap], offs, pitch=pitch)
        except N.DvcError as err:
            code = err.code
    else:
        st = torch.cuda.Stream()
        e = enc or N.JpegEncoder(W, H, color, quality, max_batch, 0, optimize, device_ptrs=True, stream=st.cuda_stream)
        with torch.cuda.stream(st):
            d_in = torch.from_numpy(src).cuda()
            d_out = torch.full((cap + guard,), FILL, dtype=torch.uint8, device="cuda")
            d_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            if enc is not None:   # a handle on a stream of its own: the buffers are ready before it starts
                st.synchronize()
            e.encode_stream(d_in, d_out[:cap], d_offs, pitch=pitch)
            try:
                e.sync()
            except N.DvcError as err:
                code = err.code
            out, offs = d_out.cpu().numpy(), d_offs.cpu().numpy().astype(np.uint64)
    if enc is None:
        e.close()
    return out, [int(v) for v in offs], code


def _samples(out, offs):
    return [out[a:b].tobytes() for a, b in zip(offs, offs[1:])]


@pytest.mark.parametrize("mode", ["device", "host"])
@pytest.mark.parametrize("gray", [False, True], ids=["colour16x16", "gray8x8"])
def test_one_frame_one_segment(gpu_lib, gray, mode):
    N = gpu_lib._native
    f = C.frame("noise16_q100")
    frames = (f[:8, :8, 1] if gray else f)[None]
    want = _reference(N, frames, 100, 8, False)
    out, offs, code = _stream(N, frames, 100, 8, False, mode, guard=64)
    assert code == 0 and offs == [0, len(want[0])]
    assert _samples(out, offs) == want and (out[offs[1]:] == FILL).all()


@pytest.mark.parametrize("pitch", [0, 236], ids=["packed", "pitch236"])
@pytest.mark.parametrize("mode", ["device", "host"])
@pytest.mark.parametrize("optimize", [False, True], ids=["fixed", "optimized"])
def test_five_frames_in_three_launch_groups(gpu_lib, optimize, mode, pitch):
    """max_batch 2, n 5: the carry crosses two group boundaries, and with optimised
    tables every group has a prefix of its own. Sample starts fall on any alignment."""
    N = gpu_lib._native
    frames = five_frames()
    want = _reference(N, frames, 90, 2, optimize)
    out, offs, code = _stream(N, frames, 90, 2, optimize, mode, guard=64, pitch=pitch)
    assert code == 0 and offs[0] == 0
    assert [b - a for a, b in zip(offs, offs[1:])] == [len(w) for w in want]
    for t, (got, w) in enumerate(zip(_samples(out, offs), want)):
        assert got == w, f"sample {t}"
    assert (out[offs[-1]:] == FILL).all()
    assert len({o % 4 for o in offs[:-1]}) >= 3, offs
    if optimize:   # three table groups: the prefix behind the short header differs
        hl = len(N.JpegEncoder(70, 37, True, 90, 2, -1, True).header)
        assert all(w[hl:hl + 2] == b"\xff\xc4" for w in want)
        firsts = [w[hl:hl + 2 + int.from_bytes(w[hl + 2:hl + 4], "big")] for w in want]      # the DHT segment
        assert firsts[0] == firsts[1] and firsts[2] == firsts[3] and len({firsts[0], firsts[2], firsts[4]}) == 3


@pytest.mark.parametrize("mode", ["device", "host"])
@pytest.mark.parametrize("optimize", [False, True], ids=["fixed", "optimized"])
def test_cap_on_either_side_of_the_last_sample_s_end(gpu_lib, optimize, mode):
    N = gpu_lib._native
    frames = five_frames()
    want = _reference(N, frames, 90, 2, optimize)
    total = sum(len(w) for w in want)
    dev = dict(device_ptrs=True) if mode == "device" else {}
    with N.JpegEncoder(70, 37, True, 90, 2, 0, optimize, **dev) as enc:
        out, offs, code = _stream(N, frames, 90, 2, optimize, mode, cap=total, guard=64, enc=enc)
        assert code == 0 and offs[-1] == total and _samples(out, offs) == want
        assert (out[total:] == FILL).all()
        out, short, code = _stream(N, frames, 90, 2, optimize, mode, cap=total - 1, guard=64, enc=enc)
        assert code == N.DVC_E_NOMEM
        assert short == offs                                         # the needed places of all five
        assert _samples(out, short[:-1]) == want[:-1]                # the four before it are intact
        assert (out[short[-2]:] == FILL).all()                       # the last is not written, the guard untouched
        assert len(out) == total - 1 + 64
        out, again, code = _stream(N, frames, 90, 2, optimize, mode, cap=total, guard=64, enc=enc)
        assert code == 0 and again == offs and _samples(out, again) == want


def test_no_frames_null_arguments_and_a_host_only_handle(gpu_lib):
    """The codes of dvc_jpeg_encode for the same misuse."""
    N = gpu_lib._native
    L = N.lib()
    frames = np.ascontiguousarray(five_frames()[:1])
    out, offs, sizes = np.zeros(1 << 16, np.uint8), np.full(2, 7, np.uint64), np.zeros(1, np.uint32)
    row, fs = 3 * 70, 3 * 70 * 37

    def both(h, f, n, o, last_stream, last_encode):
        a = L.dvc_jpeg_encode_stream(h, f, row, fs, n, o, out.size, last_stream)
        b = L.dvc_jpeg_encode(h, f, row, fs, n, o, out.size, last_encode)
        assert a == b
        return a

    with N.JpegEncoder(70, 37, True, 90, 2) as enc:
        h, f, o = enc._h, frames.ctypes.data, out.ctypes.data
        assert both(h, f, 0, o, offs.ctypes.data, sizes.ctypes.data) == N.DVC_OK and offs[0] == 0
        assert both(h, f, -1, o, offs.ctypes.data, sizes.ctypes.data) == N.DVC_E_INVALID
        assert both(None, f, 1, o, offs.ctypes.data, sizes.ctypes.data) == N.DVC_E_INVALID
        assert both(h, None, 1, o, offs.ctypes.data, sizes.ctypes.data) == N.DVC_E_INVALID
        assert both(h, f, 1, None, offs.ctypes.data, sizes.ctypes.data) == N.DVC_E_INVALID
        assert both(h, f, 1, o, None, None) == N.DVC_E_INVALID
        assert L.dvc_jpeg_encode_stream(h, f, row - 1, fs, 1, o, out.size, offs.ctypes.data) == N.DVC_E_INVALID
        assert both(h, f, 1, o, offs.ctypes.data, sizes.ctypes.data) == N.DVC_OK      # and it still encodes
    with N.JpegEncoder(70, 37, True, 90, 2, device=-1) as enc:
        assert both(enc._h, frames.ctypes.data, 1, out.ctypes.data, offs.ctypes.data, sizes.ctypes.data) == N.DVC_E_STATE
