"""GPU: the host plumbing the six handles share (csrc/host_common.h), through
the handles, where no other GPU test runs a branch of it.

* stage_rows_h2d (host frames up into rows of ip bytes) through dvc_jpeg_encode,
  whose other host tests hand over packed, contiguous frames only: a packed
  batch in one copy, packed frames a copy each (a gap between frames), 2-D
  copies (rows or pitch that are not ip). Through dvc_quality_compare,
  tests/test_quality_gpu.py::test_host_pointers_pitch_and_stride runs the first
  and the last; the middle one is here.
* HandleStream: each single-stream handle created on the legacy default stream
  (hip_stream NULL with DVC_FLAG_JOIN_STREAM) and on a torch stream computes
  what it computes on a stream of its own.
* DevMem::release: the decoder's input staging grows on a live handle.
Bit-exact against each handle's reference, as everywhere."""
import ctypes

import numpy as np
import pytest

from tests import mjpeg_dec_cases as D
from tests import mjpeg_ref
from tests import quality_ref as R
from tests import test_mjpeg_decode_gpu as TD

pytestmark = pytest.mark.gpu

QUALITY = 75


@pytest.fixture(scope="module")
def N(gpu_lib):
    return gpu_lib._native


def _frames(W, H, n=3, seed=0):
    return np.random.default_rng(seed + W).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _laid_out(frames, pitch, stride, fill=0x5A):
    """`frames` (n, H, W, 3) in a byte buffer: frame t at t*stride, rows of `pitch` bytes."""
    n, H, W, _ = frames.shape
    buf = np.full(n * stride + 8, fill, np.uint8)
    for t in range(n):
        for y in range(H):
            o = t * stride + y * pitch
            buf[o:o + 3 * W] = frames[t, y].reshape(-1)
    return buf


def _jpeg_encode(N, buf, W, H, pitch, stride, n, stream=None, flags=0):
    """n host frames -> [entropy bytes] through one handle of max_batch 3 (one staging call)."""
    h, bound = ctypes.c_void_p(), ctypes.c_size_t()
    N.check(N.lib().dvc_jpeg_bound(W, H, N.FMT_BGR, ctypes.byref(bound)))
    N.check(N.lib().dvc_jpeg_create(W, H, N.FMT_BGR, QUALITY, 3, 0, stream, flags, ctypes.byref(h)))
    out, sizes = np.full((n, bound.value), 0xA5, np.uint8), np.zeros(n, np.uint32)
    try:
        N.check(N.lib().dvc_jpeg_encode(h, buf.ctypes.data, pitch, stride, n, out.ctypes.data, bound.value,
                                        sizes.ctypes.data))
        N.check(N.lib().dvc_jpeg_sync(h))
    finally:
        N.lib().dvc_jpeg_destroy(h)
    return [out[t, :int(sizes[t])].tobytes() for t in range(n)]


def _jpeg_want(frames):
    return [mjpeg_ref.encode(f, QUALITY)["stream"] for f in frames]


# (frames, bytes a row is padded by, bytes a frame is padded by)
LAYOUTS = [(1, 0, 0), (3, 0, 0), (3, 5, 8), (3, 0, 8)]


@pytest.mark.parametrize("n,pad,gap", LAYOUTS)
@pytest.mark.parametrize("W", [20, 18])          # rows of 60 = ip bytes: packed; of 54, ip 56: always 2-D copies
def test_jpeg_stages_host_frames_of_any_layout(N, W, n, pad, gap):
    H = 12
    frames = _frames(W, H)[:n]
    pitch = 3 * W + pad
    stride = pitch * H + gap
    got = _jpeg_encode(N, _laid_out(frames, pitch, stride), W, H, pitch, stride, n)
    assert got == _jpeg_want(frames)


def _quality_compare(N, W, H, ba, pitch, stride, bb, n, stream=None, flags=0):
    h = ctypes.c_void_p()
    N.check(N.lib().dvc_quality_create(W, H, 3, 0, stream, flags, ctypes.byref(h)))
    out = np.zeros(n, R.FRAME)
    try:
        N.check(N.lib().dvc_quality_compare(h, ba.ctypes.data, pitch, stride, bb.ctypes.data, 3 * W, 3 * W * H, n,
                                            out.ctypes.data))
        N.check(N.lib().dvc_quality_sync(h))
    finally:
        N.lib().dvc_quality_destroy(h)
    return out


def test_quality_stages_packed_frames_with_a_gap(N):
    """20x12: rows of 60 = ip bytes, frames 8 bytes apart: a copy a frame."""
    W, H = 20, 12
    a, b = _frames(W, H), _frames(W, H, seed=1)
    stride = 3 * W * H + 8
    got = _quality_compare(N, W, H, _laid_out(a, 3 * W, stride), 3 * W, stride, np.ascontiguousarray(b), 3)
    assert np.array_equal(got, R.records(a, b))


# ---- the stream a single-stream handle works on ----------------------------------------

def _ofc_run(N, frames, masks, stream=None, flags=0):
    n, H, W, _ = frames.shape
    h = ctypes.c_void_p()
    N.check(N.lib().dvc_ofc_create(W, H, 100.0, n, 0, stream, flags, ctypes.byref(h)))
    out = np.full_like(frames, 0xA5)
    try:
        N.check(N.lib().dvc_ofc_run(h, frames.ctypes.data, 3 * W, 3 * W * H, masks.ctypes.data, W, W * H, 1, n,
                                    out.ctypes.data, 3 * W * H))
        N.check(N.lib().dvc_ofc_sync(h))
    finally:
        N.lib().dvc_ofc_destroy(h)
    return out


def _jpegd_decode(N, jpgs, stream=None, flags=0):
    h = TD._handle(N, 70, 37, 2, stream, flags)
    try:
        frames, status, rc = TD._decode_host(N, h, jpgs)
        assert rc == 0 and not status.any()
        N.check(N.lib().dvc_jpegd_sync(h))
    finally:
        N.lib().dvc_jpegd_destroy(h)
    return frames


def test_small_handles_on_the_default_and_on_a_caller_stream(N, oracle_lib):
    """One call and a sync on each of dvc_quality, dvc_jpeg, dvc_jpegd and dvc_ofc, created
    on a stream of its own, on the legacy default stream (NULL, DVC_FLAG_JOIN_STREAM) and on
    a torch stream: the same outputs, the reference's. (dvc_ofc takes the flag as it took it
    before: its outputs are what is asserted.)"""
    import torch
    s = torch.cuda.Stream()
    streams = [(None, 0), (None, N.DVC_FLAG_JOIN_STREAM), (ctypes.c_void_p(s.cuda_stream), 0)]
    W, H = 20, 12
    a, b = _frames(W, H), _frames(W, H, seed=1)
    jpgs = [D.stream("ref", "noise70x37_q90", False, v) for v in (0, 1)]
    of_frames = _frames(24, 16, 2, seed=2)
    masks = np.zeros((2, 16, 24), np.uint8)
    masks[0, :8, 8:], masks[1, 4:, :12] = 255, 255
    for stream, flags in streams:
        q = _quality_compare(N, W, H, np.ascontiguousarray(a), 3 * W, 3 * W * H, np.ascontiguousarray(b), 3, stream,
                             flags)
        assert np.array_equal(q, R.records(a, b)), flags
        enc = _jpeg_encode(N, np.ascontiguousarray(a), W, H, 3 * W, 3 * W * H, 3, stream, flags)
        assert enc == _jpeg_want(a), flags
        dec = _jpegd_decode(N, jpgs, stream, flags)
        for t in (0, 1):
            assert np.array_equal(dec[t], D.expected("ref", "noise70x37_q90", False, t)), flags
        ofc = _ofc_run(N, of_frames, masks, stream, flags)
        for t in (0, 1):
            assert np.array_equal(ofc[t], oracle_lib.of_compress(of_frames[t], masks[t], 100.0)), flags
    torch.cuda.synchronize()


def test_jpegd_staging_grows_on_a_live_handle(N):
    """A small sample, one more than 256 bytes larger (the staging area is released and
    allocated again), the small one again."""
    small = ("ref", "noise70x37_q90", True)
    big = ("ref", "noise70x37_q90", False)
    ns, nb = (len(D.stream(*c)) - D.header_len(D.stream(*c)) for c in (small, big))
    assert nb > -(-ns // 256) * 256 + 256       # beyond the small sample's slot, rounded up to 256
    h = TD._handle(N, 70, 37, 2)
    try:
        for c in (small, big, small):
            frames, status, rc = TD._decode_host(N, h, [D.stream(*c)])
            assert rc == 0 and not status.any()
            assert np.array_equal(frames[0], D.expected(*c)), c
    finally:
        N.lib().dvc_jpegd_destroy(h)
