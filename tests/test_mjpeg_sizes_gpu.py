"""GPU: the Motion-JPEG kernels at the sizes where their loops take a later
trip and their index expressions leave the first frame, byte for byte:
dvc_jpeg_encode against tests/mjpeg_ref.py (257 restart segments, a full
64-block chunk at Q = 1 with its carry, 1920x1080 per sampled restart segment)
and dvc_jpegd_decode against Pillow (2, 3 and 16 lanes a wave in k_jpegd_huff
with an idle tail, batches of up to 149 different frames, markers across chunk
and window ends, damaged frames that share waves with good ones, 1920x1080),
and the two together at 1920x1080. tests/test_mjpeg_sizes.py asserts on the
CPU, from the references alone, that each fixture reaches its path."""
import ctypes
import io

import numpy as np
import pytest

from tests import mjpeg_cases as C
from tests import mjpeg_dec_cases as D
from tests import mjpeg_ref
from tests import quality_ref as Q
from tests.test_mjpeg_decode_gpu import _decode_host, _pack, _set_header
from tests.test_mjpeg_decode_gpu import _handle as _dec_handle
from tests.test_mjpeg_gpu import _bound, _encode_host
from tests.test_mjpeg_gpu import _handle as _enc_handle
from tests.test_mjpeg_sizes import LANE_BATCHES

pytestmark = pytest.mark.gpu

VARIANTS = (0, 1, 0)                                             # max_batch 2: a call of 3 splits


def _first_diff(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


# ---- encoder -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.SIZE_CASES))
def test_encode_size_cases_match_reference_bytes(gpu_lib, name):
    N = gpu_lib._native
    gray = C.SIZE_GRAY[name]
    frames = np.stack([C.frame(name, v)[..., 1] if gray else C.frame(name, v) for v in VARIANTS])
    got, sizes = _encode_host(N, frames, C.quality(name))         # (asserts nothing is written past a frame's bytes)
    for t, v in enumerate(VARIANTS):
        ref = C.reference(name, v, gray)["stream"]
        assert int(sizes[t]) == len(ref), f"{name} frame {t}: {sizes[t]} bytes, reference {len(ref)}"
        assert got[t] == ref, f"{name} frame {t}: first difference at byte {_first_diff(got[t], ref)}"


def test_encode_tall_colour_device_pointers_unaligned_pitch(gpu_lib):
    """tall16x4112 at a pitch of 3 * 16 + 5 bytes: k_jpeg_dct's byte loads, 257 segments."""
    import torch
    N = gpu_lib._native
    name = "tall16x4112"
    H, W = C.frame(name).shape[:2]
    pitch = 3 * W + 5
    host = np.full((3, H, pitch), 0x5A, np.uint8)
    for t, v in enumerate(VARIANTS):
        host[t, :, :3 * W] = C.frame(name, v).reshape(H, 3 * W)
    stride = _bound(N, W, H, N.FMT_BGR)
    h = _enc_handle(N, W, H, N.FMT_BGR, C.quality(name), 2, None, N.DVC_FLAG_DEVICE_PTRS)
    try:
        d_in = torch.from_numpy(host).cuda()
        d_out = torch.full((3, stride), 0xA5, dtype=torch.uint8, device="cuda")
        d_sizes = torch.zeros(3, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        N.check(N.lib().dvc_jpeg_encode(h, d_in.data_ptr(), pitch, H * pitch, 3, d_out.data_ptr(), stride,
                                        d_sizes.data_ptr()))
        N.check(N.lib().dvc_jpeg_sync(h))
        out, sizes = d_out.cpu().numpy(), d_sizes.cpu().numpy()
    finally:
        N.lib().dvc_jpeg_destroy(h)
    for t, v in enumerate(VARIANTS):
        ref = C.reference(name, v)["stream"]
        assert int(sizes[t]) == len(ref) and out[t, :len(ref)].tobytes() == ref, (t, _first_diff(out[t].tobytes(), ref))
        assert (out[t, len(ref):] == 0xA5).all()


@pytest.fixture(scope="module")
def hd_streams(gpu_lib):
    """The two hd1920x1080 frames through one dvc_jpeg_encode call at max_batch 2 -> ([entropy data], sizes)."""
    frames = np.stack([C.frame(C.HD_CASE, v) for v in (0, 1)])
    return _encode_host(gpu_lib._native, frames, C.quality(C.HD_CASE))


def test_encode_1080p_sampled_segments_match_reference_bytes(gpu_lib, hd_streams):
    """The production shape: 68 segments of 720 blocks (three trips of k_jpeg_bits' scan, twelve chunks
    of k_jpeg_pack). A whole-frame reference in Python is too slow; restart segments are independent
    (tests/test_mjpeg_sizes.py proves the identity), so sampled segments are compared."""
    N = gpu_lib._native
    got, sizes = hd_streams
    bound = _bound(N, 1920, 1080, N.FMT_BGR)
    assert got[0] != got[1]
    for t, sample in ((1, (0, 1, 33, 66, 67)), (0, (0, 67))):
        assert int(sizes[t]) == len(got[t]) < bound
        segs, marks = C.split_stream(got[t])
        assert marks == [0xD0 + i % 8 for i in range(67)] + [0xD9]   # exactly 67 RST markers, then EOI
        for i in sample:
            ref = C.segment_reference(C.HD_CASE, t, i)
            assert segs[i] == ref, f"frame {t} segment {i}: {len(segs[i])} bytes, reference {len(ref)}, first " \
                f"difference at byte {_first_diff(segs[i], ref)}"


# ---- decoder -------------------------------------------------------------------------
def _decode_variants(N, name, n, max_batch):
    jpgs = [D.stream("pil", name, None, v) for v in range(n)]
    W, H = D.SIZE_CASES[name][:2]
    h = _dec_handle(N, W, H, max_batch)
    try:
        frames, status, rc = _decode_host(N, h, jpgs)
    finally:
        N.lib().dvc_jpegd_destroy(h)
    assert rc == 0 and not status.any()
    return frames


def _assert_pillow(frames, name, skip=()):
    for v, f in enumerate(frames):
        if v in skip:
            continue
        want = D.pillow_frame(name, v)
        assert np.array_equal(f, want), f"{name} frame {v}: {np.count_nonzero(f != want)} bytes differ from Pillow, " \
            f"first at {tuple(int(a[0]) for a in np.nonzero(f != want))}"


@pytest.mark.parametrize("name,n", list(LANE_BATCHES))
def test_decode_lane_buckets(gpu_lib, name, n):
    """One call of n different frames on a handle of max_batch n: k_jpegd_huff runs 2, 3 or 16 lanes a
    wave and the last workgroup has idle lanes (tests/test_mjpeg_sizes.py: LANE_BATCHES)."""
    _assert_pillow(_decode_variants(gpu_lib._native, name, n, n), name)


def test_decode_split_call_equals_one_batch(gpu_lib):
    """max_batch 8, 19 frames: the call splits 8 + 8 + 3 at one lane a wave; the same frames as in one batch of 19."""
    N = gpu_lib._native
    name = "pil136x104_gray_b1"
    split, whole = _decode_variants(N, name, 19, 8), _decode_variants(N, name, 19, 19)
    assert np.array_equal(split, whole)
    _assert_pillow(split, name)


def _decode_device(N, hdr, datas, W, H, ch, pad, guard=8):
    """Entropy data through device pointers on a caller's stream: data_stride is the largest sample exactly
    (a frame's last byte is followed at once by the next frame's first), rows of ch * W + pad bytes, `guard`
    bytes between the frames' slots -> (slots (n, H * pitch + guard), status, the first dvc_jpegd_sync)."""
    import torch
    n = len(datas)
    stride = max(len(d) for d in datas)
    buf, sizes = _pack(datas, stride)
    pitch = ch * W + pad
    slot = H * pitch + guard
    s = torch.cuda.Stream()
    h = _dec_handle(N, W, H, n, ctypes.c_void_p(s.cuda_stream), N.DVC_FLAG_DEVICE_PTRS)
    try:
        assert _set_header(N, h, hdr)[1:] == (W, H, ch)
        with torch.cuda.stream(s):
            d_in = torch.from_numpy(buf).pin_memory().to("cuda", non_blocking=True)
            d_sizes = torch.from_numpy(sizes.view(np.int32)).pin_memory().to("cuda", non_blocking=True)
            d_out = torch.full((n, slot), 0xA5, dtype=torch.uint8, device="cuda")
            d_status = torch.full((n,), 77, dtype=torch.int32, device="cuda")
            N.check(N.lib().dvc_jpegd_decode(h, d_in.data_ptr(), stride, d_sizes.data_ptr(), n, d_out.data_ptr(), pitch,
                                             slot, d_status.data_ptr()))
            out = d_out.to("cpu", non_blocking=True)             # copied out on the caller's stream
            status = d_status.to("cpu", non_blocking=True)
        s.synchronize()
        rc = N.lib().dvc_jpegd_sync(h)
        assert N.lib().dvc_jpegd_sync(h) == N.DVC_OK             # reported once
    finally:
        N.lib().dvc_jpegd_destroy(h)
    return out.numpy(), status.numpy(), rc


def _rows(slot, W, H, ch, pad):
    """A slot -> (the frame, True when the row padding and the guard bytes are intact)."""
    pitch = ch * W + pad
    rows = slot[:H * pitch].reshape(H, pitch)
    intact = bool((rows[:, ch * W:] == 0xA5).all() and (slot[H * pitch:] == 0xA5).all())
    f = rows[:, :ch * W]
    return (f.reshape(H, W, 3) if ch == 3 else f), intact


def test_decode_device_pointers_packed_samples_padded_pitch(gpu_lib):
    N = gpu_lib._native
    name, n = "pil136x104_gray_b1_q95", 28
    jpgs = [D.stream("pil", name, None, v) for v in range(n)]
    hl = D.header_len(jpgs[0])
    out, status, rc = _decode_device(N, jpgs[0][:hl], [j[hl:] for j in jpgs], 136, 104, 1, 5)
    assert rc == N.DVC_OK and not status.any()
    for v in range(n):
        f, intact = _rows(out[v], 136, 104, 1, 5)
        assert intact, v
        assert np.array_equal(f, D.pillow_frame(name, v)), v


def test_damaged_frames_share_waves_with_good_ones(gpu_lib):
    """28 frames at 3 lanes a wave: frame 13 (truncated: the right marker count, so a lane of k_jpegd_huff
    returns early next to lanes of frames 12 and 14) and frame 20 (a marker missing: k_jpegd_index refuses
    it) are reported and left untouched; every other frame equals Pillow."""
    N = gpu_lib._native
    name, n, bad = "pil136x104_gray_b1_q95", 28, (13, 20)
    hdr, data = D.damaged("truncated", ("pil", name, None), n, 13, ((20, "no_rst"),))
    W, H = 136, 104
    # host pointers: the call returns the first damaged frame's status
    buf, sizes = _pack(data)
    h = _dec_handle(N, W, H, n)
    try:
        _set_header(N, h, hdr)
        out = np.full((n, H * W + 16), 0xA5, np.uint8)
        status = np.full(n, 77, np.int32)
        rc = N.lib().dvc_jpegd_decode(h, buf.ctypes.data, buf.shape[1], sizes.ctypes.data, n, out.ctypes.data, W,
                                      out.shape[1], status.ctypes.data)
        assert [t for t in range(n) if status[t] < 0] == list(bad) and not status[status >= 0].any()
        assert rc == status[13] and N.lib().dvc_jpegd_sync(h) == N.DVC_OK
    finally:
        N.lib().dvc_jpegd_destroy(h)
    assert (out[:, H * W:] == 0xA5).all() and all((out[t] == 0xA5).all() for t in bad)
    _assert_pillow(out[:, :H * W].reshape(n, H, W), name, skip=bad)
    # device pointers: asynchronous, dvc_jpegd_sync reports it, once
    out, status, rc = _decode_device(N, hdr, data, W, H, 1, 0, guard=16)
    assert [t for t in range(n) if status[t] < 0] == list(bad) and not status[status >= 0].any()
    assert rc == status[13]
    assert all((out[t] == 0xA5).all() for t in bad) and (out[:, H * W:] == 0xA5).all()
    _assert_pillow(out[:, :H * W].reshape(n, H, W), name, skip=bad)


def test_decode_1080p_equals_pillow(gpu_lib):
    """The production geometry: 68 segments, chunks of 12 KB (48 windows of k_jpegd_index), blockIdx.y up
    to 134 in k_jpegd_out, planes of 2 MB. Two frames through host pointers, one through device pointers."""
    N = gpu_lib._native
    name = "pil1920x1080_rows1"
    _assert_pillow(_decode_variants(N, name, 2, 2), name)
    jpg = D.stream("pil", name, None, 1)
    hl = D.header_len(jpg)
    out, status, rc = _decode_device(N, jpg[:hl], [jpg[hl:]], 1920, 1080, 3, 5)
    f, intact = _rows(out[0], 1920, 1080, 3, 5)
    assert rc == N.DVC_OK and status[0] == 0 and intact
    assert np.array_equal(f, D.pillow_frame(name, 1))


# ---- the two together ----------------------------------------------------------------
def _luma_psnr(a, b):
    return Q.psnr(int(((Q.luma(a) - Q.luma(b)) ** 2).sum()), a.shape[0] * a.shape[1])


def test_round_trip_1080p(gpu_lib, hd_streams):
    """The GPU encoder's two hd1920x1080 streams behind dvc_jpeg_header's bytes decode to the same frames on
    the GPU and in Pillow, at a luma PSNR no more than 1 dB below that of Pillow's own quality-75 encode of
    the frame. Measured on an MI355X: 28.375 dB against Pillow's 28.381 dB for frame 0, 28.408 dB against
    28.414 dB for frame 1 (a third of each frame is noise)."""
    from PIL import Image
    N = gpu_lib._native
    hdr = mjpeg_ref.header_bytes(1920, 1080, N.FMT_BGR, C.quality(C.HD_CASE))
    jpgs = [hdr + s for s in hd_streams[0]]
    h = _dec_handle(N, 1920, 1080, 2)
    try:
        frames, status, rc = _decode_host(N, h, jpgs)
    finally:
        N.lib().dvc_jpegd_destroy(h)
    assert rc == 0 and not status.any()
    for t in (0, 1):
        assert np.array_equal(frames[t], D.pillow(jpgs[t])), f"frame {t}: the GPU decoder differs from Pillow"
        src = C.frame(C.HD_CASE, t)
        buf = io.BytesIO()
        Image.fromarray(src[..., ::-1].copy()).save(buf, "JPEG", quality=75, subsampling=2)
        ours, pil = _luma_psnr(src, frames[t]), _luma_psnr(src, D.pillow(buf.getvalue()))
        print(f"hd1920x1080 frame {t}: luma PSNR {ours:.3f} dB, Pillow's own encode {pil:.3f} dB")
        assert ours > pil - 1.0, (t, ours, pil)
