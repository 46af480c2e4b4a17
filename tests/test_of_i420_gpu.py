"""GPU parity: DVC_FLAG_OUT_I420 on the optical-flow path. The compressed
frames of the OF worker (dvc_of_step / _step_batch) and of the compressor
(dvc_ofc_run) as the encoder's 4:2:0 input: byte for byte cvtColor
BGR2YUV_I420 (the oracle's bgr_to_i420) of the oracle's BGR frame.

Sizes: k_of_out covers 64 px x 32 rows a workgroup, 8 blocks to a wave.
  64x32     one workgroup, every block full, every luma and chroma store a dword
  70x38     W % 4 = 2 (byte luma on odd rows), chroma rows of 35 bytes (byte
            chroma), 6 px in the last block column, 6 rows in the last block
            row, a second workgroup in x and in y
  136x40    W % 8 = 0 with 17 blocks a row (the third wave column holds one
            group), 5 block rows (a partial second workgroup in y), chroma
            dwords at a pitch of 68
  1920x1080 (compressor only, 2 frames) 135 block rows, the workload's alignment
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(64, 32), (70, 38), (136, 40)]
_cache = {}


def _clip(W, H):
    """6 synthetic frames with two frames of uniform noise spliced in."""
    from dvc_amd.synthetic import SyntheticClip
    f = SyntheticClip(W, H, seed=W + H).frames(6)
    rng = np.random.default_rng(W * H)
    noise = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([f[:3], noise[:1], f[3:5], noise[1:], f[5:]]))


def _worker_case(oracle, W, H, yuv=False):
    """(frames, BGR frames the oracle saw, oracle masks, oracle compressed frames
    as I420), computed once per size; ``yuv``: the frames as 4:2:0 (I420) frames,
    the oracle fed their cvtColor YUV2BGR."""
    key = ("of", W, H, yuv)
    if key not in _cache:
        frames = _clip(W, H)
        src = frames
        if yuv:
            src = np.stack([oracle.bgr_to_i420(f) for f in frames])
            frames = np.stack([oracle.yuv420_to_bgr(f) for f in src])
        ref = oracle.OracleOF(W, H)
        ref.prime(frames[0])
        outs = [ref.step(f)[:2] for f in frames[1:]]
        ref.close()
        masks = np.stack([m for m, _ in outs])
        want = np.stack([oracle.bgr_to_i420(c) for _, c in outs])
        for a in (src, masks, want):
            a.setflags(write=False)
        _cache[key] = (src, masks, want)
    return _cache[key]


def _rect_masks(W, H, n, seed):
    """Gray masks: frame 0 empty and frame 1 full (where n allows both beside two
    drawn frames), the others random rectangles of nonzero values."""
    rng = np.random.default_rng(seed)
    m = np.zeros((n, H, W), np.uint8)
    drawn = list(range(n))
    if n >= 4:
        m[1] = 255
        drawn = drawn[2:]
    for t in drawn:
        for _ in range(2):
            w, h = int(rng.integers(4, W // 2)), int(rng.integers(4, H // 2))
            x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
            m[t, y:y + h, x:x + w] = rng.integers(1, 256, (h, w), dtype=np.uint8)
    return m, drawn


def _comp_case(oracle, W, H):
    """(frames, gray masks, their 3-channel form, indices of the drawn frames,
    oracle outputs as I420), once per size. The 3-channel masks gray back to the
    gray masks exactly ((v, v, v) -> v; the sprinkled (1, 0, 0) -> 0, of:147-149),
    so one oracle run serves both."""
    key = ("ofc", W, H)
    if key not in _cache:
        n = 2 if W * H > 1 << 20 else 5
        rng = np.random.default_rng(W + 3 * H)
        frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        frames[0, : H // 2] = _clip(W, H)[1, : H // 2]      # smooth content beside the noise
        gm, drawn = _rect_masks(W, H, n, W * 7 + H)
        m3 = np.repeat(gm[..., None], 3, axis=-1)
        m3[(gm == 0) & (rng.random((n, H, W)) < 0.02)] = (1, 0, 0)
        want = np.stack([oracle.bgr_to_i420(oracle.of_compress(frames[t], gm[t], 100.0)) for t in range(n)])
        for a in (frames, gm, m3, want):
            a.setflags(write=False)
        _cache[key] = (frames, gm, m3, drawn, want)
    return _cache[key]


def _diff(got, want):
    d = np.argwhere(got != want)
    return f"{len(d)} bytes differ, first at {d[:4].tolist()}"


# ------------------------------------------------------------------ worker ----
@pytest.mark.parametrize("batched", [False, True], ids=["step", "step_batch"])
@pytest.mark.parametrize("W,H", SIZES)
def test_worker_i420_equals_oracle(gpu_lib, oracle_lib, W, H, batched):
    """One frame per step, and one step_batch call on a handle of max_batch 4
    (7 frames: the call splits): compressed[t] == bgr_to_i420 of the oracle's
    compressed frame; the masks equal the oracle's and a BGR handle's."""
    frames, rmasks, want = _worker_case(oracle_lib, W, H)
    got = {}
    for fmt in ("I420", "BGR"):
        g = gpu_lib.OFWorker(W, H, max_batch=4 if batched else 1, out_format=fmt)
        g.prime(frames[0])
        if batched:
            got[fmt] = g.step_batch(frames[1:])
        else:
            outs = [g.step(f) for f in frames[1:]]
            got[fmt] = (np.stack([m for m, _ in outs]), np.stack([c for _, c in outs]))
        g.close()
    masks, cps = got["I420"]
    assert cps.shape == (len(frames) - 1, H * 3 // 2, W)
    for t in range(len(frames) - 1):
        assert np.array_equal(masks[t], rmasks[t]), f"mask differs at frame {t + 1}"
        assert np.array_equal(masks[t], got["BGR"][0][t]), f"mask != the BGR handle's at frame {t + 1}"
        assert np.array_equal(cps[t], want[t]), f"compressed (I420) at frame {t + 1}: {_diff(cps[t], want[t])}"
        assert np.array_equal(oracle_lib.bgr_to_i420(got["BGR"][1][t]), want[t]), f"BGR handle at frame {t + 1}"


def test_worker_i420_from_nv12_surfaces(gpu_lib, oracle_lib):
    """4:2:0 input surfaces read in place (k_of_out converts as it loads) with
    I420 outputs: NV12 decoder surfaces of padded pitch and chroma offset."""
    import torch
    from tests.test_video_io_gpu import _nv12, _surface
    W, H, pitch, crows = 136, 40, 192, 48
    i420, rmasks, want = _worker_case(oracle_lib, W, H, yuv=True)
    n = len(i420)
    surf = np.stack([_surface(_nv12(f, H, W), H, W, "NV12", pitch, crows) for f in i420])
    d = torch.from_numpy(surf).cuda()
    mk = torch.empty((n - 1, H, W), dtype=torch.uint8, device="cuda")
    cp = torch.empty((n - 1, H * 3 // 2, W), dtype=torch.uint8, device="cuda")
    N = gpu_lib._native
    p = gpu_lib.of.derive_of_params(W, H, flags=N.DVC_FLAG_DEVICE_PTRS | N.DVC_FLAG_OUT_I420, in_format="NV12",
                                    chroma_rows=crows)
    p.max_batch = 4
    L = N.lib()
    h = ctypes.c_void_p()
    N.check(L.dvc_of_create(ctypes.byref(p), 0, None, ctypes.byref(h)))
    try:
        N.check(L.dvc_of_prime(h, d[0].data_ptr(), pitch))
        N.check(L.dvc_of_step_batch(h, d[1].data_ptr(), pitch, surf[0].nbytes, n - 1, mk.data_ptr(), H * W,
                                    cp.data_ptr(), H * W * 3 // 2))
        N.check(L.dvc_of_sync(h))
    finally:
        L.dvc_of_destroy(h)
    mk, cp = mk.cpu().numpy(), cp.cpu().numpy()
    for t in range(n - 1):
        assert np.array_equal(mk[t], rmasks[t]), f"mask differs at frame {t + 1}"
        assert np.array_equal(cp[t], want[t]), f"compressed (I420) at frame {t + 1}: {_diff(cp[t], want[t])}"


# -------------------------------------------------------------- compressor ----
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("W,H", SIZES + [(1920, 1080)])
def test_compressor_i420_equals_oracle(gpu_lib, oracle_lib, W, H, ch):
    """dvc_ofc_run with the flag, 1- and 3-channel masks: == bgr_to_i420 of the
    oracle's of_compress, and == dvc_bgr_to_i420 of a flag-less handle's output.
    Every drawn-rectangle frame has static and non-static full blocks (checked
    from the mask), so neither branch of the kernel can carry the test alone.
    (1080p runs 2 frames, both drawn: the empty and the full mask are at the
    three small sizes.)"""
    frames, gm, m3, drawn, want = _comp_case(oracle_lib, W, H)
    n = len(frames)
    assert len(drawn) >= 2 and (n < 4 or (not gm[0].any() and gm[1].all()))
    for t in drawn:
        blocks = gm[t, : H // 8 * 8, : W // 8 * 8].reshape(H // 8, 8, W // 8, 8).max(axis=(1, 3))
        assert (blocks == 0).any() and (blocks != 0).any(), f"mask {t}: static and non-static full blocks"
    masks = gm if ch == 1 else m3
    N = gpu_lib._native
    with N.OFCompressor(W, H, max_batch=3, out_format="I420") as c:
        got = c.run(frames, masks)
    with N.OFCompressor(W, H, max_batch=3) as c:
        bgr = c.run(frames, masks)
    assert got.shape == (n, H * 3 // 2, W) and bgr.shape == (n, H, W, 3)
    conv = N.bgr_to_i420(bgr)
    for t in range(n):
        assert np.array_equal(got[t], want[t]), f"frame {t}: {_diff(got[t], want[t])}"
        assert np.array_equal(got[t], conv[t]), f"frame {t} != dvc_bgr_to_i420 of the BGR output"


# --------------------------------------------------------- device pointers ----
def test_device_pointers_padded_stride_caller_stream(gpu_lib, oracle_lib):
    """Both handles at 70x38 with device pointers on a caller's stream: 3 frames
    at an out_stride of W*H*3/2 + 8 (frames 1 and 2 start at addresses that are
    no multiple of 4) into 0xA5-filled buffers, copied out on that stream with
    no other sync; every byte outside the frames is still 0xA5."""
    import torch
    W, H, n = 70, 38, 3
    FB = W * H * 3 // 2
    stride = FB + 8
    assert stride % 4
    N = gpu_lib._native
    L = N.lib()
    frames, rmasks, want = _worker_case(oracle_lib, W, H)
    cframes, gm, _, _, cwant = _comp_case(oracle_lib, W, H)
    s = torch.cuda.Stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    p = gpu_lib.of.derive_of_params(W, H, flags=N.DVC_FLAG_DEVICE_PTRS | N.DVC_FLAG_OUT_I420)
    p.max_batch = 2
    h, c = ctypes.c_void_p(), ctypes.c_void_p()
    N.check(L.dvc_of_create(ctypes.byref(p), 0, sp, ctypes.byref(h)))
    try:
        N.check(L.dvc_ofc_create(W, H, 100.0, 2, 0, sp, N.DVC_FLAG_DEVICE_PTRS | N.DVC_FLAG_OUT_I420, ctypes.byref(c)))
        with torch.cuda.stream(s):
            d = torch.from_numpy(frames[:n + 1].copy()).pin_memory().to("cuda", non_blocking=True)
            d_mk = torch.full((n, W * H + 8), 0xA5, dtype=torch.uint8, device="cuda")
            d_cp = torch.full((n, stride), 0xA5, dtype=torch.uint8, device="cuda")
            N.check(L.dvc_of_prime(h, d[0].data_ptr(), 3 * W))
            N.check(L.dvc_of_step_batch(h, d[1].data_ptr(), 3 * W, 3 * W * H, n, d_mk.data_ptr(), W * H + 8,
                                        d_cp.data_ptr(), stride))
            dc = torch.from_numpy(cframes[:n].copy()).pin_memory().to("cuda", non_blocking=True)
            dm = torch.from_numpy(gm[:n].copy()).pin_memory().to("cuda", non_blocking=True)
            d_out = torch.full((n, stride), 0xA5, dtype=torch.uint8, device="cuda")
            N.check(L.dvc_ofc_run(c, dc.data_ptr(), 3 * W, 3 * W * H, dm.data_ptr(), W, W * H, 1, n, d_out.data_ptr(),
                                  stride))
            mk = d_mk.to("cpu", non_blocking=True)             # copied out on the caller's stream, no other sync
            cp = d_cp.to("cpu", non_blocking=True)
            out = d_out.to("cpu", non_blocking=True)
        s.synchronize()
        assert L.dvc_of_sync(h) == N.DVC_OK and L.dvc_ofc_sync(c) == N.DVC_OK
    finally:
        L.dvc_of_destroy(h)
        if c:
            L.dvc_ofc_destroy(c)
    mk, cp, out = mk.numpy(), cp.numpy(), out.numpy()
    for t in range(n):
        assert np.array_equal(mk[t, :W * H].reshape(H, W), rmasks[t]), f"mask differs at frame {t + 1}"
        assert np.array_equal(cp[t, :FB].reshape(H * 3 // 2, W), want[t]), f"worker frame {t + 1}"
        assert np.array_equal(out[t, :FB].reshape(H * 3 // 2, W), cwant[t]), f"compressor frame {t}"
    assert (mk[:, W * H:] == 0xA5).all() and (cp[:, FB:] == 0xA5).all() and (out[:, FB:] == 0xA5).all()


# ---------------------------------------------------------------- refusals ----
@pytest.mark.parametrize("W,H", [(71, 38), (70, 37)])
def test_odd_sides_refused_at_create(gpu_lib, W, H):
    N = gpu_lib._native
    L = N.lib()
    for flags, code in ((N.DVC_FLAG_OUT_I420, N.DVC_E_UNSUPPORTED), (0, N.DVC_OK)):
        p = gpu_lib.of.derive_of_params(W, H, flags=flags)
        h = ctypes.c_void_p()
        rc = L.dvc_of_create(ctypes.byref(p), 0, None, ctypes.byref(h))
        assert rc == code, ("dvc_of_create", flags, rc)
        assert rc == N.DVC_OK or (L.dvc_last_error() or b"").strip(), "dvc_last_error names the reason"
        if h:
            L.dvc_of_destroy(h)
        c = ctypes.c_void_p()
        rc = L.dvc_ofc_create(W, H, 100.0, 2, 0, None, flags, ctypes.byref(c))
        assert rc == code, ("dvc_ofc_create", flags, rc)
        assert rc == N.DVC_OK or (L.dvc_last_error() or b"").strip(), "dvc_last_error names the reason"
        if c:
            L.dvc_ofc_destroy(c)


# ------------------------------------------------------------------ driver ----
def test_driver_y4m_sinks_take_i420(gpu_lib, oracle_lib, tmp_path, monkeypatch):
    """process_single_video_of with Y4M sinks: compressed.y4m holds the
    compressor's I420 frames and overlay.y4m one batched conversion per chunk —
    never a conversion of one frame at a time."""
    from dvc_amd import _native, video_io
    from dvc_amd.motion_compression_opt import process_single_video_of
    from dvc_amd.synthetic import SyntheticClip
    W, H, n = 160, 96, 12
    calls = []
    real = _native.bgr_to_i420

    def spy(frames, device=0):
        calls.append(np.ndim(frames))
        return real(frames, device)

    monkeypatch.setattr(_native, "bgr_to_i420", spy)
    monkeypatch.setenv("DVC_VIDEO_SINK", "y4m")
    process_single_video_of(f"synthetic://{W}x{H}?frames={n}", str(tmp_path))
    assert calls and all(d == 4 for d in calls), f"bgr_to_i420 called with frames of ndim {calls}"
    monkeypatch.setattr(_native, "bgr_to_i420", real)
    out = tmp_path / f"{W}x{H}"

    def frames_of(name, read):
        cap = video_io.Y4mReader(str(out / name))
        assert cap.isOpened() and cap.get(video_io.CAP_PROP_FRAME_COUNT) == n - 1, name
        got = [getattr(cap, read)()[1] for _ in range(n - 1)]
        cap.release()
        return got

    src = SyntheticClip(W, H, seed=0).frames(n)
    overlay = frames_of("overlay.y4m", "read")               # what the second pass read
    masks = frames_of("mask.y4m", "read")
    comp = frames_of("compressed.y4m", "read_yuv")
    for t in range(n - 1):
        want = oracle_lib.bgr_to_i420(oracle_lib.of_compress(overlay[t], masks[t], 100.0))
        assert np.array_equal(comp[t], want), f"compressed.y4m frame {t}: {_diff(comp[t], want)}"
    for t, f in enumerate(frames_of("overlay.y4m", "read_yuv")):
        assert np.array_equal(f, oracle_lib.bgr_to_i420(src[t + 1])), f"overlay.y4m frame {t}"
