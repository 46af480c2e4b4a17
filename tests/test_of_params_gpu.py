"""GPU: the optical-flow kernels away from the reference's Farneback arguments.

dvc_of_create accepts a range of (pyr_scale, levels, winsize, iterations,
poly_n, poly_sigma); every other OF test runs the one point the reference
hard-codes (0.3, 2, 9, 2, 5, 1.1). Here each test id is one other point, chosen
for the code only it reaches: the poly_n 7 instantiations of the front and
pyramid kernels, the box radius 8 variant of the running-sum scan (its
compile-time path at winsize 17, its generic path below), the generic path of
the radius 4 variants, k_flow<0>, one and three iterations (buffer parity, the
counter sets), deeper pyramids and other blur radii, an even winsize (window
2 (winsize // 2) + 1, scale 1 / winsize^2).

(a) bit for bit against the oracle run with the same arguments: the stages of
    one frame pair (expansions of every level, the first iteration of every
    level that keeps it, the final flow), then a clip through
    test_of_gpu._run_pair (flow, every mask plane, mask, compressed, stats);
(b) against the float64 formulation of tests/farneback_ref.py, with the
    tolerance test_of_oracle.py derived for that set on the CPU;
(c) dvc_of_ktime_kernel names the form that must have run.
"""
import numpy as np
import pytest

from tests import farneback_ref as F
from tests.test_of_gpu import _first_diff, _run_pair

pytestmark = pytest.mark.gpu

FB_KEYS = ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma")
P7 = dict(poly_n=7, poly_sigma=1.5)
ALL = dict(pyr_scale=0.5, levels=3, winsize=13, iterations=3, poly_n=7, poly_sigma=1.5)


def _expected_kernel(kw):
    if kw.get("direct_sums"):
        return "k_flow"
    return "k_flow_scan2" if kw.get("winsize", 9) // 2 == 4 else "k_flow_scan"


def _keeps_first_iteration(level, iterations):
    """include/dvc.h, dvc_of_debug_read item 2."""
    return iterations in (2, 3) if level == 0 else iterations <= 2


def _bits_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        raise AssertionError(f"{what}: {_first_diff(got, want)}, max abs {np.abs(got - want).max()}")


def _stages(gpu_lib, oracle_lib, frames, bgr, kw):
    """One frame pair, stage by stage against the oracle's primitives chained
    as oc_farneback chains them (`frames`: what the GPU gets, `bgr`: the same
    frames as BGR)."""
    N = gpu_lib._native
    H, W = bgr.shape[1:3]
    p = F.Params(**{k: kw[k] for k in FB_KEYS if k in kw})
    sliding = not kw.get("direct_sums", False)
    gpu = gpu_lib.OFWorker(W, H, keep_planes=True, **kw)
    gpu.prime(frames[0])
    gpu.step(frames[1])
    g0, g1 = oracle_lib.bgr2gray(bgr[0]), oracle_lib.bgr2gray(bgr[1])
    assert np.array_equal(gpu.plane(N.OF_PLANE_GRAY), g1), "gray"
    L = int(oracle_lib._of_lib().oc_fb_levels(W, H, p.pyr_scale, p.levels))
    assert L == F.levels(W, H, p)
    flow = None
    for k in range(L, -1, -1):
        R = [oracle_lib.fb_level_poly(g, k, p.pyr_scale, p.poly_n, p.poly_sigma) for g in (g0, g1)]
        for what in (1, 0):            # debug_read 1: the previous frame's expansion
            _bits_equal(gpu.debug_read(what, k), R[1 - what], f"R level {k} ({'prev' if what else 'cur'})")
        h, w = R[0].shape[:2]
        flow = np.zeros((h, w, 2), np.float32) if flow is None else oracle_lib.fb_upsample(flow, w, h, p.pyr_scale)
        for it in range(p.iterations):
            flow = oracle_lib.fb_iteration(R[0], R[1], flow, winsize=p.winsize, sliding=sliding)
            if it:
                continue
            if _keeps_first_iteration(k, p.iterations):
                _bits_equal(gpu.debug_read(2, k), flow, f"first iteration of level {k}")
            else:           # overwritten by iteration 2, or never stored: refused, not stale data
                with pytest.raises(N.DvcError) as ei:
                    gpu.debug_read(2, k)
                assert ei.value.code == N.DVC_E_STATE
    want = oracle_lib.farneback(g0, g1, sliding=sliding, **p.kwargs())
    _bits_equal(flow, want, "the chained primitives are oc_farneback")
    _bits_equal(gpu.flow(), want, "final flow")
    assert gpu.ktime_kernel() == _expected_kernel(kw)
    gpu.close()


def _yuv(oracle_lib, frames, fmt):
    """(4:2:0 frames for the GPU, the BGR frames cvtColor makes of them for the oracle)."""
    from tests.test_video_io_gpu import _nv12
    H, W = frames.shape[1:3]
    i420 = np.stack([oracle_lib.bgr_to_i420(f) for f in frames])
    bgr = np.stack([oracle_lib.yuv420_to_bgr(f) for f in i420])
    return (i420 if fmt == "I420" else np.stack([_nv12(f, H, W) for f in i420])), bgr


# id, W, H, Farneback / worker keywords, _run_pair keywords
ORACLE_CASES = [
    ("poly7-124x108", 124, 108, P7, {}),                       # L = 1, coarse level 37 x 32
    ("poly7-333x185", 333, 185, P7, {}),                       # interior and edge tiles, odd width
    ("poly7-I420-170x100", 170, 100, dict(P7, in_format="I420"), {}),
    ("poly7-NV12-170x100", 170, 100, dict(P7, in_format="NV12"), {}),
    ("winsize5", 124, 108, dict(winsize=5), {}),               # m = 2 in the radius 4 scan: partial strip, partial block
    ("winsize5-direct", 124, 108, dict(winsize=5, direct_sums=True), {}),
    ("winsize8", 124, 108, dict(winsize=8), {}),               # k_flow_scan2 with scale 1 / 64
    ("winsize13", 124, 108, dict(winsize=13), {}),             # m = 6 in the radius 8 scan
    ("winsize17-124x108", 124, 108, dict(winsize=17), {}),     # m = 8: its compile-time path, the largest LDS request
    ("winsize17-136x76", 136, 76, dict(winsize=17), {}),       # height not a multiple of 8
    ("winsize17-direct", 124, 108, dict(winsize=17, direct_sums=True), {}),
    ("winsize1", 96, 64, dict(winsize=1), {}),                 # m = 0
    ("winsize1-direct", 96, 64, dict(winsize=1, direct_sums=True), {}),
    ("iterations1-124x108", 124, 108, dict(iterations=1), {}),
    ("iterations1-96x64", 96, 64, dict(iterations=1), {}),     # one level: no flow buffer is ever written
    ("iterations3", 124, 108, dict(iterations=3), dict(batch=2)),
    ("pyr0.5_levels3", 264, 260, dict(pyr_scale=0.5, levels=3), {}),   # L = 3, exact 2x resizes, 19-tap blur
    ("pyr0.8_levels5", 124, 108, dict(pyr_scale=0.8, levels=5), {}),   # L = 5: the deepest accepted
    ("levels0", 124, 108, dict(levels=0), {}),
    ("all-264x260", 264, 260, ALL, dict(batch=2, window_size=3)),
]


@pytest.mark.parametrize("W,H,kw,run_kw", [pytest.param(*c[1:], id=c[0]) for c in ORACLE_CASES])
def test_params_vs_oracle(gpu_lib, oracle_lib, W, H, kw, run_kw):
    from dvc_amd.synthetic import clip
    bgr = clip(W, H, 4, seed=W + H, n_objects=3)
    frames = bgr
    fmt = kw.get("in_format", "BGR")
    if fmt != "BGR":
        frames, bgr = _yuv(oracle_lib, bgr, fmt)
    _stages(gpu_lib, oracle_lib, frames, bgr, kw)
    st = _run_pair(gpu_lib, oracle_lib, frames, ref_frames=bgr, **run_kw, **kw)
    assert st["motion_px"] > 0, "the clip moves"


def test_params_all_device_pointers(gpu_lib, oracle_lib):
    """Every argument non-default at once, device frames, two batches of two in
    flight, a vote window that evicts."""
    import torch
    from dvc_amd.synthetic import clip
    W, H, n = 264, 260, 5
    frames = clip(W, H, n, seed=W + H + 1, n_objects=3)
    d_in = torch.from_numpy(frames).to("cuda:0")
    d_mask = torch.empty((n - 1, H, W), dtype=torch.uint8, device="cuda:0")
    d_cp = torch.empty((n - 1, H, W, 3), dtype=torch.uint8, device="cuda:0")
    w = gpu_lib.OFWorker(W, H, device_ptrs=True, max_batch=2, window_size=3, **ALL)
    w.prime(d_in[0])
    w.step_batch(d_in[1:], mask=d_mask, compressed=d_cp)
    w.sync()
    assert w.ktime_kernel() == "k_flow_scan"
    ref = oracle_lib.OracleOF(W, H, window_size=3, **ALL)
    ref.prime(frames[0])
    for t in range(1, n):
        rmask, rcp, _ = ref.step(frames[t])
        assert np.array_equal(d_mask[t - 1].cpu().numpy(), rmask), t
        assert np.array_equal(d_cp[t - 1].cpu().numpy(), rcp), t
    assert w.stats()["frames"] == n - 1
    w.close()
    ref.close()


# ------------------------------------------------------------- vs float64 ----
def _check_flow(got, want, tol, what):
    """test_of_reference_gpu._check_flow with the set's own tolerance."""
    err = float(np.abs(got - want).max())
    print(f"{what}: max abs error {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol, what
    mag = np.hypot(want[..., 0], want[..., 1])
    near = np.abs(mag - F.FLOW_THRESHOLD) <= tol
    differ = (np.hypot(got[..., 0], got[..., 1]) > F.FLOW_THRESHOLD) != (mag > F.FLOW_THRESHOLD)
    assert not (differ & ~near).any(), "raw mask differs away from the threshold"
    return near


@pytest.mark.parametrize("direct", [False, True], ids=["running", "direct"])
@pytest.mark.parametrize("name", sorted(F.PARAM_SETS))
def test_params_vs_float64(gpu_lib, name, direct):
    """Expansion of every level, the coarsest level's first iteration and the
    final flow of each textured pair of the set, both box-sum orders."""
    from tests.test_of_reference_gpu import _worker
    ps = F.PARAM_SETS[name]
    p = ps.p
    kw = dict(p.kwargs(), direct_sums=direct)
    for W, H, dx, dy in ps.cases:
        g0, g1, polys, want = F.flow_case(W, H, dx, dy, p)
        gpu = _worker(gpu_lib, g0, g1, **kw)
        assert gpu.ktime_kernel() == _expected_kernel(kw)
        L = F.levels(W, H, p)
        worst = 0.0
        for k in range(L + 1):
            for what, i in ((1, 0), (0, 1)):
                got = gpu.debug_read(what, k)
                assert got.shape == polys[i, k].shape, (k, got.shape)
                worst = max(worst, float(np.abs(got - polys[i, k]).max()))
        print(f"{name} polyexp {W}x{H}: max abs error {worst:.3e} (tolerance {ps.poly_tol:.3e})")
        assert worst <= ps.poly_tol
        if _keeps_first_iteration(L, p.iterations):
            h, w = polys[0, L].shape[:2]
            err = float(np.abs(gpu.debug_read(2, L) - F.iteration(polys[0, L], polys[1, L], np.zeros((h, w, 2)), p)).max())
            print(f"{name} iteration {w}x{h}: max abs error {err:.3e} (tolerance {ps.iter_tol:.3e})")
            assert err <= ps.iter_tol
        near = _check_flow(gpu.flow(), want, ps.flow_tol, f"{name} flow {W}x{H} ({dx}, {dy})")
        assert near.mean() < F.MASK_EXCUSED_SHARE
        gpu.close()


@pytest.mark.parametrize("direct", [False, True], ids=["running", "direct"])
def test_winsize1_vs_float64(gpu_lib, direct):
    """winsize 1: the running sums against float64 with OpenCV's start of the
    sums written in, the direct sums against the one-pixel box (the comment
    above farneback_ref.W1_CASE; figures from test_of_oracle.py)."""
    from tests.test_of_reference_gpu import _worker
    g0, g1, _, running, direct_flow = F.winsize1_case()
    gpu = _worker(gpu_lib, g0, g1, winsize=1, direct_sums=direct)
    assert gpu.ktime_kernel() == ("k_flow" if direct else "k_flow_scan")
    measured = F.W1_DIRECT_FLOW_MEASURED if direct else F.W1_RUNNING_FLOW_MEASURED
    _check_flow(gpu.flow(), direct_flow if direct else running, 8 * measured, f"winsize 1, direct={direct}")
    gpu.close()


# ------------------------------------------------- the edges of the range ----
@pytest.mark.parametrize("W,H,kw,code,text", [
    (124, 108, dict(poly_n=6), "DVC_E_UNSUPPORTED", "poly_n"),
    (124, 108, dict(winsize=0), "DVC_E_UNSUPPORTED", "winsize"),
    (124, 108, dict(winsize=18), "DVC_E_UNSUPPORTED", "winsize"),      # m = 9
    (124, 108, dict(winsize=19), "DVC_E_UNSUPPORTED", "winsize"),
    (124, 108, dict(iterations=0), "DVC_E_INVALID", "iterations"),
    (124, 108, dict(pyr_scale=1.0), "DVC_E_INVALID", "pyr_scale"),
    (124, 108, dict(pyr_scale=0.0), "DVC_E_INVALID", "pyr_scale"),
    (124, 108, dict(levels=-1), "DVC_E_INVALID", "levels"),
    (124, 108, dict(pyr_scale=0.9, levels=6), "DVC_E_UNSUPPORTED", "7 pyramid levels"),
    (2048, 2048, dict(pyr_scale=0.25, levels=3), "DVC_E_UNSUPPORTED", "159 taps"),   # sigma 31.5: cvRound(157.5) | 1; refused before any buffer is allocated
], ids=["poly_n6", "winsize0", "winsize18", "winsize19", "iterations0", "pyr_scale1", "pyr_scale0", "levels-1", "7levels", "159taps"])
def test_params_refused(gpu_lib, W, H, kw, code, text):
    N = gpu_lib._native
    with pytest.raises(N.DvcError) as ei:
        gpu_lib.OFWorker(W, H, **kw)
    assert ei.value.code == getattr(N, code), ei.value
    assert text in str(ei.value)


@pytest.mark.parametrize("kw", [dict(winsize=16), dict(winsize=17, poly_n=7), dict(pyr_scale=0.9, levels=5)],
                         ids=["winsize16", "winsize17-poly7", "6levels"])
def test_params_accepted_at_the_edge(gpu_lib, kw):
    gpu_lib.OFWorker(124, 108, **kw).close()


def test_debug_read_first_iteration_not_kept(gpu_lib):
    """dvc_of_debug_read item 2 where no buffer holds the first iteration's
    flow: one iteration on a one-level frame never stores a flow; it is refused
    (DVC_E_STATE), not answered with whatever the buffer held."""
    from dvc_amd.synthetic import clip
    N = gpu_lib._native
    frames = clip(96, 64, 2, seed=2)
    gpu = gpu_lib.OFWorker(96, 64, keep_planes=True, iterations=1)
    gpu.prime(frames[0])
    gpu.step(frames[1])
    with pytest.raises(N.DvcError) as ei:
        gpu.debug_read(2, 0)
    assert ei.value.code == N.DVC_E_STATE
    assert gpu.debug_read(0, 0).shape == (64, 96, 5)     # the other items still answer
    gpu.close()
