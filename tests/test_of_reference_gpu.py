"""GPU: the HIP optical-flow kernels against tests/farneback_ref.py — an
independent float64 formulation — directly, not through the CPU oracle.

test_of_gpu.py holds the kernels bit for bit to oracle/of_oracle.c; here the
same kernels meet a formulation that shares no code with either, with the
tolerances tests/test_of_oracle.py derived on the CPU (farneback_ref.*_TOL).
Gray frames go in as BGR = (v, v, v), which the gray kernel maps to v exactly.
The vote, the close/open, the rectangles and the compressor are exact and are
checked stage by stage from the GPU's own upstream plane.
"""
import numpy as np
import pytest

from tests import farneback_ref as F

pytestmark = pytest.mark.gpu


def _worker(gpu_lib, g0, g1, **kw):
    H, W = g0.shape
    gpu = gpu_lib.OFWorker(W, H, keep_planes=True, **kw)
    gpu.prime(F.gray_bgr(g0))
    gpu.step(F.gray_bgr(g1))
    assert np.array_equal(gpu.plane(gpu_lib._native.OF_PLANE_GRAY), g1), "gray of (v, v, v) is v"
    return gpu


def _check_flow(got, W, H, dx, dy, what):
    want = F.flow_case(W, H, dx, dy)[3]
    err = float(np.abs(got - want).max())
    print(f"{what} {W}x{H} ({dx}, {dy}): max abs error {err:.3e} (tolerance {F.FLOW_TOL:.3e})")
    assert err <= F.FLOW_TOL, what
    mag = np.hypot(want[..., 0], want[..., 1])
    near = np.abs(mag - F.FLOW_THRESHOLD) <= F.FLOW_TOL
    assert near.mean() < F.MASK_EXCUSED_SHARE
    differ = (np.hypot(got[..., 0], got[..., 1]) > F.FLOW_THRESHOLD) != (mag > F.FLOW_THRESHOLD)
    assert not (differ & ~near).any(), "raw mask differs away from the threshold"


@pytest.mark.parametrize("W,H", F.SHAPES_GPU)
def test_stages_vs_float64(gpu_lib, W, H):
    """The polynomial expansion of both frames at every pyramid level, the
    coarsest level's first iteration from zero flow, and the final flow."""
    dx, dy = F.FLOW_CASES[W, H][0]
    g0, g1, polys, _ = F.flow_case(W, H, dx, dy)
    gpu = _worker(gpu_lib, g0, g1)
    L = F.levels(W, H)
    worst = 0.0
    for k in range(L + 1):
        for what, i in ((1, 0), (0, 1)):            # debug_read 1: the previous frame's expansion
            got = gpu.debug_read(what, k)
            assert got.shape == polys[i, k].shape, (k, got.shape)
            worst = max(worst, float(np.abs(got - polys[i, k]).max()))
    print(f"polyexp {W}x{H}: max abs error {worst:.3e} (tolerance {F.POLY_TOL:.3e})")
    assert worst <= F.POLY_TOL
    h, w = polys[0, L].shape[:2]
    want = F.iteration(polys[0, L], polys[1, L], np.zeros((h, w, 2)))
    got = gpu.debug_read(2, L)
    err = float(np.abs(got - want).max())
    print(f"iteration {w}x{h}: max abs error {err:.3e} (tolerance {F.ITER_TOL:.3e})")
    assert err <= F.ITER_TOL
    _check_flow(gpu.flow(), W, H, dx, dy, "flow")
    gpu.close()


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("W,H,dx,dy", [(W, H, dx, dy) for (W, H) in F.SHAPES_GPU for dx, dy in F.FLOW_CASES[W, H]])
def test_flow_vs_float64(gpu_lib, W, H, dx, dy, direct):
    """Both box-sum orders (running sums, direct sums) on every translation."""
    g0, g1 = F.flow_case(W, H, dx, dy)[:2]
    gpu = _worker(gpu_lib, g0, g1, direct_sums=direct)
    assert gpu.ktime_kernel() == ("k_flow" if direct else "k_flow_scan2")
    _check_flow(gpu.flow(), W, H, dx, dy, "direct sums" if direct else "running sums")
    gpu.close()


@pytest.mark.parametrize("W,H,env,kernel", [
    (136, 72, {"DVC_OF_SCAN2": "0"}, "k_flow_scan"),         # the barrier-phased scan, partial last strip
    (124, 108, {"DVC_OF_UP_GATHER": "1"}, "k_flow_scan2"),   # the gather upsample between two levels
])
def test_other_kernel_forms_vs_float64(gpu_lib, W, H, env, kernel, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dx, dy = F.FLOW_CASES[W, H][-1]
    g0, g1 = F.flow_case(W, H, dx, dy)[:2]
    gpu = _worker(gpu_lib, g0, g1)
    assert gpu.ktime_kernel() == kernel
    _check_flow(gpu.flow(), W, H, dx, dy, "+".join(env))
    gpu.close()


@pytest.mark.parametrize("k", [2, 3, 4, 7])
def test_vote_morph_rect_chain(gpu_lib, k):
    """Six noise frames, window 3 (masks get dropped): after every step each
    stage is checked from the GPU's own upstream plane — the raw mask from its
    flow, the vote from its raw masks, the close/open from its vote plane, the
    rectangles from its close/open plane — and the component count."""
    N = gpu_lib._native
    rng = np.random.default_rng(k)
    frames = rng.integers(0, 256, (6, 72, 136, 3), dtype=np.uint8)
    gpu = gpu_lib.OFWorker(136, 72, keep_planes=True, flow_threshold=1.0, window_size=3, alpha_fraction=0.4,
                           morph_kernel=k)
    gpu.prime(frames[0])
    raws, comps = [], 0
    for t in range(1, len(frames)):
        mask, _ = gpu.step(frames[t])
        flow = gpu.flow().astype(np.float64)
        raw = gpu.plane(N.OF_PLANE_RAW)
        mag = np.hypot(flow[..., 0], flow[..., 1])
        close = np.abs(mag - 1.0) < 1e-5            # float32 sqrt against float64 hypot
        assert close.mean() < 1e-3
        assert np.array_equal(raw[~close], ((mag > 1.0).astype(np.uint8) * 255)[~close]), t
        assert set(np.unique(raw).tolist()) <= {0, 255} and 0.02 < (raw > 0).mean() < 0.98
        raws.append(raw)
        smooth, morph, rect = (gpu.plane(p) for p in (N.OF_PLANE_SMOOTH, N.OF_PLANE_MORPH, N.OF_PLANE_RECT))
        assert np.array_equal(smooth, F.vote(raws, 3, 0.4)), f"vote, step {t}"
        assert np.array_equal(morph, F.close_open(smooth, k)), f"close/open, step {t}"
        want_rect, n = F.rectangles(morph)
        assert np.array_equal(rect, want_rect), f"rectangles, step {t}"
        assert np.array_equal(mask, rect)
        comps += n
        assert gpu.stats()["components"] == comps, t
    gpu.close()


@pytest.mark.parametrize("W,H", [(70, 52), (200, 120)])
def test_of_compress_vs_float64(gpu_lib, W, H):
    """The 8 x 8 three-channel compressor against the float64 one: static
    blocks gray and within one level (blocks with a coefficient on a rounding
    tie excused, at most 2 %), everything else — partial edge blocks included —
    the plain YCrCb round trip."""
    bgr = F.tie_free_bgr(W, H, seed=W)
    mask = F.half_static_mask(W, H, seed=H)
    got = gpu_lib._native.of_compress(bgr, mask, 100.0)
    F.check_compress(got, bgr, mask)
