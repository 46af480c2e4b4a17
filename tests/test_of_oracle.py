"""CPU tests of the oracle's optical-flow path (the checker of the HIP kernels)
against tests/farneback_ref.py — an independent float64 formulation — and
known answers: the OF sibling of test_oracle.py. Nothing here shares code
with oracle/of_oracle.c, so a misreading of calcOpticalFlowFarneback, of the
structuring element, of the rectangles or of compress_with_motion that the
oracle and the kernels have in common fails here.

Each float comparison prints the error it measured before it asserts; the
tolerances are the named constants of farneback_ref.py (8 x the measured
float32-vs-float64 error, below a tenth of the smallest mutation effect).
"""
import numpy as np
import pytest

from tests import farneback_ref as F


def _report(name, err, tol):
    print(f"{name}: max abs error {err:.3e} (tolerance {tol:.3e})")


# ------------------------------------------------------ polynomial expansion --
def test_polyexp_recovers_quadratic():
    """Known answer for the reference itself: on an exact quadratic image the
    weighted fit returns that quadratic re-centred on each interior pixel."""
    c, bx, by, axx, ayy, axy = 3.0, -1.25, 0.75, 0.031, -0.017, 0.023
    H, W = 40, 52
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    I = c + bx * xs + by * ys + axx * xs * xs + ayy * ys * ys + axy * xs * ys
    R = F.polyexp(I)
    n = F.POLY_N
    want = np.stack([by + 2 * ayy * ys + axy * xs, bx + 2 * axx * xs + axy * ys,
                     np.full_like(xs, ayy), np.full_like(xs, axx), np.full_like(xs, axy)], axis=-1)
    assert np.abs(R - want)[n:-n, n:-n].max() < 1e-9


def test_polyexp_equals_pointwise_lstsq():
    """The vectorised fit == the definition (weighted lstsq over the 121
    samples) at corners, edges and interior pixels of a random image."""
    rng = np.random.default_rng(5)
    I = rng.uniform(0, 255, (23, 31))
    R = F.polyexp(I)
    for x, y in [(0, 0), (30, 0), (0, 22), (30, 22), (3, 11), (15, 2), (28, 20), (15, 11), (7, 16)]:
        assert np.abs(R[y, x] - F.polyexp_pixel(I, x, y)).max() < 1e-9, (x, y)


def test_levels_and_sizes(oracle_lib):
    for (W, H), L, sizes in [((96, 64), 0, [(96, 64)]), ((136, 72), 0, [(136, 72)]),
                             ((124, 108), 1, [(124, 108), (37, 32)]),
                             ((364, 356), 2, [(364, 356), (109, 107), (33, 32)]),
                             ((107, 106), 0, [(107, 106)]), ((107, 107), 1, [(107, 107), (32, 32)]),
                             ((1920, 1080), 2, [(1920, 1080), (576, 324), (173, 97)])]:
        assert F.levels(W, H) == L == oracle_lib._of_lib().oc_fb_levels(W, H, 0.3, 2)
        assert [F.level_size(W, H, k) for k in range(L + 1)] == sizes


@pytest.mark.parametrize("W,H", F.SHAPES_CPU)
def test_level_poly_vs_float64(oracle_lib, W, H):
    """Blur, resize and polynomial expansion of every pyramid level, whole
    image (border rows and columns included)."""
    worst = 0.0
    for dx, dy in F.FLOW_CASES[W, H]:
        g0, g1, polys, _ = F.flow_case(W, H, dx, dy)
        for k in range(F.levels(W, H) + 1):
            for i, g in enumerate((g0, g1)):
                got = oracle_lib.fb_level_poly(g, k)
                assert got.shape == polys[i, k].shape, (k, got.shape)
                worst = max(worst, float(np.abs(got - polys[i, k]).max()))
    _report(f"polyexp {W}x{H}", worst, F.POLY_TOL)
    assert worst <= F.POLY_TOL


# ------------------------------------------------------------- one iteration --
def _smooth_flow(w, h):
    """A few pixels of smooth flow that sends samples out of every side of the
    image. Coordinates that land within 1e-3 of an integer are moved off it:
    the in / out decision is a floor of a float32 sum in the oracle and of a
    float64 sum here, and the update is discontinuous across it."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.stack([3.37 * np.sin(xs / 17.0 + ys / 29.0 + 0.3), -4.21 * np.cos(xs / 23.0 - ys / 13.0)], axis=-1)
    for c, base in ((0, xs), (1, ys)):
        t = base + f[..., c]
        f[..., c] += np.where(np.abs(t - np.rint(t)) < 1e-3, 0.01, 0.0)
    return f.astype(np.float32)


@pytest.mark.parametrize("W,H,k", [(96, 64, 0), (124, 108, 1), (364, 356, 2), (364, 356, 1)])
def test_iteration_vs_float64(oracle_lib, W, H, k):
    """UpdateMatrices + the box solve, both box orders, from zero flow and from
    a smooth flow that leaves the image (the A0-alone branch); every frame is
    more than 10 px a side, so all four border bands and their corners count."""
    dx, dy = F.FLOW_CASES[W, H][0]
    polys = F.flow_case(W, H, dx, dy)[2]
    R0, R1 = polys[0, k].astype(np.float32), polys[1, k].astype(np.float32)   # the same inputs on both sides
    h, w = R0.shape[:2]
    assert h > 10 and w > 10
    moving = _smooth_flow(w, h)
    inside = F.displaced_inside(moving.astype(np.float64))
    assert 0.02 < 1 - inside.mean() < 0.5, "the flow must send some, not most, samples outside"
    assert not inside[0].all() and not inside[-1].all() and not inside[:, 0].all() and not inside[:, -1].all()
    worst = 0.0
    for flow in (np.zeros((h, w, 2), np.float32), moving):
        want = F.iteration(R0, R1, flow)
        for sliding in (True, False):
            got = oracle_lib.fb_iteration(R0, R1, flow, sliding=sliding)
            worst = max(worst, float(np.abs(got - want).max()))
    # and as the GPU test reads it: the oracle's own float32 expansions in,
    # against the float64 chain from the float64 expansions
    g0, g1 = F.flow_case(W, H, dx, dy)[:2]
    zero = np.zeros((h, w, 2), np.float32)
    got = oracle_lib.fb_iteration(oracle_lib.fb_level_poly(g0, k), oracle_lib.fb_level_poly(g1, k), zero)
    worst = max(worst, float(np.abs(got - F.iteration(polys[0, k], polys[1, k], zero)).max()))
    _report(f"iteration {w}x{h}", worst, F.ITER_TOL)
    assert worst <= F.ITER_TOL


# ----------------------------------------------------------------- full flow --
@pytest.mark.parametrize("W,H,dx,dy", [(W, H, dx, dy) for (W, H) in F.SHAPES_CPU for dx, dy in F.FLOW_CASES[W, H]])
def test_farneback_vs_float64(oracle_lib, W, H, dx, dy):
    """The flow through every pyramid level, both box orders, on an
    analytically translated texture. Measured: at most 1.11e-5 px between the
    oracle and float64; the float64 flow's median interior error against the
    true translation is 0.020 ... 0.035 px over the six cases (the bound 0.05
    is a sanity bound on the algorithm, not a rounding tolerance). The raw
    mask |flow| > 0.5 may differ only where the float64 magnitude lies within
    the flow tolerance of 0.5, and such pixels must stay under 0.1 %."""
    g0, g1, _, want = F.flow_case(W, H, dx, dy)
    err = want[16:-16, 16:-16] - np.array([dx, dy])
    median = float(np.median(np.hypot(err[..., 0], err[..., 1])))
    print(f"flow {W}x{H} ({dx}, {dy}): median interior error against the truth {median:.4f} px")
    mag = np.hypot(want[..., 0], want[..., 1])
    near = np.abs(mag - F.FLOW_THRESHOLD) <= F.FLOW_TOL
    gots = [oracle_lib.farneback(g0, g1, sliding=sliding) for sliding in (True, False)]
    worst = max(float(np.abs(got - want).max()) for got in gots)
    _report(f"flow {W}x{H} ({dx}, {dy})", worst, F.FLOW_TOL)
    assert median < F.FLOW_TRUTH_MEDIAN
    assert near.mean() < F.MASK_EXCUSED_SHARE
    assert worst <= F.FLOW_TOL
    for got in gots:
        differ = (np.hypot(got[..., 0], got[..., 1]) > F.FLOW_THRESHOLD) != (mag > F.FLOW_THRESHOLD)
        assert not (differ & ~near).any(), "raw mask differs away from the threshold"


def test_tolerances_discriminate():
    """8 x the measured error, and under a tenth of the smallest effect a
    single-constant mutation of the oracle has on the same comparison."""
    for measured, tol, mutation in ((F.POLY_MEASURED, F.POLY_TOL, F.POLY_MUTATION_MIN),
                                    (F.ITER_MEASURED, F.ITER_TOL, F.ITER_MUTATION_MIN),
                                    (F.FLOW_MEASURED, F.FLOW_TOL, F.FLOW_MUTATION_MIN)):
        assert measured > 0 and tol == 8 * measured
        assert tol < mutation / 10


# --------------------------------------------------------- ellipse, close/open --
ELLIPSES = {
    1: [[1]],
    2: [[0, 1],
        [1, 1]],
    3: [[0, 1, 0],
        [1, 1, 1],
        [0, 1, 0]],
    4: [[0, 0, 1, 0],
        [1, 1, 1, 1],
        [1, 1, 1, 1],
        [1, 1, 1, 1]],
    5: [[0, 0, 1, 0, 0],
        [1, 1, 1, 1, 1],
        [1, 1, 1, 1, 1],
        [1, 1, 1, 1, 1],
        [0, 0, 1, 0, 0]],
    7: [[0, 0, 0, 1, 0, 0, 0],
        [0, 1, 1, 1, 1, 1, 0],
        [1, 1, 1, 1, 1, 1, 1],
        [1, 1, 1, 1, 1, 1, 1],
        [1, 1, 1, 1, 1, 1, 1],
        [0, 1, 1, 1, 1, 1, 0],
        [0, 0, 0, 1, 0, 0, 0]],
    9: [[0, 0, 0, 0, 1, 0, 0, 0, 0],
        [0, 1, 1, 1, 1, 1, 1, 1, 0],
        [0, 1, 1, 1, 1, 1, 1, 1, 0],
        [1, 1, 1, 1, 1, 1, 1, 1, 1],
        [1, 1, 1, 1, 1, 1, 1, 1, 1],
        [1, 1, 1, 1, 1, 1, 1, 1, 1],
        [0, 1, 1, 1, 1, 1, 1, 1, 0],
        [0, 1, 1, 1, 1, 1, 1, 1, 0],
        [0, 0, 0, 0, 1, 0, 0, 0, 0]],
}


@pytest.mark.parametrize("k", sorted(ELLIPSES))
def test_ellipse_element_literal(oracle_lib, k):
    """getStructuringElement(MORPH_ELLIPSE, (k, k)) as cv2 prints it (the 5 x 5
    one is the matrix of OpenCV's morphological-operations tutorial).

    Odd elements are symmetric under both mirror flips. Under transposition
    only k = 1 and 3 are: OpenCV fills whole rows between c - dx and c + dx,
    which makes rows 1 ... k - 2 of the 5 x 5 element full while its columns 0
    and 4 are not — the tutorial's matrix is not its own transpose, and the
    test says so instead of asking for a symmetry cv2 does not have."""
    want = np.array(ELLIPSES[k], np.uint8)
    got = oracle_lib.ellipse_element(k)
    assert np.array_equal(got, want), got
    assert np.array_equal(F.ellipse(k), want)
    if k % 2:
        assert np.array_equal(got, got[::-1]) and np.array_equal(got, got[:, ::-1])
        assert np.array_equal(got, got.T) == (k <= 3)


def _masks():
    rng = np.random.default_rng(21)
    out = []
    for _ in range(60):
        H, W = int(rng.integers(3, 51)), int(rng.integers(3, 71))
        m = rng.random((H, W)) < rng.uniform(0.03, 0.9)
        if rng.random() < 0.4:       # blobs rather than salt and pepper
            m = np.repeat(np.repeat(m[::3, ::3], 3, axis=0), 3, axis=1)[:H, :W]
        out.append(m.astype(np.uint8) * 255)
    out.append(np.full((17, 29), 255, np.uint8))
    out.append(np.zeros((17, 29), np.uint8))
    frame = np.zeros((31, 43), np.uint8)      # components touching every border
    frame[0, 3:9] = frame[-1, 20:41] = frame[5:12, 0] = frame[14:30, -1] = 255
    frame[0, 0] = frame[-1, -1] = frame[0, -1] = frame[-1, 0] = 255
    frame[10:20, 10:25] = 255
    out.append(frame)
    ring = np.zeros((20, 20), np.uint8)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = 255, 255, 255, 255
    out.append(ring)
    return out


MASKS = _masks()


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 9])
def test_close_open_vs_shifted_minmax(oracle_lib, k):
    el = np.array(ELLIPSES[k], np.uint8)
    for n, m in enumerate(MASKS):
        got, want = oracle_lib.morph_close_open(m, k), F.close_open(m, k, el)
        assert np.array_equal(got, want), (k, n, m.shape)


def test_close_open_known_answers(oracle_lib):
    """k = 1 is the identity; full and empty masks stay as they are at every k
    (pixels outside the image take no part); the default k = 2 element
    [[0,1],[1,1]] removes an isolated pixel; a one-pixel hole is closed by the
    plus (k = 3)."""
    for m in MASKS[:10]:
        assert np.array_equal(oracle_lib.morph_close_open(m, 1), m)
    for k in (2, 3, 4, 5, 7, 9):
        for v in (0, 255):
            m = np.full((13, 11), v, np.uint8)
            assert np.array_equal(oracle_lib.morph_close_open(m, k), m), (k, v)
    m = np.zeros((9, 9), np.uint8)
    m[2, 2] = 255
    assert oracle_lib.morph_close_open(m, 2).max() == 0
    m = np.full((9, 9), 255, np.uint8)
    m[4, 4] = 0
    assert (oracle_lib.morph_close_open(m, 3) == 255).all()


def test_rect_mask_vs_label(oracle_lib):
    for n, m in enumerate(MASKS):
        got, cnt = oracle_lib.rect_mask(m)
        want, wcnt = F.rectangles(m)
        assert cnt == wcnt and np.array_equal(got, want), (n, m.shape)
    m = np.zeros((10, 12), np.uint8)      # known answer: grown one pixel right and down, clipped
    m[2:4, 3:6] = 255
    m[9, 11] = 255
    out, cnt = oracle_lib.rect_mask(m)
    want = np.zeros_like(m)
    want[2:5, 3:7] = 255
    want[9, 11] = 255
    assert cnt == 2 and np.array_equal(out, want)


# ---------------------------------------------------------------------- vote --
def test_vote_threshold_vs_reference_expression(oracle_lib):
    for L in range(1, 31):
        for alpha in (0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.7, 1.0):
            assert oracle_lib.vote_threshold(alpha, L) == F.vote_threshold(alpha, L), (alpha, L)
    # products whose float64 value is not the exact one, e.g. 0.1 * 3 * 255 = 76.50000000000001
    assert 0.1 * 3 * 255 != 76.5 and oracle_lib.vote_threshold(0.1, 3) == 1
    assert oracle_lib.vote_threshold(0.2, 30) == 6 and oracle_lib.vote_threshold(0.0, 5) == 0
    assert oracle_lib.vote_threshold(1.0, 30) == 30 and oracle_lib.vote_threshold(0.7, 10) == 7


@pytest.mark.parametrize("k", [2, 3])
def test_worker_stages_chain(oracle_lib, k):
    """The oracle's fused worker, stage by stage from its own upstream plane:
    the vote over its raw masks (window 3, so masks are dropped), close/open,
    rectangles — the chain the GPU test checks on the kernels."""
    rng = np.random.default_rng(k)
    frames = rng.integers(0, 256, (7, 72, 136, 3), dtype=np.uint8)
    ref = oracle_lib.OracleOF(136, 72, flow_threshold=1.0, window_size=3, alpha_fraction=0.4, morph_kernel=k)
    ref.prime(frames[0])
    raws = []
    for t in range(1, len(frames)):
        mask, _, flow = ref.step(frames[t])
        raw = ref.plane(0)
        assert np.array_equal(raw, (np.hypot(flow[..., 0], flow[..., 1]) > 1.0).astype(np.uint8) * 255)
        assert 0.02 < (raw > 0).mean() < 0.98
        raws.append(raw)
        assert np.array_equal(ref.plane(1), F.vote(raws, 3, 0.4)), t
        assert np.array_equal(ref.plane(2), F.close_open(ref.plane(1), k)), t
        assert np.array_equal(ref.plane(3), F.rectangles(ref.plane(2))[0]), t
        assert np.array_equal(mask, ref.plane(3))
    ref.close()


# --------------------------------------------------------------- compression --
@pytest.mark.parametrize("W,H", [(70, 52), (200, 120)])
def test_of_compress_vs_float64(oracle_lib, W, H):
    bgr = F.tie_free_bgr(W, H, seed=W)
    ycc = oracle_lib.bgr2ycrcb(bgr)
    assert np.array_equal(ycc, F.bgr2ycrcb(bgr)), "fixed-point YCrCb == rounded float64 formulas away from ties"
    mask = F.half_static_mask(W, H, seed=H)
    got = oracle_lib.of_compress(bgr, mask, 100.0)
    F.check_compress(got, bgr, mask, oracle_lib.ycrcb2bgr(ycc))
    if W % 8 and H % 8:        # the partial right and bottom blocks have a zero mask and are passed through
        assert (mask[H // 8 * 8:] == 0).all() and (mask[:, W // 8 * 8:] == 0).all()
