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


def test_polyexp_poly_n7_equals_pointwise_lstsq():
    """The same at poly_n 7, sigma 1.5: the 15 x 15 window, 225 samples."""
    p = F.Params(poly_n=7, poly_sigma=1.5)
    rng = np.random.default_rng(6)
    I = rng.uniform(0, 255, (23, 31))
    R = F.polyexp(I, p)
    for x, y in [(0, 0), (30, 0), (0, 22), (30, 22), (5, 11), (15, 3), (26, 18), (15, 11)]:
        assert np.abs(R[y, x] - F.polyexp_pixel(I, x, y, p)).max() < 1e-9, (x, y)
    assert np.abs(R - F.polyexp(I)).max() > 1.0, "another window, another fit"


@pytest.mark.parametrize("W,H,scale,levels,sizes", [
    (264, 260, 0.5, 3, [(264, 260), (132, 130), (66, 65), (33, 32)]),     # 32.5 rounds to even, as lrint does
    (264, 260, 0.5, 5, [(264, 260), (132, 130), (66, 65), (33, 32)]),     # min_size 32 ends it
    (124, 108, 0.8, 5, [(124, 108), (99, 86), (79, 69), (63, 55), (51, 44), (41, 35)]),
    (124, 108, 0.3, 0, [(124, 108)]),
    (124, 108, 0.9, 6, [(124, 108), (112, 97), (100, 87), (90, 79), (81, 71), (73, 64), (66, 57)]),
])
def test_levels_and_sizes_other_scales(oracle_lib, W, H, scale, levels, sizes):
    p = F.Params(pyr_scale=scale, levels=levels)
    L = len(sizes) - 1
    assert F.levels(W, H, p) == L == oracle_lib._of_lib().oc_fb_levels(W, H, scale, levels)
    assert [F.level_size(W, H, k, p) for k in range(L + 1)] == sizes
    g = np.zeros((H, W), np.uint8)
    for k in range(L + 1):
        assert oracle_lib.fb_level_poly(g, k, pyr_scale=scale).shape == sizes[k][::-1] + (5,)


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


# ------------------------------------------------- non-default parameter sets --
def _oracle_kw(p):
    return dict(pyr_scale=p.pyr_scale, poly_n=p.poly_n, poly_sigma=p.poly_sigma)


def measure_param_set(oracle_lib, ps):
    """Every oracle-vs-float64 figure of one parameter set over its cases: the
    expansion at every level, the coarsest level's first iteration and the
    final flow (both box orders each), the share of pixels near the threshold,
    the median error against the true translation, and the float64 distance to
    the neighbouring set."""
    p = ps.p
    out = dict(poly=0.0, iter=0.0, flow=0.0, near=0.0, median=0.0, margin=np.inf, mask_ok=True)
    for W, H, dx, dy in ps.cases:
        g0, g1, polys, want = F.flow_case(W, H, dx, dy, p)
        L = F.levels(W, H, p)
        for k in range(L + 1):
            for i, g in enumerate((g0, g1)):
                got = oracle_lib.fb_level_poly(g, k, **_oracle_kw(p))
                assert got.shape == polys[i, k].shape == F.level_size(W, H, k, p)[::-1] + (5,), (k, got.shape)
                out["poly"] = max(out["poly"], float(np.abs(got - polys[i, k]).max()))
        R0, R1 = (oracle_lib.fb_level_poly(g, L, **_oracle_kw(p)) for g in (g0, g1))
        zero = np.zeros(R0.shape[:2] + (2,), np.float32)
        want_it = F.iteration(polys[0, L], polys[1, L], zero, p)
        mag = np.hypot(want[..., 0], want[..., 1])
        for sliding in (True, False):
            got = oracle_lib.fb_iteration(R0, R1, zero, winsize=p.winsize, sliding=sliding)
            out["iter"] = max(out["iter"], float(np.abs(got - want_it).max()))
            got = oracle_lib.farneback(g0, g1, sliding=sliding, **p.kwargs())
            out["flow"] = max(out["flow"], float(np.abs(got - want).max()))
            differ = (np.hypot(got[..., 0], got[..., 1]) > F.FLOW_THRESHOLD) != (mag > F.FLOW_THRESHOLD)
            out["mask_ok"] &= not (differ & (np.abs(mag - F.FLOW_THRESHOLD) > ps.flow_tol)).any()
        out["near"] = max(out["near"], float((np.abs(mag - F.FLOW_THRESHOLD) <= ps.flow_tol).mean()))
        err = want[16:-16, 16:-16] - np.array([dx, dy])
        out["median"] = max(out["median"], float(np.median(np.hypot(err[..., 0], err[..., 1]))))
        other = F.flow_case(W, H, dx, dy, ps.neighbour)[3]
        out["margin"] = min(out["margin"], float(np.abs(want - other).max()))
    return out


@pytest.mark.parametrize("name", sorted(F.PARAM_SETS))
def test_param_set_vs_float64(oracle_lib, name):
    """The oracle at a non-default point of the space dvc_of_create accepts:
    expansion, first iteration and final flow against float64, both box orders,
    within 8 x the error measured for this set (the table of farneback_ref.py);
    the raw mask may differ only within that tolerance of the threshold, on
    under 0.1 % of the pixels."""
    ps = F.PARAM_SETS[name]
    m = measure_param_set(oracle_lib, ps)
    _report(f"{name} polyexp", m["poly"], ps.poly_tol)
    _report(f"{name} iteration", m["iter"], ps.iter_tol)
    _report(f"{name} flow", m["flow"], ps.flow_tol)
    print(f"{name}: near the threshold {m['near']:.2e}, median error against the truth {m['median']:.4f} px")
    assert m["poly"] <= ps.poly_tol and m["iter"] <= ps.iter_tol and m["flow"] <= ps.flow_tol
    assert m["near"] < F.MASK_EXCUSED_SHARE and m["mask_ok"]
    assert m["median"] < F.FLOW_TRUTH_MEDIAN


@pytest.mark.parametrize("name", sorted(F.PARAM_SETS))
def test_param_set_discriminates(name):
    """No mutation needed: the float64 flow of the set differs from the float64
    flow of its nearest accepted neighbour (the default, or the adjacent value)
    by at least 10 x the set's tolerance on every case, so code that ignored
    the parameter — or scaled an even box by its odd window — cannot pass."""
    ps = F.PARAM_SETS[name]
    assert ps.neighbour != ps.p
    for W, H, dx, dy in ps.cases:
        a, b = F.flow_case(W, H, dx, dy, ps.p)[3], F.flow_case(W, H, dx, dy, ps.neighbour)[3]
        margin = float(np.abs(a - b).max())
        print(f"{name} {W}x{H}: max |flow - neighbour's| {margin:.3e} (10 x tolerance {10 * ps.flow_tol:.3e})")
        assert margin >= 10 * ps.flow_tol
        assert margin >= 0.999 * ps.margin, "the table's margin is the smallest over the cases"
    for measured, tol in ((ps.poly_measured, ps.poly_tol), (ps.iter_measured, ps.iter_tol),
                          (ps.flow_measured, ps.flow_tol)):
        assert measured > 0 and tol == 8 * measured


def test_winsize1_vs_float64(oracle_lib):
    """winsize 1 (m = 0), each box order against what it computes in exact
    arithmetic: the running sums against float64 with OpenCV's start of the
    sums written in (the pixel plus row 0, column 0 and the corner), the direct
    sums against the one-pixel box. The two differ by pixels from each other —
    by definition, not by rounding (the comment above farneback_ref.W1_CASE)."""
    W, H, dx, dy = F.W1_CASE
    p = F.Params(winsize=1)
    g0, g1, polys, running, direct = F.winsize1_case()
    R0, R1 = polys[0].astype(np.float32), polys[1].astype(np.float32)
    zero = np.zeros((H, W, 2), np.float32)
    for sliding, want, it_m, flow_m in ((True, running, F.W1_RUNNING_ITER_MEASURED, F.W1_RUNNING_FLOW_MEASURED),
                                        (False, direct, F.W1_DIRECT_ITER_MEASURED, F.W1_DIRECT_FLOW_MEASURED)):
        name = "winsize1 " + ("running sums" if sliding else "direct sums")
        got = oracle_lib.fb_iteration(R0, R1, zero, winsize=1, sliding=sliding)
        err = float(np.abs(got - F.iteration(R0, R1, zero, p, running_sums=sliding)).max())
        _report(name + " iteration", err, 8 * it_m)
        assert err <= 8 * it_m
        got = oracle_lib.farneback(g0, g1, sliding=sliding, **p.kwargs())
        err = float(np.abs(got - want).max())
        _report(name + " flow", err, 8 * flow_m)
        assert err <= 8 * flow_m
        mag = np.hypot(want[..., 0], want[..., 1])
        near = np.abs(mag - F.FLOW_THRESHOLD) <= 8 * flow_m
        differ = (np.hypot(got[..., 0], got[..., 1]) > F.FLOW_THRESHOLD) != (mag > F.FLOW_THRESHOLD)
        print(f"{name}: near the threshold {near.mean():.2e}")
        assert not (differ & ~near).any()
        margin = float(np.abs(want - F.flow_case(W, H, dx, dy)[3]).max())
        print(f"{name}: max |flow - the default's| {margin:.3e}")
        assert margin >= F.W1_MARGIN >= 10 * 8 * flow_m
    between = float(np.abs(running - direct).max())
    print(f"winsize1: running vs direct sums in float64 {between:.3e} px")
    assert between > 1.0


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
