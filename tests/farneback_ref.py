"""Independent float64 formulation of the optical-flow path — test helper.

Written from Farnebäck's two-frame motion estimation ("Two-Frame Motion
Estimation Based on Polynomial Expansion", SCIA 2003) and the documented
parameters of ``cv2.calcOpticalFlowFarneback(prev, next, None, 0.3, 2, 9, 2,
5, 1.1, 0)``, in plain NumPy / scipy float64. It shares no code with
``oracle/of_oracle.c`` or the HIP kernels: the polynomial expansion solves the
full 6x6 weighted normal equations per pixel, the update step is written with
2x2 matrices, the box is ``ndimage.uniform_filter``, the morphology is shifted
max / min, the rectangles come from ``ndimage.label``.

Where the definition leaves a choice open and OpenCV makes one, the choice is
encoded here with a comment naming the place in OpenCV 4.x
(``modules/video/src/optflowgf.cpp`` unless stated otherwise).

``tests/test_of_oracle.py`` (CPU) checks the oracle against this module and
``tests/test_of_reference_gpu.py`` checks the HIP kernels against it directly.
"""
from __future__ import annotations

import dataclasses
import functools
from collections import deque

import numpy as np
from scipy import fft, ndimage

PYR_SCALE = 0.3
MIN_SIZE = 32          # calcOpticalFlowFarneback: const int min_size = 32
MAX_LEVELS = 2         # the reference's `levels` argument: extra levels above level 0
WINSIZE = 9
ITERATIONS = 2
POLY_N = 5             # window radius: (2 * 5 + 1)^2 = 11 x 11
POLY_SIGMA = 1.1
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)   # FarnebackUpdateMatrices: `static const float border[]`


@dataclasses.dataclass(frozen=True)
class Params:
    """The six calcOpticalFlowFarneback arguments; the defaults are the module
    constants above (what the reference passes). Frozen and hashable: a key of
    :func:`flow_case`'s cache. ``kwargs()`` are the keywords OFWorker, OracleOF
    and oracle.farneback take."""
    pyr_scale: float = PYR_SCALE
    levels: int = MAX_LEVELS
    winsize: int = WINSIZE
    iterations: int = ITERATIONS
    poly_n: int = POLY_N
    poly_sigma: float = POLY_SIGMA

    def kwargs(self) -> dict:
        return dataclasses.asdict(self)


DEFAULT = Params()

# Shapes of the comparisons (W, H): one level; L = 1 with an odd coarse level;
# L = 2 with level sizes 109 x 107 and 33 x 32; the GPU adds a partial strip.
SHAPES_CPU = ((96, 64), (124, 108), (364, 356))
SHAPES_GPU = ((96, 64), (136, 72), (124, 108), (364, 356))

# ---------------------------------------------------------------------------
# Measured float32-vs-float64 errors and the tolerances derived from them.
#
# *_MEASURED: the largest |oracle - this module| over every case of the
# matching test in tests/test_of_oracle.py (all levels of SHAPES_CPU, both box
# orders where there is a box), measured on the CPU; each test prints its
# figure. *_TOL = 8 x measured, the headroom for another float32 summation
# order; every tolerance must stay below a tenth of *_MUTATION_MIN
# (test_tolerances_discriminate).
#
# *_MUTATION_MIN comes from eight single-constant mutations of of_oracle.c,
# applied one at a time to a scratch copy (never committed), each of which
# fails tests/test_of_oracle.py. Largest error of each comparison over its
# cases (weakest affected case in brackets; "-" where the stage is untouched):
#
#   mutation                        polyexp        iteration       flow [px]
#   poly_sigma 1.1 -> 1.15          1.86  (0.27)   0.038 (0.014)   0.167 (0.0125)
#   border table .4472 -> .5        -              0.90  (0.44)    0.53  (0.104)
#   pyramid sigma factor .5 -> .45  0.87  (0.53)   0.0099 (0.0039) 0.088 (0.00106)
#   resize without half-pixel       10.8  (9.7)    0.18  (0.081)   0.27  (0.054)
#   xy coefficient x.25 -> x.5      -              4.4   (1.2)     1.40  (0.34)
#   blur reflect -> replicate       1.79  (1.12)   0.15  (0.0052)  0.53  (0.129)
#   box 9 -> 7                      -              7.4   (2.6)     1.72  (0.52)
#   upscale 1/0.3 -> 3              -              -               0.26  (0.069)
#
# (The iteration column of a pyramid or expansion mutation is the sub-case that
# feeds the oracle's own expansions in.) *_MUTATION_MIN is the smallest
# bracketed figure of its column: the weakest case any mutation leaves.
#
# The polynomial coefficients have a value scale of ~30 (gray levels per
# pixel); the flows are in pixels.
#
# The figures above are the reference's arguments (0.3, 2, 9, 2, 5, 1.1). The
# other argument sets dvc_of_create accepts have one row each in PARAM_SETS
# further down (it needs Params): measured error, 8 x tolerance and the margin
# to the nearest accepted neighbour, and the answer on winsize 1 in words.
POLY_MEASURED = 5.5e-5        # 5.40e-5 at 364 x 356
POLY_TOL = 8 * POLY_MEASURED
POLY_MUTATION_MIN = 0.27
ITER_MEASURED = 1.8e-5        # 1.76e-5 at level 1 of 364 x 356 (109 x 107)
ITER_TOL = 8 * ITER_MEASURED
ITER_MUTATION_MIN = 3.9e-3
FLOW_MEASURED = 1.2e-5        # 1.11e-5 at 364 x 356, (-2.3, 1.6)
FLOW_TOL = 8 * FLOW_MEASURED
FLOW_MUTATION_MIN = 1.05e-3
# Sanity bound on what the algorithm does (median interior error against the
# true translation); not a rounding tolerance.
FLOW_TRUTH_MEDIAN = 0.05
FLOW_THRESHOLD = 0.5
MASK_EXCUSED_SHARE = 1e-3


# ------------------------------------------------------------------ pyramid --
def levels(W: int, H: int, p: Params = DEFAULT) -> int:
    """Number of extra pyramid levels: scale *= pyr_scale while both sides stay >= min_size."""
    scale, k = 1.0, 0
    while k < p.levels:
        scale *= p.pyr_scale
        if W * scale < MIN_SIZE or H * scale < MIN_SIZE:
            break
        k += 1
    return k


def gauss_taps(ksize: int, sigma: float) -> np.ndarray:
    """cv2.getGaussianKernel: the fixed [1/4, 1/2, 1/4] table for sigma <= 0 at
    ksize 3 (imgproc/src/smooth.dispatch.cpp, small_gaussian_tab), else the
    normalised samples of exp(-x^2 / 2 sigma^2)."""
    if sigma <= 0:
        assert ksize == 3
        return np.array([0.25, 0.5, 0.25])
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2
    g = np.exp(-x * x / (2 * sigma * sigma))
    return g / g.sum()


def resize_linear(img: np.ndarray, dw: int, dh: int) -> np.ndarray:
    """cv2.resize INTER_LINEAR: sample at (d + 0.5) * (src / dst) - 0.5, the
    coordinate clamped to the image; img is (h, w) or (h, w, c)."""
    sh, sw = img.shape[:2]
    if (sw, sh) == (dw, dh):
        return np.array(img, dtype=np.float64)
    fx = np.clip((np.arange(dw) + 0.5) * (sw / dw) - 0.5, 0, sw - 1)
    fy = np.clip((np.arange(dh) + 0.5) * (sh / dh) - 0.5, 0, sh - 1)
    x0 = np.minimum(np.floor(fx).astype(int), max(sw - 2, 0))
    y0 = np.minimum(np.floor(fy).astype(int), max(sh - 2, 0))
    x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
    ax, ay = fx - x0, fy - y0
    if img.ndim == 3:
        ax, ay = ax[:, None], ay[:, None]
    img = np.asarray(img, dtype=np.float64)
    rows = img[y0] * (1 - ay)[:, None] + img[y1] * ay[:, None]        # (dh, sw[, c])
    return rows[:, x0] * (1 - ax)[None] + rows[:, x1] * ax[None]


def level_size(W: int, H: int, k: int, p: Params = DEFAULT):
    scale = p.pyr_scale ** k
    return int(np.rint(W * scale)), int(np.rint(H * scale))


def level_image(gray: np.ndarray, k: int, p: Params = DEFAULT) -> np.ndarray:
    """Level k of the pyramid: the full-size image blurred with sigma =
    (1 / scale - 1) / 2 (REFLECT_101 = scipy's 'mirror'), then resized."""
    H, W = gray.shape
    sigma = (1.0 / p.pyr_scale ** k - 1) * 0.5
    ksize = max(int(np.rint(sigma * 5)) | 1, 3)
    taps = gauss_taps(ksize, sigma)
    img = gray.astype(np.float64)
    img = ndimage.correlate1d(img, taps, axis=1, mode="mirror")
    img = ndimage.correlate1d(img, taps, axis=0, mode="mirror")
    w, h = level_size(W, H, k, p)
    return resize_linear(img, w, h)


# ------------------------------------------------------ polynomial expansion --
def _poly_basis(p: Params = DEFAULT):
    """Window offsets, applicability and the basis (1, x, y, x^2, y^2, xy)."""
    o = np.arange(-p.poly_n, p.poly_n + 1, dtype=np.float64)
    g = np.exp(-o * o / (2 * p.poly_sigma ** 2))
    return o, g / g.sum()


def polyexp(I: np.ndarray, p: Params = DEFAULT) -> np.ndarray:
    """Gaussian-weighted least-squares fit of c + bx x + by y + axx x^2 +
    ayy y^2 + axy xy over the (2 poly_n + 1)^2 window (11 x 11 by default) of
    every pixel (replicated
    borders): r = (B^T W B)^-1 B^T W f with the full 6 x 6 Gram matrix.
    Returns (h, w, 5): by, bx, ayy, axx, axy (the project's channel order)."""
    o, g = _poly_basis(p)
    I = np.asarray(I, dtype=np.float64)
    px = [np.ones_like(o), o, o * o]
    # basis functions as (power of x, power of y)
    basis = [(0, 0), (1, 0), (0, 1), (2, 0), (0, 2), (1, 1)]
    Y, X = np.meshgrid(o, o, indexing="ij")
    Wt = np.outer(g, g)
    Bm = np.stack([X ** a * Y ** b for a, b in basis], axis=-1).reshape(-1, 6)     # ((2 n + 1)^2, 6)
    G = Bm.T @ (Wt.reshape(-1, 1) * Bm)                                             # B^T W B
    # B^T W f: the weight g(x) g(y) x^a y^b separates into a row and a column pass
    moments = np.empty(I.shape + (6,))
    for j, (a, b) in enumerate(basis):
        t = ndimage.correlate1d(I, g * px[a], axis=1, mode="nearest")
        moments[..., j] = ndimage.correlate1d(t, g * px[b], axis=0, mode="nearest")
    r = np.linalg.solve(G, moments.reshape(-1, 6).T).T.reshape(I.shape + (6,))
    return np.stack([r[..., 2], r[..., 1], r[..., 4], r[..., 3], r[..., 5]], axis=-1)


def polyexp_pixel(I: np.ndarray, x: int, y: int, p: Params = DEFAULT) -> np.ndarray:
    """The same fit at one pixel by weighted ``lstsq`` over the explicit 121
    (at poly_n 7: 225) samples — the definition itself, used to check
    :func:`polyexp`."""
    o, g = _poly_basis(p)
    H, W = I.shape
    ys = np.clip(y + o.astype(int), 0, H - 1)
    xs = np.clip(x + o.astype(int), 0, W - 1)
    f = np.asarray(I, dtype=np.float64)[np.ix_(ys, xs)].reshape(-1)
    Y, X = np.meshgrid(o, o, indexing="ij")
    Bm = np.stack([np.ones_like(X), X, Y, X * X, Y * Y, X * Y], axis=-1).reshape(-1, 6)
    sw = np.sqrt(np.outer(g, g)).reshape(-1)
    r = np.linalg.lstsq(Bm * sw[:, None], f * sw, rcond=None)[0]
    return np.array([r[2], r[1], r[4], r[3], r[5]])


# ------------------------------------------------------------- one iteration --
def border_scale(W: int, H: int) -> np.ndarray:
    def side(n):
        s = np.ones(n)
        for i, b in enumerate(BORDER):
            if i < n:
                s[i] *= b
                s[n - 1 - i] *= b
        return s
    return np.outer(side(H), side(W))


def _bilinear(R: np.ndarray, fx: np.ndarray, fy: np.ndarray):
    """R (h, w, c) sampled at (fx, fy); also whether the 2 x 2 cell is inside."""
    H, W = R.shape[:2]
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    inside = (x0 >= 0) & (x0 < W - 1) & (y0 >= 0) & (y0 < H - 1)
    xc, yc = np.clip(x0, 0, W - 2), np.clip(y0, 0, H - 2)
    ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]
    v = (R[yc, xc] * (1 - ax) + R[yc, xc + 1] * ax) * (1 - ay) + (R[yc + 1, xc] * (1 - ax) + R[yc + 1, xc + 1] * ax) * ay
    return v, inside


def displaced_inside(flow: np.ndarray) -> np.ndarray:
    """Where the 2 x 2 cell around x + d lies inside the image."""
    H, W = flow.shape[:2]
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x0, y0 = np.floor(xs + flow[..., 0]), np.floor(ys + flow[..., 1])
    return (x0 >= 0) & (x0 < W - 1) & (y0 >= 0) & (y0 < H - 1)


def iteration(R0: np.ndarray, R1: np.ndarray, flow: np.ndarray, p: Params = DEFAULT,
              running_sums: bool = False) -> np.ndarray:
    """One displacement update. With A = [[axx, axy/2], [axy/2, ayy]] and
    b = (bx, by) of each frame: A = (A0 + A1(x + d)) / 2, db = (b0 - b1(x + d))
    / 2 + A d, G = A^T A and h = A^T db averaged over the winsize x winsize box
    (9 x 9 by default; replicated borders), d = adj(G) h / (det G + 1e-3).
    ``running_sums`` matters at winsize 1 only (see below)."""
    R0, R1 = np.asarray(R0, np.float64), np.asarray(R1, np.float64)
    flow = np.asarray(flow, np.float64)
    H, W = R0.shape[:2]
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    S, inside = _bilinear(R1, xs + flow[..., 0], ys + flow[..., 1])
    # OpenCV's choice where the displaced cell leaves the image
    # (FarnebackUpdateMatrices, the `else` branch): A0 alone, and b1 taken as 0.
    m = inside[..., None]
    quad = np.where(m, (R0[..., 2:] + S[..., 2:]) / 2, R0[..., 2:])
    lin = (R0[..., :2] - np.where(m, S[..., :2], 0.0)) / 2
    ayy, axx, axy = quad[..., 0], quad[..., 1], quad[..., 2]
    A = np.empty((H, W, 2, 2))
    A[..., 0, 0], A[..., 0, 1], A[..., 1, 0], A[..., 1, 1] = axx, axy / 2, axy / 2, ayy
    db = np.stack([lin[..., 1], lin[..., 0]], axis=-1) + np.einsum("...ij,...j->...i", A, flow)
    s = border_scale(W, H)
    A, db = A * s[..., None, None], db * s[..., None]
    G = np.einsum("...ki,...kj->...ij", A, A)
    h = np.einsum("...ki,...k->...i", A, db)
    # OpenCV's choice for an even winsize (FarnebackUpdateFlow_Blur: `int m =
    # block_size/2`, `double scale = 1./(block_size*block_size)`): the sums run
    # over the odd window 2 (winsize // 2) + 1, yet are scaled by 1 / winsize^2.
    box = 2 * (p.winsize // 2) + 1
    rescale = (box * box) / float(p.winsize * p.winsize)
    G = ndimage.uniform_filter(G, size=(box, box, 1, 1), mode="nearest") * rescale
    h = ndimage.uniform_filter(h, size=(box, box, 1), mode="nearest") * rescale
    if running_sums and box == 1:
        # OpenCV's choice at winsize 1 (FarnebackUpdateFlow_Blur): it keeps
        # running sums, and starts the vertical one with `srow0[x]*(m+2)` plus
        # rows 1 ... m - 1 — the 2 m + 1 rows of the window above row 0. At m = 0
        # that window has one row, the start puts two, and the surplus copy of
        # row 0 never leaves the sum; the horizontal sum does the same with
        # column 0. What OpenCV solves at (y, x) is therefore the sum over (y, x),
        # (0, x), (y, 0) and (0, 0) — in exact arithmetic, not by rounding.
        G = G + G[:1] + G[:, :1] + G[:1, :1]
        h = h + h[:1] + h[:, :1] + h[:1, :1]
    # FarnebackUpdateFlow_Blur regularises the determinant, not the diagonal
    idet = 1.0 / (G[..., 0, 0] * G[..., 1, 1] - G[..., 0, 1] * G[..., 1, 0] + 1e-3)
    dx = (G[..., 1, 1] * h[..., 0] - G[..., 0, 1] * h[..., 1]) * idet
    dy = (G[..., 0, 0] * h[..., 1] - G[..., 1, 0] * h[..., 0]) * idet
    return np.stack([dx, dy], axis=-1)


def farneback(g0: np.ndarray, g1: np.ndarray, polys=None, p: Params = DEFAULT, running_sums: bool = False) -> np.ndarray:
    """Coarse to fine; ``polys(img_index, k)`` may supply cached expansions."""
    H, W = g0.shape
    flow = None
    for k in range(levels(W, H, p), -1, -1):
        if polys is None:
            R0, R1 = polyexp(level_image(g0, k, p), p), polyexp(level_image(g1, k, p), p)
        else:
            R0, R1 = polys(0, k), polys(1, k)
        h, w = R0.shape[:2]
        flow = np.zeros((h, w, 2)) if flow is None else resize_linear(flow, w, h) * (1.0 / p.pyr_scale)
        for _ in range(p.iterations):
            flow = iteration(R0, R1, flow, p, running_sums)
    return flow


# ------------------------------------------------------------------- inputs --
def textured_pair(W: int, H: int, dx: float, dy: float, seed: int):
    """Two uint8 frames of a sum of 24 random low-frequency sinusoids (wave
    vectors uniform in the disk |k| <= 0.35 rad/px: no flat regions, nothing
    the 11 x 11 window aliases), the second evaluated analytically at (x - dx,
    y - dy): the true flow is (dx, dy) everywhere. One common affine maps both
    to 20 ... 235."""
    rng = np.random.default_rng(seed)
    n = 24
    mag = 0.35 * np.sqrt(rng.uniform(0, 1, n))
    ang = rng.uniform(0, 2 * np.pi, n)
    kx, ky = mag * np.cos(ang), mag * np.sin(ang)
    ph = rng.uniform(0, 2 * np.pi, n)
    amp = rng.uniform(0.5, 1.0, n)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))

    def f(x, y):
        return np.einsum("n,nhw->hw", amp, np.sin(kx[:, None, None] * x + ky[:, None, None] * y + ph[:, None, None]))
    a, b = f(xs, ys), f(xs - dx, ys - dy)
    lo, hi = min(a.min(), b.min()), max(a.max(), b.max())
    to8 = lambda v: np.rint(20 + (v - lo) * (215.0 / (hi - lo))).astype(np.uint8)
    return to8(a), to8(b)


def gray_bgr(g: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=-1))


# Translations (dx, dy) per shape: a sub-pixel and a multi-pixel one, both
# signs on both axes across the set. The estimate is biased towards zero by the
# regularised determinant and gets two iterations a level, so its error
# against the truth grows with the displacement: in float64 it passes
# FLOW_TRUTH_MEDIAN near |d| = 3 px at these sizes, whatever the rounding.
# The multi-pixel cases therefore stay at 2 ... 2.8 px.
FLOW_CASES = {
    (96, 64): ((0.6, -0.4), (-1.3, 0.9)),
    (136, 72): ((-0.5, 0.7),),
    (124, 108): ((0.7, 0.3), (1.7, -1.2)),
    (364, 356): ((-0.45, 0.8), (-2.3, 1.6)),
}


@functools.lru_cache(maxsize=None)
def flow_case(W: int, H: int, dx: float, dy: float, p: Params = DEFAULT):
    """(g0, g1, {(frame, level): polyexp}, flow) of one textured pair, computed
    once a session and shared read-only by every test that needs it."""
    g0, g1 = textured_pair(W, H, dx, dy, seed=W + H)
    polys = {(i, k): polyexp(level_image(g, k, p), p) for k in range(levels(W, H, p) + 1)
             for i, g in enumerate((g0, g1))}
    flow = farneback(g0, g1, polys=lambda i, k: polys[i, k], p=p)
    for a in (g0, g1, flow, *polys.values()):
        a.setflags(write=False)
    return g0, g1, polys, flow


# ------------------------------------------------- non-default parameter sets --
@dataclasses.dataclass(frozen=True)
class ParamSet:
    """One point of the parameter space dvc_of_create accepts, with the inputs
    it is checked on and the figures measured there (the table below)."""
    p: Params
    neighbour: Params            # the nearest accepted set its flow must differ from
    cases: tuple                 # (W, H, dx, dy) textured pairs: CPU and GPU float64 comparisons
    poly_measured: float
    iter_measured: float
    flow_measured: float
    margin: float                # smallest max |flow(p) - flow(neighbour)| over the cases, float64

    @property
    def poly_tol(self):
        return 8 * self.poly_measured

    @property
    def iter_tol(self):
        return 8 * self.iter_measured

    @property
    def flow_tol(self):
        return 8 * self.flow_measured


# The median error of the float64 flow against the true translation stays under
# FLOW_TRUTH_MEDIAN on every case below (0.015 ... 0.044 px; the displacements
# are chosen for that: at (-2.3, 1.6) pyr_scale 0.5 measures 0.052), and no
# pixel of a case lies within its tolerance of the 0.5 threshold.
#
# winsize 1 is not in the table; it has constants of its own. The question was
# why the oracle's running sums and its direct sums differ by 7.7 px there, and
# from the float64 definition by as much. Answer: neither rounding nor an
# oracle defect. In exact arithmetic OpenCV's running sums do not compute the
# one-pixel box at m = 0 (the start `srow0[x]*(m+2)` of FarnebackUpdateFlow_Blur
# assumes m >= 1, see iteration()): they solve G and h summed over (y, x),
# (0, x), (y, 0) and (0, 0). With that start written into iteration(...,
# running_sums=True) the oracle's running sums agree with float64 to 1.4e-5
# (one iteration) and 9.8e-5 px (final flow, 96 x 64, (-1.3, 0.9)): the same
# chain as any other winsize, the larger figure coming from the update itself.
# The direct sums do compute the one-pixel box, and there G = A^T A has det G =
# det(A)^2: on that frame 22 % of the pixels have det G below the 1e-3
# regulariser (median 0.025), so the update amplifies float32 rounding. Oracle
# direct sums vs float64: 2.9e-4 (iteration) and 8.1e-4 px (flow), the worst
# pixel at det G = 5.9e-6; restricted to det G >= 0.1 the iteration differs by
# 4.7e-6, to det G >= 1 by 6.2e-7 — ill-conditioning, not a defect. Neither
# order estimates the translation (median error 0.25 and 0.11 px), so winsize 1
# is held to float64 in both orders but exempt from FLOW_TRUTH_MEDIAN.
W1_CASE = (96, 64, -1.3, 0.9)
W1_RUNNING_ITER_MEASURED = 1.4e-5
W1_RUNNING_FLOW_MEASURED = 9.8e-5      # tolerance 7.9e-4; margin to the default's flow 5.0 px
W1_DIRECT_ITER_MEASURED = 2.9e-4
W1_DIRECT_FLOW_MEASURED = 8.1e-4       # tolerance 6.5e-3; margin to the default's flow 19.9 px
W1_MARGIN = 5.0

_C124, _C96, _C136, _C264, _C333 = (124, 108, 1.3, -0.9), (96, 64, -1.3, 0.9), (136, 76, 1.1, -0.8), \
    (264, 260, -1.7, 1.2), (333, 185, 1.4, -0.9)
_P7 = Params(poly_n=7, poly_sigma=1.5)
_ALL = Params(0.5, 3, 13, 3, 7, 1.5)

PARAM_SETS = {
    # name: parameters, neighbour, cases, then the largest |oracle - this module| over the cases and both
    # box orders for the expansion (every level), the coarsest level's first iteration and the final flow
    # [px]; each tolerance is 8 x its figure (flow tolerance in the comment); last the margin: the smallest
    # max |flow - the neighbour's flow| over the cases in float64, which must be >= 10 x the flow tolerance
    # (test_param_set_discriminates). Measured on the CPU by tests/test_of_oracle.py, which prints each.
    "poly7": ParamSet(_P7, Params(poly_sigma=1.5), (_C124, _C333),
                      2.6e-5, 1.3e-6, 7.8e-6, 0.0129),          # tol 6.2e-5 px; vs poly_n 5 at sigma 1.5
    "winsize5": ParamSet(Params(winsize=5), DEFAULT, (_C124,),
                         2.0e-5, 2.1e-6, 1.3e-5, 2.24),         # tol 1.0e-4 px
    "winsize8": ParamSet(Params(winsize=8), DEFAULT, (_C124,),
                         2.0e-5, 5.9e-7, 5.0e-6, 0.314),        # tol 4.0e-5 px; vs 9: same window, scale 1/64
    "winsize13": ParamSet(Params(winsize=13), DEFAULT, (_C124,),
                          2.0e-5, 3.7e-7, 2.8e-6, 1.15),        # tol 2.2e-5 px
    "winsize17": ParamSet(Params(winsize=17), Params(winsize=15), (_C124, _C136),
                          2.0e-5, 1.9e-6, 2.6e-6, 0.219),       # tol 2.1e-5 px; vs winsize 15
    "iterations1": ParamSet(Params(iterations=1), DEFAULT, (_C124, _C96),
                            2.0e-5, 3.7e-6, 4.7e-6, 0.612),     # tol 3.8e-5 px
    "iterations3": ParamSet(Params(iterations=3), DEFAULT, (_C124,),
                            2.0e-5, 6.1e-7, 4.6e-6, 0.183),     # tol 3.7e-5 px
    "pyr0.5_levels3": ParamSet(Params(pyr_scale=0.5, levels=3), DEFAULT, (_C264,),
                               1.5e-5, 4.5e-7, 1.3e-5, 0.132),  # tol 1.0e-4 px; L = 3: 132x130, 66x65, 33x32
    "pyr0.8_levels5": ParamSet(Params(pyr_scale=0.8, levels=5), DEFAULT, (_C124,),
                               2.8e-5, 7.7e-7, 4.8e-6, 0.211),  # tol 3.8e-5 px; L = 5, coarsest 41x35
    "levels0": ParamSet(Params(levels=0), DEFAULT, (_C124,),
                        1.3e-5, 6.4e-6, 5.2e-6, 0.313),         # tol 4.2e-5 px
    "all": ParamSet(_ALL, DEFAULT, (_C264,),
                    1.3e-5, 5.2e-7, 4.3e-6, 1.52),              # tol 3.4e-5 px
}


@functools.lru_cache(maxsize=None)
def winsize1_case():
    """(g0, g1, {frame: polyexp}, flow as OpenCV's running sums give it, flow by
    the one-pixel box) of W1_CASE in float64, read-only."""
    W, H, dx, dy = W1_CASE
    p = Params(winsize=1)
    assert levels(W, H, p) == 0
    g0, g1 = textured_pair(W, H, dx, dy, seed=W + H)
    polys = {i: polyexp(level_image(g, 0, p), p) for i, g in enumerate((g0, g1))}
    flows = [farneback(g0, g1, polys=lambda i, k: polys[i], p=p, running_sums=r) for r in (True, False)]
    for a in (g0, g1, *flows, *polys.values()):
        a.setflags(write=False)
    return g0, g1, polys, flows[0], flows[1]


# --------------------------------------------- vote, morphology, rectangles --
def ellipse(k: int) -> np.ndarray:
    """cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)) (imgproc/src/
    morph.dispatch.cpp): r = c = k // 2; row i spans c - dx ... c + dx with dx =
    round(c * sqrt(1 - (i - r)^2 / r^2)) clipped to the element, and is empty
    where |i - r| > r."""
    r = c = k // 2
    el = np.zeros((k, k), np.uint8)
    for i in range(k):
        dy = i - r
        if abs(dy) > r:
            continue
        dx = int(np.rint(c * np.sqrt((r * r - dy * dy) / (r * r)))) if r else 0
        el[i, max(c - dx, 0):min(c + dx + 1, k)] = 1
    return el


def _morph(m: np.ndarray, el: np.ndarray, dilate: bool) -> np.ndarray:
    """out(y, x) = max / min of m(y + i - a, x + j - a) over el[i, j] != 0 with
    anchor a = k // 2; pixels outside the image do not take part."""
    k = el.shape[0]
    a = k // 2
    H, W = m.shape
    out = np.full_like(m, 0 if dilate else 255)
    for i, j in zip(*np.nonzero(el)):
        sy, sx = i - a, j - a
        ys = slice(max(0, -sy), min(H, H - sy))
        xs = slice(max(0, -sx), min(W, W - sx))
        yd = slice(ys.start + sy, ys.stop + sy)
        xd = slice(xs.start + sx, xs.stop + sx)
        if ys.start >= ys.stop or xs.start >= xs.stop:
            continue
        op = np.maximum if dilate else np.minimum
        out[ys, xs] = op(out[ys, xs], m[yd, xd])
    return out


def close_open(m: np.ndarray, k: int, el: np.ndarray | None = None) -> np.ndarray:
    """MORPH_CLOSE then MORPH_OPEN: dilate, erode, erode, dilate."""
    el = ellipse(k) if el is None else el
    m = np.ascontiguousarray(m, np.uint8)
    return _morph(_morph(_morph(_morph(m, el, True), el, False), el, False), el, True)


def rectangles(m: np.ndarray):
    """Union of the bounding rectangles of the 8-connected components, each
    grown one pixel right and down (cv2.rectangle's inclusive far corner at
    (x + w, y + h)); returns (mask, number of components)."""
    lab, n = ndimage.label(m > 0, structure=np.ones((3, 3)))
    out = np.zeros(m.shape, np.uint8)
    for sl in ndimage.find_objects(lab):
        out[sl[0].start:sl[0].stop + 1, sl[1].start:sl[1].stop + 1] = 255
    return out, n


def vote(raw_masks, window: int, alpha: float) -> np.ndarray:
    """The reference's expression on its deque of 0 / 255 masks."""
    q = deque(maxlen=window)
    for m in raw_masks:
        q.append(m)
    cum = np.sum(np.array(q), axis=0)
    return (cum >= (alpha * len(q) * 255)).astype(np.uint8) * 255


def vote_threshold(alpha: float, L: int) -> int:
    """Smallest count c of 255s with c * 255 >= alpha * L * 255 (L + 1: none)."""
    for c in range(L + 1):
        if c * 255 >= (alpha * L * 255):
            return c
    return L + 1


# -------------------------------------------------------------- compression --
def bgr2ycrcb(bgr: np.ndarray, rounded: bool = True) -> np.ndarray:
    """Y = 0.299 R + 0.587 G + 0.114 B, Cr = (R - Y) 0.713 + 128, Cb = (B - Y)
    0.564 + 128 (cv2.cvtColor's documented 8-bit formulas). The 8-bit path
    forms Cr and Cb from the rounded Y (imgproc/src/color_yuv.simd.hpp,
    RGB2YCrCb_i)."""
    b, g, r = (bgr[..., i].astype(np.float64) for i in range(3))
    y = 0.299 * r + 0.587 * g + 0.114 * b
    yr = np.rint(y)
    ycc = np.stack([y, (r - yr) * 0.713 + 128, (b - yr) * 0.564 + 128], axis=-1)
    return np.clip(np.rint(ycc), 0, 255).astype(np.uint8) if rounded else ycc


def ycrcb2bgr(ycc: np.ndarray) -> np.ndarray:
    """R = Y + 1.403 (Cr - 128), G = Y - 0.714 (Cr - 128) - 0.344 (Cb - 128),
    B = Y + 1.773 (Cb - 128), rounded and saturated."""
    y, cr, cb = (ycc[..., i].astype(np.float64) for i in range(3))
    cr, cb = cr - 128, cb - 128
    bgr = np.stack([y + 1.773 * cb, y - 0.714 * cr - 0.344 * cb, y + 1.403 * cr], axis=-1)
    return np.clip(np.rint(bgr), 0, 255).astype(np.uint8)


def tie_free_bgr(W: int, H: int, seed: int, margin: float = 0.03) -> np.ndarray:
    """A colour test image (smooth colour waves plus +-12 levels of noise, so a
    handful of DCT coefficients per block survive quantisation at 100) whose
    float64 Y, Cr and Cb all lie further than `margin` from a rounding tie.
    OpenCV's 8-bit conversion uses constants rounded to 14 fractional bits
    (error <= 2^-15 each, <= 3 * 255 * 2^-15 = 0.023 on Y), so away from ties
    it rounds to the same integers as the float64 formulas and the DCT stage of
    both sides sees the same planes; the test asserts that this is so."""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    img = np.empty((H, W, 3))
    for c in range(3):
        kx, ky, ph = rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(0, 6.28)
        img[..., c] = 128 + 90 * np.sin(kx * xs + ky * ys + ph) + rng.uniform(-12, 12, (H, W))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    for _ in range(200):
        v = bgr2ycrcb(img, rounded=False)       # unrounded Y; Cr, Cb from the rounded Y
        bad = (np.abs(v - np.floor(v) - 0.5) < margin).any(axis=-1)
        if not bad.any():
            return img
        img[bad] = np.clip(img[bad].astype(int) + rng.integers(-3, 4, (int(bad.sum()), 3)), 0, 255).astype(np.uint8)
    raise AssertionError("no tie-free image found")


def compress(bgr: np.ndarray, mask: np.ndarray, q: float = 100.0):
    """compress_with_motion for one frame in float64, uint8 at the stage
    boundaries the reference has: BGR -> YCrCb; every full 8 x 8 block whose
    mask is all zero gets Y, Cr and Cb through dctn(block - 128), round(. / q)
    * q, idctn + 128, clip, truncating uint8 store; YCrCb -> BGR; static blocks
    BGR -> gray -> BGR. Returns (out, static (H/8, W/8) bool, near_tie (H/8,
    W/8) bool: some coefficient / q within 1e-4 of a .5 tie)."""
    H, W = mask.shape
    ycc = bgr2ycrcb(bgr)
    nby, nbx = H // 8, W // 8
    static = np.zeros((nby, nbx), bool)
    near_tie = np.zeros((nby, nbx), bool)
    for by in range(nby):
        for bx in range(nbx):
            sl = (slice(8 * by, 8 * by + 8), slice(8 * bx, 8 * bx + 8))
            if mask[sl].mean() != 0:
                continue
            static[by, bx] = True
            for c in range(3):
                d = fft.dctn(ycc[sl + (c,)].astype(np.float64) - 128, norm="ortho")
                near_tie[by, bx] |= bool((np.abs(np.abs(d / q) % 1 - 0.5) < 1e-4).any())
                rec = fft.idctn(np.round(d / q) * q, norm="ortho") + 128
                ycc[sl + (c,)] = np.clip(rec, 0, 255).astype(np.uint8)
    out = ycrcb2bgr(ycc)
    for by, bx in zip(*np.nonzero(static)):
        sl = (slice(8 * by, 8 * by + 8), slice(8 * bx, 8 * bx + 8))
        b, g, r = (out[sl + (i,)].astype(np.float64) for i in range(3))
        out[sl] = np.rint(0.299 * r + 0.587 * g + 0.114 * b).astype(np.uint8)[..., None]
    return out, static, near_tie


def half_static_mask(W, H, seed):
    """Left half static; right half with blobs; one static-side block gated by
    a single faint pixel; the partial edge blocks left at zero."""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.uint8)
    right = np.repeat(np.repeat(rng.random((H // 4 + 1, W // 4 + 1)) < 0.35, 4, axis=0), 4, axis=1)[:H, :W]
    m[:, W // 2:] = right[:, W // 2:] * 255
    m[H // 8 * 8:, :] = 0
    m[:, W // 8 * 8:] = 0
    m[11, 13] = 1
    return m


def check_compress(got, bgr, mask, roundtrip_exact=None):
    """The rules of the float64 comparison, shared with the GPU test."""
    H, W = mask.shape
    want, static, near_tie = compress(bgr, mask)
    assert static.any() and not static.all()
    assert not static[1, 1], "a single nonzero mask pixel keeps its block moving"
    spx = np.zeros((H, W), bool)
    spx[:H // 8 * 8, :W // 8 * 8] = np.repeat(np.repeat(static, 8, axis=0), 8, axis=1)
    excused = np.zeros((H, W), bool)
    excused[:H // 8 * 8, :W // 8 * 8] = np.repeat(np.repeat(near_tie, 8, axis=0), 8, axis=1)
    share = near_tie[static].mean()
    diff = np.abs(got.astype(int) - want.astype(int)).max(axis=-1)
    print(f"of_compress {W}x{H}: {int(static.sum())} static blocks, {share:.2%} excused, "
          f"max diff static {diff[spx & ~excused].max()}, elsewhere {diff[~spx].max()}")
    assert share <= 0.02
    g = got[spx]
    assert (g[:, 0] == g[:, 1]).all() and (g[:, 1] == g[:, 2]).all(), "static blocks come out gray"
    assert diff[spx & ~excused].max() <= 1
    # moving and partial edge blocks: the YCrCb round trip of the input, never quantised
    assert diff[~spx].max() <= 1
    if roundtrip_exact is None:
        roundtrip_exact = ycrcb2bgr(bgr2ycrcb(bgr))
    else:
        assert np.array_equal(got[~spx], roundtrip_exact[~spx])
    # the static blocks were quantised: they differ from the plain round trip
    assert np.abs(got[spx].astype(int) - roundtrip_exact[spx].astype(int)).max() > 8
