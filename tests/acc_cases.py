"""Parameter points of the accumulated-mask recurrence (fd:107) shared by
test_acc.py (CPU) and test_acc_gpu.py: addWeighted weights (alpha, beta, gamma)
as float32, with what the library must decide for each of them —

* ``fast``: ``acc_fast_ok`` (csrc/fd_kernels.h) holds, k_acc<4 / 8> runs its
  short form (no clamp, the dilated addend a sign-mask AND);
* ``acc0_fixed``: addWeighted(acc 0, dilated 0) == 0, all-zero blocks stay zero.

Both columns are worked out by hand from IEEE-754 arithmetic (the comments say
how) and compared with what tools/acc_fast_host_check.cc prints.

Reference-style rows are (r, 1 - r, 0) as the reference derives them from
``release_factor`` (1 - r in double, then both to float32); raw rows are free
triples, which dvc_fd_params accepts as they are.
"""
from collections import namedtuple

import numpy as np

Row = namedtuple("Row", "name alpha beta gamma fast acc0_fixed")
f32 = np.float32


def _ref(name, r, fast, acc0_fixed):
    r = float(r)
    return Row(name, f32(r), f32(1 - r), f32(0.0), fast, acc0_fixed)


def _raw(name, a, b, g, fast, acc0_fixed):
    return Row(name, f32(a), f32(b), f32(g), fast, acc0_fixed)


BELOW_ONE = float(np.nextafter(f32(1.0), f32(0.0)))   # 1 - 2^-24: beta = 2^-24 exactly

ROWS = [
    # (r, 1 - r, 0) with 0 <= r <= 1: the addends are +0 and 255 (1 - r) >= 0, no clamp can bind
    _ref("r0", 0.0, True, True),            # no memory: acc = dilated
    _ref("r0p3", 0.3, True, True),          # fd:200-207's variant
    _ref("r0p5", 0.5, True, True),          # the default
    _ref("r0p51", 0.51, True, True),        # rint(0.51) = 1: a 1 never decays to 0
    _ref("r0p9", 0.9, True, True),
    _ref("r0p999", 0.999, True, True),
    _ref("r_below1", BELOW_ONE, True, True),
    _ref("r1", 1.0, True, True),            # acc never changes
    # alpha > 1: 255 * 1.25 clamps to 255; beta = -0.25, the dilated addend -63.75
    _ref("r1p25", 1.25, False, True),
    # alpha < 0, beta = 1.5: acc * -0.5 clamps to 0 and 382.5 to 255
    _ref("r_neg0p5", -0.5, False, True),
    # every sum is NaN -> 0; fmaf(0, NaN, .) is NaN too, so acc0_fixed cannot be claimed
    _ref("r_nan", float("nan"), False, False),
    # alpha = inf, beta = -inf: 0 * inf makes both addends and every sum NaN (or inf - inf)
    _ref("r_inf", float("inf"), False, False),
    # raw triples
    _raw("g0p4", 0.5, 0.5, 0.4, False, True),       # addend 0.4 is not +0, but rint(0.4) = 0
    _raw("g0p6", 0.5, 0.5, 0.6, False, False),      # rint(0.6) = 1: an all-zero block does not stay zero
    _raw("g_neg0p4", 0.5, 0.5, -0.4, False, True),  # rint(-0.4) = -0, saturates to 0
    # gamma = -0: fmaf(0, 0.5, -0) = (+0) + (-0) = +0 under round-to-nearest, so the
    # dilated-0 addend is +0 after all and the short form holds (same bytes as r0p5)
    _raw("g_negzero", 0.5, 0.5, -0.0, True, True),
    # the dilated-0 addend really is -0: fmaf(0, -0.5, -0) = (-0) + (-0); general form
    _raw("addend_negzero", 0.5, -0.5, -0.0, False, True),
    _raw("sum510", 1.0, 1.0, 0.0, False, True),     # 255 + 255: upper clamp
    _raw("g300", 1.0, 0.0, 300.0, False, False),    # upper clamp from gamma alone
    # undilated zeros become 1 and dilated pixels 0 (0.5 acc - 254.4 < 0): a partial edge block
    # that is dilated all over is static, whatever the kernel's padding of that block holds
    _raw("g0p6_bneg", 0.5, -1.0, 0.6, False, False),
]
BY_NAME = {r.name: r for r in ROWS}

# rows whose 33-frame decay is run on every geometry (test_acc_gpu.py)
DECAY = ("r0", "r0p3", "r0p51", "r1", "r1p25", "g0p6", "r_nan")
# rows that take the short form: compared with the general form under DVC_ACC_GENERAL=1
SHORT_VS_GENERAL = ("r0", "r0p3", "r0p5", "r0p9", "r1")


def weights(row):
    """(alpha, beta, gamma) as Python floats holding the float32 values exactly."""
    return float(row.alpha), float(row.beta), float(row.gamma)


# ------------------------------------------------------------- the clip ----
# (W, H, block size): the smallest frames at which each accumulate kernel's cases exist
GEOMS = [
    (264, 264, 4),    # k_acc<4>: full blocks, two 64-block words across
    (264, 264, 8),    # k_acc<8>
    (262, 258, 4),    # partial blocks right and below; every remainder even (no odd-DCT stop)
    (262, 258, 8),
    (262, 258, 6),    # k_acc_rows, W % 64 != 0 in the last word
    (264, 264, 16),   # k_acc_rows, blocks wider than a quad
]
# one geometry of each kernel for the batched modes
MODE_GEOMS = [(262, 258, 4), (262, 258, 8), (262, 258, 6)]
N_FRAMES = 34         # frame 0 primes; 1 seeded step; 2 the rectangles leave; 3..33 decay but for EVENTS
# frames after frame 2 with motion: a small rectangle appears (12, 27, 33) and leaves (13, 28). Every
# other frame from 3 on repeats its predecessor. Without them every dilated field after frame 2 is
# zero, and k_acc<B> masks the fields of idle frames (docc): what its load pipeline fetches for the
# second and third chunk of a launch would not matter, nor would the clamped tail's last frame.
EVENTS = (12, 13, 27, 28, 33)
# a threshold above the texture's own |blur5 - blur25| and far below the rectangles' contrast
WORKER_KW = dict(motion_threshold=24.5, kernel_size=7, min_area=500)


def clip(W, H):
    """(34, H, W, 3) uint8. Frame 0: a fixed low-contrast noise texture (the
    block DCTs have something to quantise, no motion of its own). Frame 1 adds
    bright rectangles far above min_area: one over every row of the left part
    (x + y takes all 256 residues inside it and, outside, in the untouched
    middle), which also touches the bottom edge, and one touching the right
    edge. Frame 2 removes them (motion in the same places once more) and brings
    a rectangle that stays (so that its dilated mask is not frame 1's). From
    frame 3 on the frames repeat, no motion, the accumulated mask only decays,
    but for three short events (EVENTS) in other block rows: a rectangle in
    frame 12 only, one in frame 27 only, one that appears in the last frame."""
    rng = np.random.default_rng(264 * W + H)
    tex = (112 + rng.integers(0, 17, (H, W, 3))).astype(np.uint8)
    frames = np.repeat(tex[None], N_FRAMES, axis=0)
    frames[1, :, 12:92] = (250, 240, 230)
    frames[1, 40:120, W - 40:] = (20, 250, 240)
    frames[2:, 60:100, 120:150] = (250, 245, 240)
    frames[12, 150:180, 120:160] = (10, 20, 30)
    frames[27, 20:50, 170:210] = (255, 255, 255)
    frames[33, 200:230, 130:170] = (15, 15, 15)
    return np.ascontiguousarray(frames)


def seed_plane(W, H):
    """seed[y, x] = (x + y) & 255: with the dilated plane of the seeded step, all 512 (acc, dilated) pairs."""
    y, x = np.mgrid[0:H, 0:W]
    return ((x + y) & 255).astype(np.uint8)


def worker_kwargs(row, block):
    return dict(WORKER_KW, block_size=block, accumulate=weights(row))


def static_blocks(acc, block):
    """Per block (partial edge blocks included): every accumulated byte is 0 (fd:120)."""
    H, W = acc.shape
    nby, nbx = -(-H // block), -(-W // block)
    pad = np.zeros((nby * block, nbx * block), np.uint8)
    pad[:H, :W] = acc
    return ~pad.reshape(nby, block, nbx, block).any(axis=(1, 3))


def oracle_run(oracle, W, H, block, row, n):
    """The oracle over frames 1..n of clip(W, H) from the seeded state: per
    frame (overlay, compressed, acc, dilated, cumulative stats)."""
    frames = clip(W, H)
    ref = oracle.OracleFD(W, H, **worker_kwargs(row, block))
    ref.prime(frames[0])
    ref.set_state(ref.plane(0), seed_plane(W, H))
    out = []
    for t in range(1, n + 1):
        ov, cp, acc = ref.step(frames[t])
        out.append((ov, cp, acc, ref.plane(4), ref.stats()))
    ref.close()
    return out
