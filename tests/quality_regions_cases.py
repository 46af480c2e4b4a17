"""Shapes, block sizes, masks and contents shared by the region tests of the
quality meter (CPU and GPU), with the reference's records computed once per case
and left unchanged."""
import functools

import numpy as np

from tests import quality_cases as C
from tests import quality_regions_ref as RR

# (W, H), the smallest at which each index expression leaves its first trip: one
# window; remainders outside any window; two tiles each way with a 2-pixel
# remainder (halo cells and their classes cross tile edges); three tiles each way
SHAPES = [(8, 8), (11, 13), (130, 34), (264, 72)]
# 5 puts block edges inside cells; 128 is larger than a tile and partial at every shape
BLOCKS = [1, 4, 5, 8, 16, 128]
MASKS = ["zero", "full", "random", "corner"]
CONTENTS = ["noise", "identical", "black_white"]


@functools.lru_cache(maxsize=None)
def mask(kind, W, H, block):
    """One mask frame, read-only. "random": about half of the blocks hold non-zero
    bytes, a third of their bytes, of the values 1, 128 and 255."""
    m = np.zeros((H, W), np.uint8)
    if kind == "full":
        m[:] = 255
    elif kind == "corner":
        m[H - 1, W - 1] = 1
    elif kind == "random":
        rng = np.random.default_rng([W, H, block])
        by, bx = -(-H // block), -(-W // block)
        live = np.repeat(np.repeat(rng.random((by, bx)) < 0.5, block, axis=0), block, axis=1)[:H, :W]
        m[:] = np.where(live & (rng.random((H, W)) < 1 / 3), rng.choice(np.array([1, 128, 255], np.uint8), (H, W)), 0)
    elif kind != "zero":
        raise KeyError(kind)
    m.setflags(write=False)
    return m


def batch(W, H, block):
    """Every mask with every content: (ref, test, masks) stacks and their (mask, content) names."""
    names = [(k, c) for k in MASKS for c in CONTENTS]
    ref = np.stack([C.pair(c, W, H)[0] for _, c in names])
    test = np.stack([C.pair(c, W, H)[1] for _, c in names])
    masks = np.stack([mask(k, W, H, block) for k, _ in names])
    return ref, test, masks, names


@functools.lru_cache(maxsize=None)
def expected(kind, content, W, H, block, partial_static):
    """The reference's record of the case: (sse[2][4], ssim_q32[3], windows[3], pixels[2])."""
    return RR.frame(*C.pair(content, W, H), mask(kind, W, H, block), block, partial_static)
