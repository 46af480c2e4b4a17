"""An independent numpy restatement of DESIGN.md "Quality metrics", "Kept and
static regions", written from its text: the class map by block reduction of the
mask, masked int64 sums, and a window's class from an all / any test over its 64
pixels (the package goes through 4x4 cells). The luma and the per-window formula
are tests/quality_ref.py's; nothing is shared with the package."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from tests import quality_ref as R

REGIONS = np.dtype([("sse", "<u8", (2, 4)), ("ssim_q32", "<i8", (3,)), ("windows", "<u4", (3,)),
                    ("pixels", "<u4", (2,)), ("reserved", "<u4")])


def class_map(mask, block, partial_static):
    """(H, W) bool, True where the pixel is static."""
    mask = np.asarray(mask)
    if mask.ndim != 2 or mask.dtype != np.uint8 or not 1 <= block <= 128 or partial_static not in (0, 1):
        raise ValueError("an (H, W) uint8 mask, block in 1..128, partial_static 0 or 1")
    H, W = mask.shape
    by, bx = -(-H // block), -(-W // block)
    padded = np.zeros((by * block, bx * block), bool)
    padded[:H, :W] = mask != 0                      # bytes outside the frame do not count
    static = ~padded.reshape(by, block, bx, block).any(axis=(1, 3))
    if not partial_static:                          # of:159: partial blocks are skipped, so kept
        if H % block:
            static[-1, :] = False
        if W % block:
            static[:, -1] = False
    return np.repeat(np.repeat(static, block, axis=0), block, axis=1)[:H, :W]


def window_q(a, b):
    """q of every 8x8 window at (4i, 4j), (H/4 - 1, W/4 - 1) int64 (quality_ref.frame's formula)."""
    ya, yb = R.luma(a), R.luma(b)
    s1, s2, ss, s12 = R._box8(ya), R._box8(yb), R._box8(ya * ya + yb * yb), R._box8(ya * yb)
    var, cov = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    A, B = 2 * s1 * s2 + 416, 2 * cov + 235963
    C, D = s1 * s1 + s2 * s2 + 416, var + 235963
    v = (A.astype(np.float64) * B.astype(np.float64)) / (C.astype(np.float64) * D.astype(np.float64))
    return np.rint(v * 4294967296.0).astype(np.int64)


def frame(a, b, mask, block, partial_static):
    """(sse[2][4], ssim_q32[3], windows[3], pixels[2]) of one frame pair under one mask."""
    a, b = np.asarray(a), np.asarray(b)
    H, W = a.shape[:2]
    if a.shape != b.shape or np.asarray(mask).shape != (H, W) or W < 8 or H < 8:
        raise ValueError("two BGR frames and a mask of one size, 8x8 at least")
    static = class_map(mask, block, partial_static)
    d = a.astype(np.int64) - b.astype(np.int64)
    err = np.concatenate([d * d, ((R.luma(a) - R.luma(b)) ** 2)[..., None]], axis=2)
    sse = [[int(err[sel][:, c].sum()) for c in range(4)] for sel in (~static, static)]
    q = window_q(a, b)
    win = sliding_window_view(static, (8, 8))[::4, ::4][:H // 4 - 1, :W // 4 - 1]
    all_static, any_static = win.all(axis=(2, 3)), win.any(axis=(2, 3))
    sel = (~any_static, all_static, any_static & ~all_static)          # kept, static, mixed
    return (sse, [int(q[s].sum()) for s in sel], [int(s.sum()) for s in sel],
            [int((~static).sum()), int(static.sum())])


def as_tuple(rec):
    """A dvc_quality_regions record as frame() writes it."""
    return ([[int(v) for v in row] for row in rec["sse"]], [int(v) for v in rec["ssim_q32"]],
            [int(v) for v in rec["windows"]], [int(v) for v in rec["pixels"]])


def records(ref, test, masks, block, partial_static):
    out = np.zeros(len(ref), REGIONS)
    for i, (a, b, m) in enumerate(zip(ref, test, masks)):
        sse, q, w, p = frame(a, b, m, block, partial_static)
        out[i] = (sse, q, w, p, 0)
    return out


def folded(rec):
    """The whole-frame seven integers a regions record adds up to (quality_ref.frame's form)."""
    sse, q, w, p = rec
    return [sse[0][i] + sse[1][i] for i in range(4)], sum(q), sum(w), sum(p)


class RefMeter(R.RefMeter):
    """quality_ref.RefMeter with the regions call."""

    def compare_regions(self, ref, test, mask, block, partial_static):
        assert len(ref) <= self.max_batch
        return records(ref, test, mask, block, partial_static)
