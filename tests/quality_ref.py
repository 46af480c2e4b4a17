"""An independent numpy restatement of DESIGN.md "Quality metrics", written from
its text: int64 sums, float64 A B / (C D), np.rint. It shares no code with the
package; the tests compare the GPU meter and the sanitized host program with it
integer for integer."""
import numpy as np

FRAME = np.dtype([("sse", "<u8", (4,)), ("ssim_q32", "<i8"), ("windows", "<u4"), ("pixels", "<u4")])


def luma(bgr):
    """OpenCV BGR2GRAY 8U of an (..., 3) uint8 array, as int64."""
    p = bgr.astype(np.int64)
    return (1868 * p[..., 0] + 9617 * p[..., 1] + 4899 * p[..., 2] + 8192) >> 14


def _box8(x):
    """Sums of x over the 8x8 windows at every (4i, 4j): cells of 4x4, then 2x2 cells."""
    H, W = x.shape
    ch, cw = H // 4, W // 4
    cells = x[:ch * 4, :cw * 4].reshape(ch, 4, cw, 4).sum(axis=(1, 3))
    return cells[:-1, :-1] + cells[:-1, 1:] + cells[1:, :-1] + cells[1:, 1:]


def frame(a, b):
    """The seven integers of one frame pair: (sse[4], ssim_q32, windows, pixels)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("two BGR uint8 frames of one size")
    H, W = a.shape[:2]
    if W < 8 or H < 8:
        raise ValueError("a frame below 8x8 has no window")
    d = a.astype(np.int64) - b.astype(np.int64)
    ya, yb = luma(a), luma(b)
    sse = [int((d[..., c] ** 2).sum()) for c in range(3)] + [int(((ya - yb) ** 2).sum())]
    s1, s2, ss, s12 = _box8(ya), _box8(yb), _box8(ya * ya + yb * yb), _box8(ya * yb)
    var, cov = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    A, B = 2 * s1 * s2 + 416, 2 * cov + 235963
    C, D = s1 * s1 + s2 * s2 + 416, var + 235963
    for t in (A, B, C, D):
        assert np.abs(t).max() < 2 ** 31
    v = (A.astype(np.float64) * B.astype(np.float64)) / (C.astype(np.float64) * D.astype(np.float64))
    q = np.rint(v * 4294967296.0).astype(np.int64)
    return sse, int(q.sum()), (W // 4 - 1) * (H // 4 - 1), W * H


def records(ref, test):
    """frame() over two stacks of frames, as a FRAME record array."""
    out = np.zeros(len(ref), FRAME)
    for i, (a, b) in enumerate(zip(ref, test)):
        sse, q, w, p = frame(a, b)
        out[i] = (sse, q, w, p)
    return out


class RefMeter:
    """What _native.QualityMeter is to quality.compare_videos, on the CPU."""

    def __init__(self, max_batch=8):
        self.max_batch = max_batch

    def compare(self, ref, test):
        return records(ref, test)

    def close(self):
        pass


def psnr(sse, count):
    return float("inf") if sse == 0 else 10.0 * np.log10(255.0 ** 2 * count / sse)
