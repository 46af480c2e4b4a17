"""The Motion-JPEG test frames shared by tests/test_mjpeg.py (an independent
decoder on the reference stream) and tests/test_mjpeg_gpu.py (the GPU encoder
byte for byte against the reference stream). Each reference is computed once."""
import functools

import numpy as np

from tests import mjpeg_ref


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _zz63():
    """Four luma blocks 128 + 100 * the (7,7) DCT basis, gray pixels (Cb = Cr = 128):
    F(7,7) = 4 * 100, quality 50's Q(7,7) = 99 gives level 4; pixel rounding moves
    every other coefficient by < 3.3, below half of quality 50's smallest Q (10)."""
    c7 = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    blk = np.rint(128 + 100 * np.outer(c7, c7)).astype(np.uint8)
    return np.repeat(np.tile(blk, (2, 2))[:, :, None], 3, 2)


def _alt8():
    """8x8 blocks alternating 0 / 255 (gray pixels): at quality 100 consecutive luma
    DC levels are -1024 and +1016, a difference of 2040 = DC size 11."""
    by, bx = np.indices((2, 4))
    return np.repeat(np.kron(((by + bx) % 2) * 255, np.ones((8, 8), np.int64)).astype(np.uint8)[:, :, None], 3, 2)


def _mixed():
    """130x50: a synthetic surveillance frame, its right third replaced by noise."""
    from dvc_amd.synthetic import SyntheticClip
    f = SyntheticClip(130, 50, seed=5).frame(2).copy()
    f[:, 90:] = _noise(40, 50, 11)
    return f


def _smooth_noise(w, h, seed):
    y, x = np.indices((h, w))
    base = (96 + 60 * np.sin(x / 7.0) + 50 * np.cos(y / 11.0))[:, :, None]
    return np.clip(base + np.random.default_rng(seed).integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


# name -> (frame builder, quality); the issue's table, row by row
CASES = {
    "const16": (lambda: np.full((16, 16, 3), (90, 120, 200), np.uint8), 75),      # EOB-only blocks
    "noise33x17_q90": (lambda: _noise(33, 17, 1), 90),                            # edge replication, odd chroma
    "noise33x17_q50": (lambda: _noise(33, 17, 1), 50),
    "noise70x37_q90": (lambda: _noise(70, 37, 2), 90),
    "noise70x37_q50": (lambda: _noise(70, 37, 2), 50),
    "noise16_q100": (lambda: _noise(16, 16, 3), 100),                             # Q = 1, longest codes, clamps
    "zz63": (_zz63, 50),                                                          # three ZRLs
    "alt8": (_alt8, 100),                                                         # DC size 11
    "rst_wrap32x160": (lambda: _smooth_noise(32, 160, 4), 75),                    # 10 segments: RST index wraps
    "wide1120x32": (lambda: _noise(1120, 32, 6), 90),                             # 420 blocks a segment
    "mixed130x50_q20": (_mixed, 20),
}
# frames smaller than one MCU (beyond the issue's table): every sample but a few is edge replication
EXTRA = {
    "tiny1x1": (lambda: np.array([[[10, 200, 90]]], np.uint8), 75),
    "tiny5x3": (lambda: _noise(5, 3, 8), 90),
}
ALL = {**CASES, **EXTRA}
GRAY_CASE = "noise70x37_q90"


@functools.lru_cache(maxsize=None)
def frame(name, variant=0):
    """variant 1: the frame turned by 180 degrees (a second, different frame of a batch)."""
    f = ALL[name][0]()
    f = f[::-1, ::-1] if variant else f
    f = np.ascontiguousarray(f)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(name, variant=0, gray=False):
    f = frame(name, variant)
    return mjpeg_ref.encode(f[..., 1] if gray else f, ALL[name][1])
