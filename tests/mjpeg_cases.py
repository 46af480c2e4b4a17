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


def _hd(seed):
    """1920x1080: a synthetic surveillance frame, its right third replaced by noise
    (long segments, 0xFF bytes to stuff)."""
    from dvc_amd.synthetic import SyntheticClip
    f = SyntheticClip(1920, 1080, seed=seed).frame(3).copy()
    f[:, 1280:] = _noise(640, 1080, 20 + seed)
    return f


# The sizes at which the encoder's loops take a later trip (tests/test_mjpeg_sizes.py asserts
# each property from the reference's own output; tests/test_mjpeg_sizes_gpu.py runs the kernels).
# Kept out of ALL: the parametrised tests above do not grow.
SIZE_CASES = {
    "tall8x2056_gray": (lambda: _smooth_noise(8, 2056, 21), 75),       # one component: 257 segments
    "tall16x4112": (lambda: _smooth_noise(16, 4112, 22), 75),          # colour: 257 segments
    "dense176x16_q100": (lambda: _noise(176, 16, 23), 100),            # 66 blocks a segment at Q = 1
    "dense520x8_q100_gray": (lambda: _noise(520, 8, 24), 100),         # one component: 65 blocks
}
SIZE_GRAY = {"tall8x2056_gray": True, "tall16x4112": False, "dense176x16_q100": False, "dense520x8_q100_gray": True}
# two different frames (variants 0 and 1); too large for a whole-frame reference: segment_reference
HD_CASE = "hd1920x1080"
HD_CASES = {HD_CASE: ((lambda: _hd(5), lambda: _hd(6)), 75)}
_EVERY = {**ALL, **SIZE_CASES}


def quality(name):
    return HD_CASES[name][1] if name in HD_CASES else _EVERY[name][1]


@functools.lru_cache(maxsize=None)
def frame(name, variant=0):
    """variant 1: the frame turned by 180 degrees (a second, different frame of a batch);
    of HD_CASES: the second frame."""
    if name in HD_CASES:
        f = HD_CASES[name][0][variant]()
    else:
        f = _EVERY[name][0]()
        f = f[::-1, ::-1] if variant else f
    f = np.ascontiguousarray(f)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(name, variant=0, gray=False):
    assert name not in HD_CASES, "too slow as a whole frame: segment_reference"
    f = frame(name, variant)
    return mjpeg_ref.encode(f[..., 1] if gray else f, _EVERY[name][1])


@functools.lru_cache(maxsize=None)
def _strip_reference(name, variant, i, gray):
    f = frame(name, variant)
    m = 8 if gray else 16
    assert 0 <= i * m < f.shape[0]
    strip = f[i * m:i * m + m]
    return mjpeg_ref.encode(strip[..., 1] if gray else strip, quality(name))


def segment_reference(name, variant, i, gray=False):
    """Restart segment i of a frame (its entropy bytes, without the RST marker or EOI
    behind them), from the reference encoder run on MCU row i alone. Segments are
    independent: the DC predictors restart, chroma is subsampled inside the MCU, a
    full strip needs no edge replication, and a partial last strip is replicated
    downwards exactly as the whole frame's bottom is."""
    s = _strip_reference(name, variant, i, gray)["stream"]
    assert s[-2:] == b"\xff\xd9"
    return s[:-2]


def segment_stuffed(name, variant, i, gray=False):
    """How many 0xFF bytes of segment i the reference stuffed."""
    return _strip_reference(name, variant, i, gray)["stuffed"]


def split_stream(stream):
    """Entropy data -> ([segment bytes], [the marker byte behind each]). In entropy data
    0xFF is followed by 0x00 or by a marker's second byte."""
    b = np.frombuffer(stream, np.uint8)
    segs, marks, a = [], [], 0
    for i in np.nonzero((b[:-1] == 0xFF) & (b[1:] != 0))[0].tolist():
        segs.append(stream[a:i])
        marks.append(stream[i + 1])
        a = i + 2
    assert a == len(stream), "the stream ends with a marker"
    return segs, marks


@functools.lru_cache(maxsize=None)
def block_bit_offsets(name, variant=0, gray=False, seg=0):
    """(bit offset of every block of restart segment `seg` in scan order, the segment's bits),
    by the reference's own block coder on the reference's levels."""
    ref = reference(name, variant, gray)
    info, lv = ref["info"], ref["levels"]
    tabs = {cid: (info["huff"][(0, td)], info["huff"][(1, ta)]) for cid, td, ta in info["scan"]}
    tabs = [tabs[c[0]] for c in info["comps"]]
    bits, pred, off = mjpeg_ref._Bits(), [0, 0, 0], []
    for mx in range(info["dri"]):
        order = [(0, seg, mx)] if gray else [(0, 2 * seg + dy, 2 * mx + dx) for dy in (0, 1) for dx in (0, 1)] + \
            [(1, seg, mx), (2, seg, mx)]
        for c, by, bx in order:
            off.append(bits.n)
            pred[c] = mjpeg_ref._code_block(bits, lv[c][by, bx], pred[c], *tabs[c])
    return off, bits.n
