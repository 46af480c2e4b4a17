"""Shapes and contents shared by the quality-meter tests (CPU and GPU), with the
reference's records computed once per case and left unchanged."""
import functools
import io

import numpy as np

from tests import quality_ref as R

TW, TH = 128, 32   # the kernel's tile (csrc/quality_kernels.h: kQualityTileW, kQualityTileH)

# (W, H): one window; remainders that the squared error counts and SSIM ignores, on rows
# that are not 4-byte aligned; one pixel, one cell and almost two cells past a tile,
# each way; more than two tiles each way; a total squared error past 2^32
SHAPES = ([(8, 8), (11, 13), (12, 9), (15, 15)]
          + [(TW + dx, TH + dy) for dx in (1, 4, 7) for dy in (1, 4, 7)]
          + [(2 * TW + 5, 2 * TH + 3), (264, 256)])
CONTENTS = ["identical", "black_white", "halves", "noise", "jpeg75"]


def jpeg_round_trip(frame, quality=75):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(buf, "JPEG", quality=quality)
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))[:, :, ::-1])


@functools.lru_cache(maxsize=None)
def pair(content, W, H):
    """(reference, test) frames of one case, read-only."""
    rng = np.random.default_rng([W, H, CONTENTS.index(content)])
    if content == "identical":
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        b = a.copy()
    elif content == "black_white":
        a, b = np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8)
    elif content == "halves":   # 8x8 blocks, left half 255, against the complement
        a = np.where((np.arange(W) % 8 < 4)[None, :, None], 255, 0).astype(np.uint8) * np.ones((H, 1, 3), np.uint8)
        b = 255 - a
    elif content == "noise":
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        b = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif content == "jpeg75":
        from dvc_amd.synthetic import clip
        a = clip(W, H, 1, seed=5)[0]
        b = jpeg_round_trip(a)
    else:
        raise KeyError(content)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def expected(content, W, H):
    """The reference's seven integers of the case: (sse[4], ssim_q32, windows, pixels)."""
    return R.frame(*pair(content, W, H))


def as_tuple(rec):
    """A dvc_quality_frame record as expected() writes it."""
    return [int(v) for v in rec["sse"]], int(rec["ssim_q32"]), int(rec["windows"]), int(rec["pixels"])
