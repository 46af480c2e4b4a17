"""Picture quality of a compressed output against its source: per-frame squared
error and integer SSIM from the GPU meter (``_native.QualityMeter``,
``dvc_quality_compare``), PSNR and SSIM derived from them here in float64 —
DESIGN.md "Quality metrics" is the definition.

The reference reports what compression saves (``performance_analysis.py``:
``reduction_percentage``) and nothing about what it costs; this is the other
half of that rate-distortion point.

Alignment. The drivers do not write an output for the frame they prime on:
the FD driver reads frame 0, primes, and writes outputs for frames 1..
(``frame_differencing.py``: ``worker.prime(first)``, then the chunk loop), so
``compressed_final_video`` frame k is source frame k + 1; the OF driver's first
pass does the same with ``overlay.mp4`` (``temporal_smoothing_flow``:
``worker.prime(first_frame)``, then ``out_overlay.write(pipe.ins[i][t])``) and
its second pass pairs ``overlay.mp4`` and ``mask.mp4`` from their first frames
(``compress_with_motion``: ``read_pair`` hands back the pair read before the
loop first), so ``compressed`` frame k is overlay frame k, source frame k + 1.
``DRIVER_REF_SKIP`` = 1 is that offset for both.
"""
from __future__ import annotations

import math
import os

import numpy as np

from . import video_io
from ._native import QUALITY_FRAME

DRIVER_REF_SKIP = 1   # source frames in front of the first output frame (FD and OF drivers alike)


def psnr(sse, count) -> float:
    """10 log10(255^2 count / sse) in float64; inf for identical pictures."""
    sse, count = int(sse), int(count)
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 * count / sse)


def frame_metrics(rec) -> dict:
    """One ``dvc_quality_frame`` record -> its PSNRs (dB) and SSIM."""
    px = int(rec["pixels"])
    return {"psnr_y": psnr(rec["sse"][3], px),
            "psnr_bgr": psnr(int(rec["sse"][0]) + int(rec["sse"][1]) + int(rec["sse"][2]), 3 * px),
            "ssim_y": int(rec["ssim_q32"]) / (int(rec["windows"]) * 2.0 ** 32)}


def summarize(records) -> dict:
    """A video's figures from its frame records: PSNR pools the squared error
    over the frames, SSIM is the mean over the frames; both with the worst frame."""
    n = len(records)
    if n == 0:
        return {"frames": 0, "psnr_y": math.nan, "psnr_y_min": math.nan, "psnr_bgr": math.nan, "psnr_bgr_min": math.nan,
                "ssim_y": math.nan, "ssim_y_min": math.nan}
    per = [frame_metrics(r) for r in records]
    px = sum(int(r["pixels"]) for r in records)
    sse = [sum(int(r["sse"][c]) for r in records) for c in range(4)]
    return {"frames": n,
            "psnr_y": psnr(sse[3], px), "psnr_y_min": min(m["psnr_y"] for m in per),
            "psnr_bgr": psnr(sse[0] + sse[1] + sse[2], 3 * px), "psnr_bgr_min": min(m["psnr_bgr"] for m in per),
            "ssim_y": math.fsum(m["ssim_y"] for m in per) / n, "ssim_y_min": min(m["ssim_y"] for m in per)}


def _size(cap):
    return int(cap.get(video_io.CAP_PROP_FRAME_WIDTH)), int(cap.get(video_io.CAP_PROP_FRAME_HEIGHT))


def compare_videos(ref_path, test_path, ref_skip=0, meter=None):
    """Compare ``test_path`` frame k with ``ref_path`` frame k + ``ref_skip``,
    both opened through ``video_io.open_source``, in chunks of the meter's
    ``max_batch`` until either ends. Returns ``(records, summary)``: the
    ``dvc_quality_frame`` record of every pair and :func:`summarize` of them
    (plus ``width`` and ``height``). ``meter``: the object that compares, with
    ``max_batch``, ``compare(ref, test)`` and ``close()`` (default: a
    :class:`_native.QualityMeter` on ``DVC_DEVICE``, closed on return). Frames of
    different sizes, or frames that are not BGR, raise ``ValueError``."""
    ref, test = video_io.open_source(ref_path), video_io.open_source(test_path)
    own = None
    try:
        if not ref.isOpened() or not test.isOpened():
            raise ValueError(f"unable to open {ref_path if not ref.isOpened() else test_path}")
        (W, H), ts = _size(ref), _size(test)
        if (W, H) != ts:
            raise ValueError(f"frame sizes differ: {ref_path} is {W}x{H}, {test_path} is {ts[0]}x{ts[1]}")
        for _ in range(int(ref_skip)):
            if not ref.read()[0]:
                break
        if meter is None:
            from . import _native as N
            dev = int(os.environ.get("DVC_DEVICE", os.environ.get("LOCAL_RANK", 0)))
            meter = own = N.QualityMeter(W, H, device=dev, max_batch=8)
            bufs = [N.pinned((meter.max_batch, H, W, 3)) for _ in range(2)]
        else:
            bufs = [np.empty((meter.max_batch, H, W, 3), np.uint8) for _ in range(2)]
        chunks, more = [], True
        while more:
            n = 0
            while n < meter.max_batch:
                (ok_a, a), (ok_b, b) = ref.read(), test.read()
                if not (ok_a and ok_b):
                    more = False
                    break
                if a.shape != (H, W, 3) or b.shape != (H, W, 3):
                    raise ValueError(f"frames {a.shape} against {b.shape}: two BGR frames of {W}x{H} are needed")
                bufs[0][n], bufs[1][n] = a, b
                n += 1
            if n:
                chunks.append(np.array(meter.compare(bufs[0][:n], bufs[1][:n])))
        records = np.concatenate(chunks) if chunks else np.zeros(0, QUALITY_FRAME)
        return records, dict(summarize(records), width=W, height=H)
    finally:
        ref.release()
        test.release()
        if own is not None:
            own.close()
