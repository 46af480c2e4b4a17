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


# ---- kept and static regions (DESIGN.md "Quality metrics", "Regions") -------------------

def _psnr_or_nan(sse, count) -> float:
    return psnr(sse, count) if count else math.nan


def _ratio_or_nan(num, den) -> float:
    return num / den if den else math.nan


def _region_figures(sse, pixels) -> dict:
    """PSNRs of the kept and static pixels from sse[class][channel] and pixels[class] (ints)."""
    out = {}
    for c, name in enumerate(("kept", "static")):
        out["psnr_y_" + name] = _psnr_or_nan(sse[c][3], pixels[c])
        out["psnr_bgr_" + name] = _psnr_or_nan(sse[c][0] + sse[c][1] + sse[c][2], 3 * pixels[c])
    out["static_pixel_share"] = _ratio_or_nan(pixels[1], pixels[0] + pixels[1])
    return out


def region_metrics(rec) -> dict:
    """One ``dvc_quality_regions`` record -> PSNR (dB) of its kept and static
    pixels, SSIM of its kept, static and mixed windows and the share of static
    pixels; ``nan`` for a class without a pixel or a window."""
    sse = [[int(v) for v in row] for row in rec["sse"]]
    out = _region_figures(sse, [int(v) for v in rec["pixels"]])
    for k, name in enumerate(("kept", "static", "mixed")):
        out["ssim_y_" + name] = _ratio_or_nan(int(rec["ssim_q32"][k]), int(rec["windows"][k]) * 2.0 ** 32)
    return out


def summarize_regions(records) -> dict:
    """A video's figures per class from its ``dvc_quality_regions`` records: PSNR
    pools the squared error and the pixels of a class over the frames; SSIM of a
    class is the mean over the frames that have such windows; with the share of
    static pixels and the window counts. ``nan`` where a class never occurs."""
    sse = [[sum(int(r["sse"][c][i]) for r in records) for i in range(4)] for c in range(2)]
    pixels = [sum(int(r["pixels"][c]) for r in records) for c in range(2)]
    out = dict(_region_figures(sse, pixels), frames=len(records))
    for k, name in enumerate(("kept", "static", "mixed")):
        per = [int(r["ssim_q32"][k]) / (int(r["windows"][k]) * 2.0 ** 32) for r in records if int(r["windows"][k])]
        out["ssim_y_" + name] = _ratio_or_nan(math.fsum(per), len(per))
        out[name + "_windows"] = sum(int(r["windows"][k]) for r in records)
    return out


def mask_gray(frame):
    """A decoded mask frame as one byte a pixel: a 3-channel frame becomes the
    project's gray (of:148-149, OpenCV BGR2GRAY 8U)."""
    m = np.asarray(frame)
    if m.ndim == 3:
        p = m.astype(np.uint32)
        m = ((1868 * p[..., 0] + 9617 * p[..., 1] + 4899 * p[..., 2] + 8192) >> 14).astype(np.uint8)
    return m


def _mask_frames(masks):
    """(iterator over mask frames, what to release afterwards) of a path or an iterable."""
    if not isinstance(masks, (str, os.PathLike)):
        return iter(masks), None
    cap = video_io.open_source(os.fspath(masks))
    if not cap.isOpened():
        raise ValueError(f"unable to open {masks}")

    def frames():
        while True:
            ok, m = cap.read()
            if not ok:
                return
            yield m
    return frames(), cap


def compare_videos_regions(ref_path, test_path, masks, block, partial_static, ref_skip=0, meter=None):
    """:func:`compare_videos` split into the kept and the static region: ``test_path``
    frame k against ``ref_path`` frame k + ``ref_skip`` under mask frame k, until
    any of the three ends. ``masks``: a video opened through
    ``video_io.open_source`` (the OF driver's ``mask.mp4``) or an iterable of
    H x W uint8 arrays (:func:`fd_static_masks`); 3-channel mask frames are grayed
    (:func:`mask_gray`). ``block``, ``partial_static``: the block rule of
    ``dvc_quality_compare_regions`` — 8 and 0 for the OF driver, ``block_size``
    and 1 for the FD driver. Returns ``(records, summary)``: the
    ``dvc_quality_regions`` record of every pair and :func:`summarize_regions` of
    them (plus ``width`` and ``height``). ``meter``: as in :func:`compare_videos`,
    with ``compare_regions``. Frames or masks of another size raise ``ValueError``."""
    from ._native import QUALITY_REGIONS
    ref, test = video_io.open_source(ref_path), video_io.open_source(test_path)
    own = mcap = None
    try:
        if not ref.isOpened() or not test.isOpened():
            raise ValueError(f"unable to open {ref_path if not ref.isOpened() else test_path}")
        (W, H), ts = _size(ref), _size(test)
        if (W, H) != ts:
            raise ValueError(f"frame sizes differ: {ref_path} is {W}x{H}, {test_path} is {ts[0]}x{ts[1]}")
        mit, mcap = _mask_frames(masks)
        for _ in range(int(ref_skip)):
            if not ref.read()[0]:
                break
        if meter is None:
            from . import _native as N
            dev = int(os.environ.get("DVC_DEVICE", os.environ.get("LOCAL_RANK", 0)))
            meter = own = N.QualityMeter(W, H, device=dev, max_batch=8)
            bufs = [N.pinned((meter.max_batch, H, W, 3)) for _ in range(2)] + [N.pinned((meter.max_batch, H, W))]
        else:
            bufs = [np.empty((meter.max_batch, H, W, 3), np.uint8) for _ in range(2)] + \
                [np.empty((meter.max_batch, H, W), np.uint8)]
        chunks, more = [], True
        while more:
            n = 0
            while n < meter.max_batch:
                m = next(mit, None)
                if m is None:
                    more = False
                    break
                (ok_a, a), (ok_b, b) = ref.read(), test.read()
                if not (ok_a and ok_b):
                    more = False
                    break
                m = mask_gray(m)
                if a.shape != (H, W, 3) or b.shape != (H, W, 3):
                    raise ValueError(f"frames {a.shape} against {b.shape}: two BGR frames of {W}x{H} are needed")
                if m.shape != (H, W) or m.dtype != np.uint8:
                    raise ValueError(f"frame sizes differ: mask frame {m.shape} {m.dtype} against {W}x{H} frames")
                bufs[0][n], bufs[1][n], bufs[2][n] = a, b, m
                n += 1
            if n:
                chunks.append(np.array(meter.compare_regions(bufs[0][:n], bufs[1][:n], bufs[2][:n], block,
                                                             partial_static)))
        records = np.concatenate(chunks) if chunks else np.zeros(0, QUALITY_REGIONS)
        return records, dict(summarize_regions(records), width=W, height=H)
    finally:
        ref.release()
        test.release()
        if mcap is not None:
            mcap.release()
        if own is not None:
            own.close()


def fd_static_masks(source_path, block_size=4, search_area=16, motion_threshold=0.5, min_area=500, kernel_size=7,
                    release_factor=0.5, quantization_level=100, scale_factor=1.0, device=None):
    """The accumulated masks the FD driver decided on (fd:107, tested at fd:120),
    one H x W uint8 array per output frame: the source replayed through an
    :class:`fd.FDWorker` one frame a step, with the parameter names and defaults
    of ``frame_differencing.filter_and_dilate_movements``, ``DVC_PLANE_ACC`` after
    each step. The driver writes no mask video of its own (its
    ``dilated_motion_mask_video`` is an overlay). Only ``scale_factor`` 1 is
    supported: :func:`compare_videos` cannot pair resized outputs either."""
    if scale_factor != 1:
        raise ValueError(f"scale_factor {scale_factor}: only 1 is supported")
    from . import _native as N
    from .fd import FDWorker
    cap = video_io.open_source(source_path)
    if not cap.isOpened():
        raise ValueError(f"unable to open {source_path}")
    worker = None
    try:
        yuv = getattr(cap, "pixel_format", "BGR") != "BGR"
        read = cap.read_yuv if yuv else cap.read
        ok, first = read()
        if not ok:
            return
        W, H = _size(cap)
        if device is None:
            device = int(os.environ.get("DVC_DEVICE", os.environ.get("LOCAL_RANK", 0)))
        worker = FDWorker(W, H, device=device, block_size=block_size, motion_threshold=motion_threshold,
                          min_area=min_area, kernel_size=kernel_size, release_factor=release_factor,
                          quantization_level=quantization_level, in_format=cap.pixel_format if yuv else "BGR")
        worker.prime(first)
        while True:
            ok, frame = read()
            if not ok:
                return
            worker.step(frame)
            yield worker.plane(N.PLANE_ACC)
    finally:
        cap.release()
        if worker is not None:
            worker.close()
