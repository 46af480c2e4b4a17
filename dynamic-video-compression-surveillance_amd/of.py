"""One camera feed on one GPU: the per-frame worker of the optical-flow path.

``OFWorker`` owns a ``dvc_of`` handle (include/dvc.h) and replaces the bodies
of the two reference loops of ``motion_compression_opt.py`` fused per frame:
``temporal_smoothing_flow`` (``of:65-101``: gray, Farneback, |flow| > thr, the
30-frame vote, close/open, rectangles) and ``compress_with_motion``
(``of:141-185``: static 8x8 blocks DCT-quantised on Y, Cr, Cb, then grey).
``prime`` is the first-frame setup (``of:54-62``), ``step`` one frame.

Frames are H x W x 3 uint8 BGR: numpy arrays in host mode; device buffers
(torch tensors or raw addresses) with ``device_ptrs=True`` (asynchronous).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from ._worker import Worker


def derive_of_params(width: int, height: int, flow_threshold: float = 0.5, alpha_fraction: float = 0.2,
                     window_size: int = 30, morph_kernel: int = 2, quantization_level: float = 100.0,
                     flags: int = 0, direct_sums: bool = False, in_format: str = "BGR",
                     chroma_rows: int = 0, pyr_scale: float = 0.3, levels: int = 2, winsize: int = 9,
                     iterations: int = 2, poly_n: int = 5, poly_sigma: float = 1.1) -> N.OfParams:
    """dvc_of_params from the reference kwargs of ``temporal_smoothing_flow``
    (of:29-31) and the arguments it hard-codes: Farneback (0.3, 2, 9, 2, 5, 1.1,
    0) at of:72-81, ``QTY_aggressive`` = 100 at of:138. ``direct_sums``: direct
    per-pixel box sums instead of OpenCV's running sums (the default).
    ``pyr_scale`` ... ``poly_sigma``: the calcOpticalFlowFarneback arguments, for
    callers other than the reference (dvc_of_create states the accepted range)."""
    p = N.OfParams()
    if direct_sums:
        flags |= N.DVC_FLAG_OF_DIRECT_SUMS
    p.width, p.height = int(width), int(height)
    p.flow_threshold = float(flow_threshold)
    p.quant = float(quantization_level)
    p.alpha_fraction = float(alpha_fraction)
    p.window = int(window_size)
    p.morph_kernel = int(morph_kernel)
    p.pyr_scale, p.levels, p.winsize = float(pyr_scale), int(levels), int(winsize)
    p.iterations, p.poly_n, p.poly_sigma = int(iterations), int(poly_n), float(poly_sigma)
    p.flags = flags
    p.in_format = N.FORMATS[in_format]
    p.chroma_rows = int(chroma_rows)
    return p


class OFWorker(Worker):
    _abi, _destroy = "dvc_of", "dvc_of_destroy"
    _outs = ("mask", "compressed")

    def __init__(self, width: int, height: int, *, device: int = 0, stream=None, device_ptrs: bool = False,
                 keep_planes: bool = False, ktiming: bool = False, max_batch: int = 1, out_format: str = "BGR",
                 **kwargs):
        """``out_format`` "BGR" or "I420": compressed frames as packed BGR, or
        as the encoder's 4:2:0 input, (H*3/2, W) (DVC_FLAG_OUT_I420; W and H
        even). The mask is the encoder's mono frame either way."""
        if out_format not in ("BGR", "I420"):
            raise ValueError(f"out_format {out_format!r}: BGR or I420")
        self.out_format = out_format
        W, H = int(width), int(height)
        self._oshape = (H, W, 3) if out_format == "BGR" else (H * 3 // 2, W)
        self._astride = (W * H,)   # dvc_of_step_batch: mask_stride
        flags = N.DVC_FLAG_OUT_I420 if out_format == "I420" else 0
        self._open(derive_of_params(width, height, flags=flags, **kwargs), kwargs.get("in_format", "BGR"), (W, H),
                   ((H, W), self._oshape), device=device, stream=stream, device_ptrs=device_ptrs,
                   keep_planes=keep_planes, ktiming=ktiming, max_batch=max_batch)

    def set_state(self, prev_gray, raw_masks) -> None:
        """Resume instead of :meth:`prime` (dvc_of_set_state): the previous gray
        (H x W, of:101) and the raw |flow| masks of the last frames, oldest
        first ((n, H, W), of:84) — :meth:`plane` with OF_PLANE_GRAY / _RAW
        exports them."""
        g = np.ascontiguousarray(prev_gray, dtype=np.uint8)
        m = np.ascontiguousarray(raw_masks, dtype=np.uint8)
        if m.ndim == 2:
            m = m[None]
        if g.shape != (self.H, self.W) or m.shape[1:] != (self.H, self.W):
            raise ValueError(f"state planes must be ({self.H}, {self.W})")
        N.check(self._lib.dvc_of_set_state(self._h, g.ctypes.data, m.ctypes.data if len(m) else None, len(m)))

    def step(self, frame, mask=None, compressed=None, want=("mask", "compressed")):
        """of:70-101 + of:151-183 for one frame. Host mode returns ``(mask,
        compressed)`` (H x W {0,255} and H x W x 3, or the (H*3/2, W) I420
        frame with ``out_format="I420"``); device mode writes into the
        given buffers and returns None."""
        return self._step(frame, mask, compressed, want)

    def step_batch(self, frames, mask=None, compressed=None, want=("mask", "compressed")):
        """n consecutive frames (identical to n :meth:`step` calls). Host mode:
        (n, H, W, 3) uint8 in, ``(masks, compressed)`` out. Device mode: CUDA
        tensors on the handle's device or explicit ``(address, n)`` tuples;
        asynchronous, returns None."""
        return self._step_batch(frames, mask, compressed, want)

    def flow(self) -> np.ndarray:
        """Farneback flow (H x W x 2 float32) of the last frame (needs keep_planes)."""
        out = np.empty((self.H, self.W, 2), np.float32)
        N.check(self._lib.dvc_of_read_flow(self._h, out.ctypes.data))
        return out

    def debug_read(self, what: int, level: int = 0) -> np.ndarray:
        """Farneback intermediates of the last frame at a pyramid level: 0 its
        polynomial expansion R (h, w, 5), 1 the previous frame's R, 2 the flow
        after the first iteration (h, w, 2) — kept only while no later
        iteration has reused its buffer (dvc_of_debug_read in include/dvc.h);
        DvcError (DVC_E_STATE) otherwise."""
        w, h = ctypes.c_int(), ctypes.c_int()
        N.check(self._lib.dvc_of_debug_read(self._h, what, level, None, ctypes.byref(w), ctypes.byref(h)))
        out = np.empty((h.value, w.value, 5 if what in (0, 1) else 2), np.float32)
        N.check(self._lib.dvc_of_debug_read(self._h, what, level, out.ctypes.data, None, None))
        return out

    def ktime_kernel(self) -> str:
        """The kernel that ran the level-0 iterations of the last batch (what
        :meth:`ktime` timed): "k_flow" (direct sums), "k_flow_scan" (the
        barrier-phased running-sum scan) or "k_flow_scan2" (the pipelined scan)."""
        if not hasattr(self._lib, "dvc_of_ktime_kernel"):   # an older build (DVC_LIB_PATH A/B)
            return "k_flow_scan2"
        k = self._lib.dvc_of_ktime_kernel(self._h)
        if k < 0:
            N.check(k)
        return {N.KTIME_FLOW: "k_flow", N.KTIME_FLOW_SCAN: "k_flow_scan", N.KTIME_FLOW_SCAN2: "k_flow_scan2"}[k]
