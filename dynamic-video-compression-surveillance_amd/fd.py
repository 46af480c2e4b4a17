"""One camera feed on one GPU: the per-frame worker of the FD path.

``FDWorker`` owns a ``dvc_fd`` handle (include/dvc.h) and replaces the body of
the reference loop ``frame_differencing.py:85-138``: ``prime`` is the frame-0
preprocessing (``fd:67-81``), ``step`` one iteration (``fd:91-133``).

Frames are H x W x 3 uint8 BGR. In host mode they are numpy arrays; in device
mode (``device_ptrs=True``) they are device buffers — torch tensors on the
handle's device, or raw integer addresses — and ``step`` is asynchronous.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _buffers as B
from . import _native as N
from ._worker import Worker


def derive_params(width: int, height: int, block_size: int = 4, motion_threshold: float = 0.5,
                  min_area: float = 500, kernel_size: int = 7, release_factor: float = 0.5,
                  quantization_level: float = 100, flags: int = 0, src_width: int = 0,
                  src_height: int = 0, in_format: str = "BGR", chroma_rows: int = 0,
                  accumulate=None) -> N.FdParams:
    """dvc_fd_params from the reference kwargs (frame_differencing.py:21-30).

    * ``ithresh = floor(motion_threshold)`` clamped to [-1, 255]: cv::threshold
      floors the threshold for 8U input (fd:97).
    * ``min_area2 = floor(2*min_area)``: ``contourArea > min_area`` is exactly
      ``2*area > floor(2*min_area)`` for the half-integer polygon areas (fd:103).
    * addWeighted receives (release_factor, 1 - release_factor, 0) as doubles and
      computes in float32 (fd:107). ``accumulate=(alpha, beta, gamma)`` hands
      over raw weights instead; any float triple is accepted (include/dvc.h).
    """
    p = N.FdParams()
    p.width, p.height = int(width), int(height)
    p.block = int(block_size)
    p.ithresh = max(-1, min(255, math.floor(motion_threshold)))
    p.min_area2 = math.floor(2.0 * float(min_area))
    p.ksize = int(kernel_size)
    p.anchor = int(kernel_size) // 2
    p.alpha = float(release_factor)
    p.beta = float(1 - release_factor)
    p.gamma = 0.0
    if accumulate is not None:
        p.alpha, p.beta, p.gamma = (float(v) for v in accumulate)
    p.quant = float(quantization_level)
    p.prime_ksize = 25   # fd:77
    p.prime_sigma = 30.0
    p.flags = flags
    p.src_width, p.src_height = int(src_width or 0), int(src_height or 0)
    p.in_format = N.FORMATS[in_format]
    p.chroma_rows = int(chroma_rows)
    return p


class FDWorker(Worker):
    _abi, _destroy = "dvc_fd", "dvc_fd_destroy"
    _outs = ("overlay", "compressed")

    def __init__(self, width: int, height: int, *, device: int = 0, stream=None,
                 device_ptrs: bool = False, keep_planes: bool = False, ktiming: bool = False,
                 max_batch: int = 1, out_format: str = "BGR", fused: bool = True, kept_plane: bool = False,
                 **kwargs):
        """``width, height``: the scaled frame size (fd:60-61); frames handed to
        :meth:`prime`/:meth:`step` are ``src_width x src_height`` (the video's,
        default the same) and are resized on the GPU (fd:74,91).
        ``max_batch``: frames one device launch covers in :meth:`step_batch`
        (bit planes for four slots of max_batch frames in flight and the
        contour filter's working arrays for one; the graph path adds a filter
        set per slot, grown to the batch, for batches of up to 128 frames:
        ~17 MB a 1080p frame and slot, fd_api.hip). ``stream``: the
        caller's HIP stream (``torch.cuda.Stream.cuda_stream``), joined as
        dvc_fd_create documents. ``in_format`` (kwarg) "BGR" / "I420" / "NV12":
        the frames handed over (4:2:0 decoder surfaces are converted on the GPU);
        ``out_format`` "BGR" or "I420": overlay and compressed frames as the
        encoder's 4:2:0 input (DVC_FLAG_OUT_I420). ``fused=False``: outputs in
        one k_out pass instead of the fused front's speculative static-block
        outputs + k_fix (DVC_FLAG_FD_UNFUSED; same bytes). ``kept_plane=True``:
        the kept mask goes from the contour filter to the dilation through
        device memory instead of staying on chip (DVC_FLAG_FD_KEPT_PLANE; same
        bytes)."""
        if out_format not in ("BGR", "I420"):
            raise ValueError(f"out_format {out_format!r}: BGR or I420")
        flags = (N.DVC_FLAG_OUT_I420 if out_format == "I420" else 0) | (0 if fused else N.DVC_FLAG_FD_UNFUSED) | \
            (N.DVC_FLAG_FD_KEPT_PLANE if kept_plane else 0)
        self.out_format = out_format
        W, H = int(width), int(height)
        self.SW = int(kwargs.get("src_width") or width)
        self.SH = int(kwargs.get("src_height") or height)
        # output frames (scaled size): packed BGR, or (H*3/2, W) I420
        self._oshape = (H, W, 3) if out_format == "BGR" else (H * 3 // 2, W)
        self._open(derive_params(width, height, flags=flags, **kwargs), kwargs.get("in_format", "BGR"),
                   (self.SW, self.SH), (self._oshape, self._oshape), device=device, stream=stream,
                   device_ptrs=device_ptrs, keep_planes=keep_planes, ktiming=ktiming, max_batch=max_batch)

    def set_state(self, prev_gray, acc) -> None:
        """Resume instead of :meth:`prime` (dvc_fd_set_state): the previous
        blurred gray and the accumulated mask (fd:107,133), H x W uint8 each —
        what :meth:`plane` exports as PLANE_GRAY / PLANE_ACC."""
        g = np.ascontiguousarray(prev_gray, dtype=np.uint8)
        a = np.ascontiguousarray(acc, dtype=np.uint8)
        if g.shape != (self.H, self.W) or a.shape != (self.H, self.W):
            raise ValueError(f"state planes must be ({self.H}, {self.W})")
        N.check(self._lib.dvc_fd_set_state(self._h, g.ctypes.data, a.ctypes.data))

    def step(self, frame, overlay=None, compressed=None, acc=None, want=("overlay", "compressed")):
        """fd:91-133 for one frame.

        Host mode: returns ``(overlay, compressed)`` numpy frames (allocated if
        not given; a name missing from ``want`` is skipped). Device mode: writes
        into the given device buffers (None = not produced) and returns None.
        """
        if acc is not None:   # the accumulated mask after this frame: only into a given buffer
            if self.device_ptrs:
                acc = B.device_buf(acc, (self.H, self.W), self.device, "acc", batched=False)[0]
            else:
                acc = B.host_out(acc, (self.H, self.W), "acc", False).ctypes.data
        return self._step(frame, overlay, compressed, want, acc)

    def step_batch(self, frames, overlay=None, compressed=None, want=("overlay", "compressed")):
        """fd:85-138 for n consecutive frames (identical to n :meth:`step` calls).

        Host mode: ``frames`` is an (n, H, W, 3) uint8 array; returns
        ``(overlay, compressed)`` arrays of the same shape (allocated if not
        given; a name missing from ``want`` is None). Device mode: ``frames``,
        ``overlay``, ``compressed`` are (n, H, W, 3) uint8 CUDA tensors on the
        handle's device (outputs may hold more frames), or explicit
        ``(address, n)`` tuples of dense frames; asynchronous, returns None.
        """
        return self._step_batch(frames, overlay, compressed, want)

    def ktime_kernel(self) -> str:
        """Which kernel ktime() timed in the last batch: "k_front_fused" (the fused
        front with the speculative outputs) or "k_out"."""
        if not hasattr(self._lib, "dvc_fd_ktime_kernel"):   # an older build (DVC_LIB_PATH A/B)
            return "k_out"
        k = self._lib.dvc_fd_ktime_kernel(self._h)
        if k < 0:
            N.check(k)
        return "k_front_fused" if k == N.KTIME_FRONT_FUSED else "k_out"

    def acc_form(self) -> str:
        """The accumulate kernel this handle launches (dvc_fd_acc_form): "short" or
        "general" (k_acc<4 / 8>; DVC_ACC_GENERAL=1 at create forces the latter) or "rows"."""
        k = self._lib.dvc_fd_acc_form(self._h)
        if k < 0:
            N.check(k)
        return {N.ACC_FORM_GENERAL: "general", N.ACC_FORM_SHORT: "short", N.ACC_FORM_ROWS: "rows"}[k]

    def graph_stats(self) -> dict:
        """Batches launched as HIP graphs (the short-batch device path) and graphs built."""
        b, g = ctypes.c_uint64(), ctypes.c_uint64()
        N.check(self._lib.dvc_fd_graph_stats(self._h, ctypes.byref(b), ctypes.byref(g)))
        return {"batches": int(b.value), "builds": int(g.value)}
