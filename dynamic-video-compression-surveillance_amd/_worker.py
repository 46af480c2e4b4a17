"""What the two per-frame workers share: one feed handle (``dvc_fd`` or
``dvc_of``, include/dvc.h) that is created with the same flags and optional
stream, primed with frame 0, stepped by frames or batches of frames in host or
device mode into two outputs, and queried the same way. ``fd.py`` and ``of.py``
add what differs: the parameters, the outputs' names and shapes, and each
path's extra calls.

``step`` is host-bound at one frame a call, so everything a call needs is
resolved per handle at construction: the bound C functions, the frame shapes,
pitch and byte counts.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _buffers as B
from . import _native as N


class Worker(N.Handle):
    _abi = ""          # "dvc_fd" / "dvc_of": the prefix of the handle's C functions
    _outs = ("", "")   # the names of the two outputs of step / step_batch
    _astride = ()      # the first output's own stride in step_batch, where the C call takes one

    def _open(self, params, in_format, src, shapes, *, device, stream, device_ptrs, keep_planes, ktiming, max_batch):
        """Create the handle for ``params`` (a dvc_*_params without the common
        flags and max_batch). ``src``: (width, height) of the ``in_format``
        frames handed in; ``shapes``: the per-frame shapes of the two outputs."""
        params.flags |= (N.DVC_FLAG_DEVICE_PTRS if device_ptrs else 0) \
            | (N.DVC_FLAG_KEEP_PLANES if keep_planes else 0) | (N.DVC_FLAG_KTIMING if ktiming else 0) \
            | (N.DVC_FLAG_JOIN_STREAM if stream is not None else 0)
        params.max_batch = int(max_batch)
        self.params = params
        self.W, self.H = int(params.width), int(params.height)
        self.in_format = in_format
        self.device = int(device)
        self.device_ptrs = device_ptrs
        sw, sh = src
        # input frames: packed BGR, or a (H*3/2, W) 4:2:0 frame
        self._fshape = (sh, sw, 3) if self.in_format == "BGR" else (sh * 3 // 2, sw)
        self._pitch = 3 * sw if self.in_format == "BGR" else sw
        self._aname, self._bname = self._outs
        self._ashape, self._bshape = shapes
        self._fbytes, self._bbytes = int(np.prod(self._fshape)), int(np.prod(self._bshape))
        self._lib = L = N.lib()
        self._c_prime, self._c_step, self._c_step_batch, self._c_sync, self._c_stats, self._c_plane, self._c_ktime = (
            getattr(L, f"{self._abi}_{f}")
            for f in ("prime", "step", "step_batch", "sync", "get_stats", "read_plane", "ktime"))
        s = ctypes.c_void_p(int(stream)) if stream is not None else None
        self._create(getattr(L, self._abi + "_create"), ctypes.byref(params), self.device, s)

    # -------------------------------------------------------------- frames --
    def prime(self, frame) -> None:
        """Frame 0. FD (fd:67-81): previous gray := GaussianBlur(gray(frame), 25x25, 30);
        acc := 0. OF (of:54-62): previous gray := gray(frame); the vote window is emptied."""
        if self.device_ptrs:
            addr = B.device_buf(frame, self._fshape, self.device, "frame", batched=False)[0]
        else:
            f = B.host_in(frame, self._fshape, "frame")
            addr = f.ctypes.data
        N.check(self._c_prime(self._h, addr, self._pitch))

    def _step(self, frame, a, b, want, *more):
        """One frame into the outputs ``a`` and ``b``; ``more``: the call's
        further pointer arguments, marshalled by the caller."""
        if self.device_ptrs:
            dev, buf = self.device, B.device_buf
            addr = buf(frame, self._fshape, dev, "frame", batched=False)[0]
            pa = buf(a, self._ashape, dev, self._aname, batched=False)[0] if a is not None else None
            pb = buf(b, self._bshape, dev, self._bname, batched=False)[0] if b is not None else None
            N.check(self._c_step(self._h, addr, self._pitch, pa, pb, *more))
            return None
        f = B.host_in(frame, self._fshape, "frame")
        a = B.host_out(a, self._ashape, self._aname, self._aname in want)
        b = B.host_out(b, self._bshape, self._bname, self._bname in want)
        N.check(self._c_step(self._h, f.ctypes.data, self._pitch, a.ctypes.data if a is not None else None,
                             b.ctypes.data if b is not None else None, *more))
        return a, b

    def _step_batch(self, frames, a, b, want):
        fshape = self._fshape
        if self.device_ptrs:
            dev, buf = self.device, B.device_buf
            addr, n = buf(frames, fshape, dev, "frames", batched=True)
            pa = buf(a, self._ashape, dev, self._aname, n=n, batched=True)[0] if a is not None else None
            pb = buf(b, self._bshape, dev, self._bname, n=n, batched=True)[0] if b is not None else None
            N.check(self._c_step_batch(self._h, addr, self._pitch, self._fbytes, n, pa, *self._astride, pb,
                                       self._bbytes))
            return None
        if not isinstance(frames, np.ndarray) or frames.ndim != len(fshape) + 1:
            raise ValueError(f"frames: expected uint8 frames of shape (n, {', '.join(map(str, fshape))})")
        n = int(frames.shape[0])
        f = B.host_in(frames, (n,) + fshape, "frames")
        a = B.host_out(a, (n,) + self._ashape, self._aname, self._aname in want)
        b = B.host_out(b, (n,) + self._bshape, self._bname, self._bname in want)
        N.check(self._c_step_batch(self._h, f.ctypes.data, self._pitch, self._fbytes, n,
                                   a.ctypes.data if a is not None else None, *self._astride,
                                   b.ctypes.data if b is not None else None, self._bbytes))
        return a, b

    # ------------------------------------------------------------- queries --
    def sync(self) -> None:
        N.check(self._c_sync(self._h))

    def stats(self) -> dict:
        s = N.FdStats()   # dvc_fd_stats and dvc_of_stats: the same four counters
        N.check(self._c_stats(self._h, ctypes.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in N.FdStats._fields_}

    def plane(self, which: int) -> np.ndarray:
        """One H x W plane of the last stepped frame (N.PLANE_* / N.OF_PLANE_*)."""
        out = np.empty((self.H, self.W), np.uint8)
        N.check(self._c_plane(self._h, int(which), out.ctypes.data))
        return out

    def ktime(self, reset: bool = False):
        """(total ms, launches) of the path's dominant kernel, hipEvent-timed (``ktiming=True``)."""
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        N.check(self._c_ktime(self._h, ctypes.byref(ms), ctypes.byref(n), 1 if reset else 0))
        return float(ms.value), int(n.value)
