"""Host side of the drop-in drivers' frame loops (``frame_differencing.py:85-138``,
``motion_compression_opt.py:65-101``) in three threads.

The reference reads a frame, processes it and writes it, one after the other.
Here a reader thread fills page-locked chunks of R frames (``cap.read()``),
the calling thread steps each chunk with one ``step_batch`` call on the GPU,
and a writer thread emits the outputs (``VideoWriter.write``): reading chunk
c+1 and writing chunk c-1 overlap chunk c's step instead of adding to it.
Three buffers each way; file I/O, frame copies and the ctypes calls release
the GIL. An input chunk is recycled after the writer is done with it (the
OF driver writes the input frames as its overlay video).

Per-frame time (``frame_times``): the reference times each frame from its
``cap.read()`` to its last ``write`` (``frame_differencing.py:86,135``); its loop
is sequential, so that interval is also the time the frame adds to the run and
the per-frame times sum to the loop's wall time. The pipeline keeps that
second meaning: a frame's time is the wall-clock interval between the write
completion of the frame before it and its own (the first frame's starts at the
pipeline's first read), spread evenly over the frames of a chunk. So
frames x average = the loop's wall time <= the run's total time, as in the
reference; a frame's read-to-write latency inside the pipeline (about three
chunk periods) is not what the file reports.

``DeviceChain`` is the same pipeline with one or both ends on the device
(``DVC_DEVICE_CHAIN``, DESIGN.md §4 "Video I/O"): Motion-JPEG samples go up as
they are read and decode there, the workers step with device pointers, and the
outputs leave as encoded samples.
"""
from __future__ import annotations

import queue
import threading
import time

import numpy as np

from . import _native as N
from ._native import pinned


class ChunkPipeline:
    NBUF = 3

    def __init__(self, R, in_shape, out_shapes, read, emit, alloc=None):
        """``read()`` -> (ok, frame) (cap.read); ``emit(i, outs, done, failing)``
        writes the first ``done`` frames of input chunk ``i`` / output buffers
        ``outs`` (on the writer thread). ``alloc(shape)``: the buffers, default
        page-locked uint8 arrays (``_native.pinned``). ``in_shape`` may be a
        list of shapes: then ``read()`` returns (ok, (frame_a, frame_b, ..)) —
        several videos read in lockstep (compress_with_motion, of:142-143) —
        and ``ins[i]`` is a tuple of chunk arrays."""
        self.R, self.read, self.emit = R, read, emit
        alloc = alloc or pinned
        self.multi = isinstance(in_shape, list)
        shapes = in_shape if self.multi else [in_shape]
        self.ins = [tuple(alloc((R,) + tuple(sh)) for sh in shapes) for _ in range(self.NBUF)]
        if not self.multi:
            self.ins = [x[0] for x in self.ins]
        self.outs = [tuple(alloc((R,) + tuple(s)) for s in out_shapes) for _ in range(self.NBUF)]
        self.free_in, self.free_out = queue.Queue(), queue.Queue()
        for k in range(self.NBUF):
            self.free_in.put(k)
            self.free_out.put(k)
        self.filled, self.to_write = queue.Queue(), queue.Queue()
        self.error = None
        self._stop = threading.Event()
        self.reader = self.writer = None
        self.t0 = None
        self.departures = []             # (time the chunk's last write returned, frames in it)

    def start(self):
        self.t0 = time.time()
        self.reader = threading.Thread(target=self._read_loop, name="dvc-reader", daemon=True)
        self.writer = threading.Thread(target=self._write_loop, name="dvc-writer", daemon=True)
        self.reader.start()
        self.writer.start()
        return self.reader, self.writer

    def _read_loop(self):
        try:
            while not self._stop.is_set():
                i = self.free_in.get()
                if i is None:
                    return
                n = 0
                while n < self.R:
                    ok, f = self.read()
                    if not ok:
                        break
                    if self.multi:
                        for buf, x in zip(self.ins[i], f):
                            buf[n] = x
                    else:
                        self.ins[i][n] = f
                    n += 1
                self.filled.put((i, n))
                if n < self.R:           # end of the video
                    return
        except Exception as e:           # surfaced by next_chunk
            self.error = e
            self.filled.put((None, 0))

    def _write_loop(self):
        try:
            while True:
                item = self.to_write.get()
                if item is None:
                    return
                i, j, done, failing = item
                self.emit(i, self.outs[j], done, failing)
                self.departures.append((time.time(), done))
                self.free_out.put(j)
                self.free_in.put(i)
        except Exception as e:           # surfaced by next_chunk / out_buffer / finish
            self.error = e
            self.free_out.put(None)
            self.free_in.put(None)       # the reader stops
            self.filled.put((None, 0))   # a caller waiting for a chunk wakes up

    def next_chunk(self):
        """(input chunk index, frames in it); 0 frames at the end of the video."""
        i, n = self.filled.get()
        if self.error is not None:
            raise self.error
        return i, n

    def out_buffer(self):
        j = self.free_out.get()
        if j is None:
            raise self.error
        return j

    def write(self, i, j, done, failing=False):
        self.to_write.put((i, j, done, failing))

    def finish(self):
        """Wait until every chunk handed to write() is written."""
        self.to_write.put(None)
        self.writer.join()
        if self.error is not None:
            raise self.error

    def frame_times(self):
        """Seconds per written frame (module docstring): chunk c's frames share
        the interval since chunk c-1's writes completed."""
        out, prev = [], self.t0
        for t, done in self.departures:
            if done > 0:
                out.extend([(t - prev) / done] * done)
                prev = t
        return out

    def stop(self):
        self._stop.set()
        self.free_in.put(None)
        self.to_write.put(None)
        for t in (self.reader, self.writer):
            if t is not None:
                t.join(timeout=60)


def chain_mode() -> str:
    """``DVC_DEVICE_CHAIN``: auto (each end that qualifies), on (both, or raise), off."""
    import os
    mode = os.environ.get("DVC_DEVICE_CHAIN", "auto")
    if mode not in ("auto", "on", "off"):
        raise ValueError(f"DVC_DEVICE_CHAIN={mode!r}: auto, on or off")
    return mode


def device_source(cap):
    """Whether ``cap`` is a Motion-JPEG reader that decodes on the GPU: its samples
    can go to the device as they lie in the file (DeviceChain's device source)."""
    from . import video_io
    return isinstance(cap, video_io.Mp4MjpegReader) and cap.isOpened() and getattr(cap, "_gpu", False) \
        and hasattr(N.JpegDecoder, "decode_device")


def device_sinks(sinks, R):
    """(engage, reason): whether every sink is an ``Mp4MjpegWriter`` whose encoder has
    the stream output; with optimised tables or a rate target (both work group by
    group) the chunks must also hold whole table groups (``reason`` "groups": the host path keeps today's groups, even under on)."""
    from . import video_io
    for s in sinks:
        if not isinstance(s, video_io.Mp4MjpegWriter) or not s._own_encoder or \
                not hasattr(s._enc, "encode_stream") or not hasattr(N.lib(), "dvc_jpeg_encode_stream"):
            return False, "encoder"
    if any((s.optimize or s.target_bytes is not None) and R % s._batch for s in sinks):
        return False, "groups"
    return True, ""


HOST_CHAIN_LINE = "device chain: source=host sink=host h2d=0 d2h=0"   # the log line of a run with no device end


def _torch_cuda() -> bool:
    try:
        import torch
        return bool(torch.cuda.is_available())
    except Exception:
        return False


def chain_ends(mode, cap, sinks, R):
    """(source on the device, sinks on the device) for ``DVC_DEVICE_CHAIN=mode``. Under
    ``on`` a Motion-JPEG end that cannot engage raises (a silent fallback cannot
    pass a test); a source or sink of another kind has no device form, and
    optimised tables whose groups the chunks would cut keep the host sink."""
    from . import video_io
    if mode == "off":
        return False, False
    # the chain's tensors and events are torch's: without torch (the drivers alone never needed
    # it), or with a library that lacks dvc_stream_create, both ends stay on the host
    usable = _torch_cuda() and hasattr(N.lib(), "dvc_stream_create")
    src = usable and device_source(cap)
    snk, why = device_sinks(sinks, R)
    snk, why = (snk, why) if usable else (False, "encoder")
    if mode == "on":
        if not src and isinstance(cap, video_io.Mp4MjpegReader):
            raise RuntimeError("DVC_DEVICE_CHAIN=on: the Motion-JPEG source does not decode on the GPU")
        if not snk and why == "encoder" and any(isinstance(s, video_io.Mp4MjpegWriter) for s in sinks):
            raise RuntimeError("DVC_DEVICE_CHAIN=on: a Motion-JPEG sink's encoder has no stream output")
    return src, snk


def open_chain(mode, R, device, cap, sinks, in_shape, out_shapes, read):
    """(DeviceChain or None when both ends stay on the host, ok, first frame): the
    frame the drivers prime with, on the device when the source is. A first sample
    outside the GPU decoder's set sends the file to Pillow and the host source, as
    the reader itself does under ``DVC_MJPEG_DECODE=auto``."""
    src, snk = chain_ends(mode, cap, sinks, R)
    while True:
        chain = None
        if src or snk:
            chain = DeviceChain(R, device, in_shape, out_shapes, read, None, source=cap if src else None,
                                sinks=sinks if snk else None)
        if not src:
            ok, first = read()
            return chain, ok, first
        try:
            ok, first = chain.first_frame()
            return chain, ok, first
        except N.DvcError as e:
            chain.close()
            if e.code != N.DVC_E_UNSUPPORTED or mode != "auto" or cap._mode != "auto" or cap._Image is None:
                raise
            cap._i, src = 0, False


def _up16(v):
    return (int(v) + 15) & ~15


class DeviceChain(ChunkPipeline):
    """ChunkPipeline with one or both ends on the device, all on one torch stream
    that every handle of the run joins (``stream_ptr``).

    Device source (``source``: a GPU-decoding Motion-JPEG reader): the reader thread
    reads whole samples into page-locked slots, :meth:`next_chunk` uploads the slots
    as they are and enqueues ``JpegDecoder.decode_device`` — one call per run of
    samples that share a header — into ``d_in[i]``; the status words come down and
    a damaged sample ends the stream there. Otherwise ``read()`` fills page-locked
    chunks of raw frames as in ChunkPipeline and :meth:`next_chunk` uploads them.

    Device sink (``sinks``: one ``Mp4MjpegWriter`` per output): :meth:`write` hands
    the device frames to ``encode_stream``; the writer thread waits for the chunk's
    event, copies ``offsets`` and then ``offsets[n]`` bytes down and gives the block
    to ``write_samples``. Otherwise the outputs come down into page-locked buffers
    and ``emit`` writes them as in ChunkPipeline. ``emit(i, outs, done, failing)``:
    ``outs`` is None with a device sink (the files are written; emit counts).

    Every copy between host and device is issued here and counted (``h2d``,
    ``d2h``); device-pointer handles copy nothing."""

    FRAME_CAP = None   # bytes a frame of the device sample buffers; None: a raw frame's (tests set less)

    def __init__(self, R, device, in_shape, out_shapes, read, emit, source=None, sinks=None):
        import torch
        self.torch, self.R, self.read, self.emit = torch, R, read, emit
        self.device = int(device)
        self.dev = torch.device("cuda", self.device)
        # a run owns its two streams (the handles', and the writer thread's copies) and destroys
        # them in close(): nothing of it stays behind in the process
        self._streams = []
        self.stream = self._new_stream()
        self.copy_stream = self._new_stream()
        self.stream_ptr = self.stream.cuda_stream
        self.source, self.sinks = source, sinks
        self.h2d = self.d2h = self._d2h_writer = 0
        self.ended = False
        self.multi = False                  # one source (ChunkPipeline's read loop asks)

        def dev_buf(shape, dtype=torch.uint8):
            return torch.empty(tuple(shape), dtype=dtype, device=self.dev)

        def pin(shape, dtype=torch.uint8):
            # page-locked memory of the library's (dvc_host_alloc), viewed as a tensor: torch's own
            # pinned allocator would record events on the run's streams when a buffer is freed,
            # which is after close() has destroyed them
            names = {torch.uint8: "uint8", torch.int32: "int32", torch.int64: "int64"}
            return torch.from_numpy(pinned(tuple(shape), names[dtype]))

        self._pin = pin
        self.d_in = [dev_buf((R,) + tuple(in_shape)) for _ in range(self.NBUF)]
        self.d_outs = [tuple(dev_buf((R,) + tuple(s)) for s in out_shapes) for _ in range(self.NBUF)]
        if source is not None:
            sizes = [s for _, s in source.samples] or [16]
            self.slot_cap = _up16(max(sizes))
            self.h_slots = [pin((R * self.slot_cap,)) for _ in range(self.NBUF)]
            self.d_slots = [dev_buf((R * self.slot_cap,)) for _ in range(self.NBUF)]
            self.h_sizes = [pin((R,), torch.int32) for _ in range(self.NBUF)]
            self.d_sizes, self.d_status = dev_buf((R,), torch.int32), dev_buf((R,), torch.int32)
            self.h_status = pin((R,), torch.int32)
            self.dec = N.JpegDecoder(source.W, source.H, R, self.device, camera=self._camera(source),
                                     device_ptrs=True, stream=self.stream_ptr)
            self.shape0 = None          # (W, H, fmt) of the first sample: the stream's
            self.pillow = False         # a JPEG outside the decoder's set arrived: Pillow from there on
        else:
            self.h_ins = [pin((R,) + tuple(in_shape)) for _ in range(self.NBUF)]
            self.ins = [t.numpy() for t in self.h_ins]
        if sinks is not None:
            self.enc = [s.device_encoder(self.stream_ptr) for s in sinks]
            # as _native.JpegEncoder.encode: slots of the raw frame size almost always fit
            self.cap = [min(e.bound + len(e.header), self.FRAME_CAP or max(4096, int(torch.Size(s).numel()))) * R
                        for e, s in zip(self.enc, out_shapes)]
            self.d_enc = [tuple(dev_buf((c,)) for c in self.cap) for _ in range(self.NBUF)]
            self.d_offs = [tuple(dev_buf((R + 1,), torch.int64) for _ in sinks) for _ in range(self.NBUF)]
            self.h_offs = [pin((R + 1,), torch.int64) for _ in sinks]
            self.h_bytes = [pin((max(c // 4, 4096),)) for c in self.cap]
        else:
            self.h_outs = [tuple(pin((R,) + tuple(s)) for s in out_shapes) for _ in range(self.NBUF)]
            self.outs = [tuple(t.numpy() for t in x) for x in self.h_outs]
        self.free_in, self.free_out = queue.Queue(), queue.Queue()
        for k in range(self.NBUF):
            self.free_in.put(k)
            self.free_out.put(k)
        self.filled, self.to_write = queue.Queue(), queue.Queue()
        self.error = None
        self._stop = threading.Event()
        self.reader = self.writer = None
        self.t0 = None
        self.departures = []

    def _new_stream(self):
        import ctypes
        s = ctypes.c_void_p()
        N.check(N.lib().dvc_stream_create(self.device, ctypes.byref(s)))
        self._streams.append(s)
        return self.torch.cuda.ExternalStream(s.value, device=self.dev)

    @staticmethod
    def _camera(source) -> bool:
        from . import video_io
        return isinstance(source, video_io._CameraMjpegReader)

    # ------------------------------------------------------------ the source --
    def _copy_up(self, dst, src):
        dst.copy_(src, non_blocking=True)
        self.h2d += src.numel() * src.element_size()

    def _decode(self, i, n, sizes, stride):
        """Upload chunk i's n slots and enqueue their decoding into d_in[i]; returns the
        frames before the first sample that ends the stream (n: none does)."""
        torch, src, dec = self.torch, self.source, self.dec
        host = self.h_slots[i].numpy()
        slots = self.d_slots[i][:n * stride]
        self._copy_up(slots, self.h_slots[i][:n * stride])
        slots = slots.view(n, stride)
        out, hsz = self.d_in[i], self.h_sizes[i]
        ok, a, decoded = n, 0, 0

        def run(a, b):                      # samples a..b-1 share the current header
            nonlocal decoded
            if b > a:
                hl = len(dec._hdr)
                for t in range(a, b):
                    hsz[t] = sizes[t] - hl
                self._copy_up(self.d_sizes[a:b], hsz[a:b])
                dec.decode_device(slots[a:], hl, self.d_sizes[a:b], out[a:], self.d_status[a:b], b - a)
                decoded = b

        for t in range(n):
            sample = host[t * stride:t * stride + sizes[t]]
            hdr = dec._hdr
            if not self.pillow and hdr is not None and sizes[t] > len(hdr) and sample[:len(hdr)].tobytes() == hdr:
                continue
            run(a, t)
            a = t + 1                        # (moved back to t below when the sample opens a new run)
            if not self.pillow:
                try:
                    hl = dec.set_header(sample.tobytes())
                except N.DvcError as e:
                    if e.code != N.DVC_E_UNSUPPORTED:
                        ok = t               # no header: a damaged sample
                        break
                    if src._mode != "auto" or src._Image is None or self.shape0 is None:
                        raise
                    self.pillow = True       # this file goes to Pillow from here on
            if self.pillow:
                try:
                    f = src._pillow(sample.tobytes())
                except (OSError, SyntaxError, ValueError):
                    if not self._camera(src):
                        raise
                    ok = t
                    break
                if f.shape != tuple(out.shape[1:]):
                    ok = t
                    break
                self._copy_up(out[t], torch.from_numpy(np.array(f)))
                continue
            shape = (dec.W, dec.H, dec.fmt)
            if self.shape0 is None:
                self.shape0 = shape
            if shape != self.shape0 or sizes[t] <= hl:   # another frame size, or nothing behind the header
                ok = t
                break
            a = t
        else:
            run(a, n)
        if decoded:
            self.h_status[:decoded].copy_(self.d_status[:decoded], non_blocking=True)
            self.d2h += 4 * decoded
            self.stream.synchronize()
            bad = np.flatnonzero(self.h_status[:decoded].numpy())
            if len(bad):
                ok = min(ok, int(bad[0]))
        return ok

    def on_device(self, frame):
        """``frame`` as a device tensor: as it is when it is one, else uploaded."""
        torch = self.torch
        if isinstance(frame, torch.Tensor):
            return frame
        h = torch.from_numpy(np.array(frame))
        d = torch.empty(h.shape, dtype=h.dtype, device=self.dev)   # (allocated outside the run's stream: it outlives it)
        with torch.cuda.stream(self.stream):
            d.copy_(h)
            self.h2d += d.numel()
            self.stream.synchronize()
        return d

    def first_frame(self):
        """Sample 0 decoded alone (the frame the drivers prime with): (ok, device frame)."""
        torch, src = self.torch, self.source
        first = torch.empty_like(self.d_in[0][:1])
        with torch.cuda.stream(self.stream):
            size = src.read_sample_into(self.h_slots[0].numpy())
            if size <= 0:
                return False, None
            keep, self.d_in[0] = self.d_in[0], first
            try:
                ok = self._decode(0, 1, [size], _up16(size))
            finally:
                self.d_in[0] = keep
            self.stream.synchronize()
        return (ok == 1), (first[0] if ok == 1 else None)

    def _read_loop(self):
        if self.source is None:
            return ChunkPipeline._read_loop(self)
        try:
            src = self.source
            while not self._stop.is_set():
                i = self.free_in.get()
                if i is None:
                    return
                ahead = [s for _, s in src.samples[src._i:src._i + self.R]]
                stride = _up16(max(ahead)) if ahead else 16
                host, sizes = self.h_slots[i].numpy(), []
                for t in range(len(ahead)):
                    got = src.read_sample_into(host[t * stride:(t + 1) * stride])
                    if got < 0:
                        break
                    sizes.append(got)
                self.filled.put((i, len(sizes), sizes, stride))
                if len(sizes) < self.R:
                    return
        except Exception as e:
            self.error = e
            self.filled.put((None, 0))

    def next_chunk(self):
        """(input chunk index, frames in it) with the frames in ``d_in[i]``; 0 frames at
        the end of the video. ``ended`` is set once the stream has ended (a short chunk
        alone does not say so)."""
        item = self.filled.get()
        if self.error is not None:
            raise self.error
        torch = self.torch
        with torch.cuda.stream(self.stream):
            if self.source is not None:
                i, n, sizes, stride = item
                ok = self._decode(i, n, sizes, stride) if n else 0
                self.ended = self.ended or ok < n or n < self.R
                return i, ok
            i, n = item
            if n:
                self._copy_up(self.d_in[i][:n], self.h_ins[i][:n])
            self.ended = self.ended or n < self.R
            return i, n

    # -------------------------------------------------------------- the sink --
    def write(self, i, j, done, failing=False, frames=None):
        """Chunk i's outputs: ``frames`` (default ``d_outs[j]``), the first ``done`` of
        each — and with ``failing`` one more of the first (fd:112 < fd:122)."""
        torch = self.torch
        frames = list(self.d_outs[j] if frames is None else frames)
        counts = [done + (1 if failing and k == 0 else 0) for k in range(len(frames))]
        with torch.cuda.stream(self.stream):
            for k, (f, c) in enumerate(zip(frames, counts)):
                if not c:
                    continue
                if self.sinks is not None:
                    self.enc[k].encode_stream(f[:c], self.d_enc[j][k], self.d_offs[j][k])
                else:
                    self.h_outs[j][k][:c].copy_(f[:c], non_blocking=True)
                    self.d2h += f[:c].numel()
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.to_write.put((i, j, done, failing, frames, counts, ev))

    def _down(self, dst, src):
        with self.torch.cuda.stream(self.copy_stream):
            dst.copy_(src, non_blocking=True)
        self.copy_stream.synchronize()
        self._d2h_writer += src.numel() * src.element_size()     # (the writer thread's own count)

    def _write_samples(self, j, k, frames, count):
        """Sink k's block of chunk buffer j -> its file. Samples that did not fit the
        device buffer (and, to keep the table groups, their group) go the host way."""
        sink, offs = self.sinks[k], self.h_offs[k]
        self._down(offs[:count + 1], self.d_offs[j][k][:count + 1])
        o = offs[:count + 1].tolist()
        fit = count
        while fit and o[fit] > self.cap[k]:
            fit -= 1
        if fit < count:
            # (the device encoder's overflow word stays set from here on: only dvc_jpeg_sync reads
            # and clears it, and the chain never calls it; the offsets above are what tells)
            fit -= fit % sink._batch
        if o[fit]:
            if self.h_bytes[k].numel() < o[fit]:
                self.h_bytes[k] = self._pin((o[fit] + o[fit] // 4,))
            self._down(self.h_bytes[k][:o[fit]], self.d_enc[j][k][:o[fit]])
            sink.write_samples(self.h_bytes[k].numpy(), o[:fit + 1])
        if fit < count:
            rest = self._pin(tuple(frames[fit:count].shape))
            self._down(rest, frames[fit:count])
            for f in rest.numpy():
                sink.write(f)

    def _write_loop(self):
        try:
            while True:
                item = self.to_write.get()
                if item is None:
                    return
                i, j, done, failing, frames, counts, ev = item
                ev.synchronize()
                if self.sinks is not None:
                    for k, c in enumerate(counts):
                        if c:
                            self._write_samples(j, k, frames[k], c)
                    self.emit(i, None, done, failing)
                else:
                    self.emit(i, self.outs[j], done, failing)
                self.departures.append((time.time(), done))
                self.free_out.put(j)
                self.free_in.put(i)
        except Exception as e:
            self.error = e
            self.free_out.put(None)
            self.free_in.put(None)
            self.filled.put((None, 0))

    def log_line(self) -> str:
        return (f"device chain: source={'device' if self.source is not None else 'host'} "
                f"sink={'device' if self.sinks is not None else 'host'} h2d={self.h2d} "
                f"d2h={self.d2h + self._d2h_writer}")

    def close(self):
        """The chain's handles, then its streams (the workers that joined them are closed before)."""
        for h in ([self.dec] if self.source is not None else []) + (self.enc if self.sinks is not None else []):
            h.close()
        streams, self._streams = self._streams, []
        if streams:
            self.torch.cuda.synchronize(self.dev)
        for s in streams:
            N.check(N.lib().dvc_stream_destroy(self.device, s))
