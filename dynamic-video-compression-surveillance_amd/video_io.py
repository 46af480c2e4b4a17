"""Frame sources and sinks for the reference-compatible drivers.

The reference reads with ``cv2.VideoCapture`` and writes ``mp4v`` with
``cv2.VideoWriter`` (``frame_differencing.py:39,63-65``;
``motion_compression_opt.py:39,50-52,121-122,135-136``). The codec is outside
the accelerated path. Here:

* ``*.npy`` clips (N x H x W x 3 uint8 BGR, memory-mapped) and
  ``synthetic://WxH?frames=N&seed=S&noisy=0|1&fps=F`` URIs are always readable;
* ``*.y4m`` (YUV4MPEG2, 4:2:0) videos are always readable: ``read()`` returns
  the BGR frame cv2.VideoCapture would (cvtColor YUV2BGR_I420, converted on
  the GPU by ``dvc_yuv420_to_bgr``), ``read_yuv()`` the raw 4:2:0 frame, which
  the FD driver hands to the GPU worker as is (in_format I420: the conversion
  runs in the worker's front stage, the decoded surface never round-trips);
* anything else goes through ``cv2.VideoCapture`` when OpenCV is importable;
* ``*.mp4`` outputs are written with ``cv2.VideoWriter(mp4v)`` when OpenCV is
  importable, otherwise as an ``.npy`` frame stream next to the requested name
  (same basename) so every output frame is still inspectable, or — with
  ``DVC_VIDEO_SINK=y4m`` or a ``.y4m`` name — as a YUV4MPEG2 video (colour
  frames 4:2:0 via ``dvc_bgr_to_i420`` on the GPU = cvtColor BGR2YUV_I420;
  single-channel frames as ``Cmono``) that any player or encoder reads, or —
  with ``DVC_VIDEO_SINK=mjpeg`` — as a real ``.mp4``: Motion-JPEG in ISO BMFF
  (an ``mp4v`` sample entry whose ``esds`` says objectTypeIndication 0x6C,
  ISO/IEC 10918-1), every frame a baseline JPEG encoded on the GPU by
  ``dvc_jpeg_encode`` at ``DVC_VIDEO_QUALITY`` (default 75), with the fixed
  Huffman tables or, with ``DVC_VIDEO_HUFFMAN=optimized``, tables built on the
  GPU for every batch of frames; with ``DVC_VIDEO_BITRATE`` (kbit/s) the
  quality is not fixed but searched on the GPU for every batch, inside
  ``DVC_VIDEO_QUALITY_RANGE=lo:hi`` (default 10:95), so that the batch stays
  under the rate (DESIGN.md "Rate target"). These are not the
  reference's MPEG-4 Part 2 files (intra-only, another codec: sizes are not
  comparable with its), but they are compressed, so the size reduction
  ``performance_analysis`` reports means something;
* such an ``.mp4`` is readable again (``Mp4MjpegReader``: the samples demuxed
  here, decoded in batches on the GPU by ``dvc_jpegd_decode``, or by Pillow —
  the same bytes; ``DVC_MJPEG_DECODE=auto|gpu|pillow``) — the OF driver's
  second pass and ``performance_analysis`` read the files the first pass wrote;
* camera Motion-JPEG is readable without OpenCV: ``*.avi`` (RIFF AVI with an
  ``MJPG`` video stream, :class:`AviMjpegReader`) and raw ``*.mjpeg`` /
  ``*.mjpg`` streams (JPEG images end to end, :class:`MjpegStreamReader`; the
  file carries no frame rate: ``DVC_MJPEG_FPS``, default 25). Both decode on a
  camera handle (``JpegDecoder(camera=True)``: 4:2:0, 4:2:2, 4:4:4, frames
  without DHT segments) and obey ``DVC_MJPEG_DECODE`` as above.
"""
from __future__ import annotations

import json
import logging
import os
import struct
from urllib.parse import parse_qs, urlparse

import numpy as np

try:  # optional: only used for real video files
    import cv2  # type: ignore
except Exception:  # pragma: no cover - cv2 is absent in this image
    cv2 = None

CAP_PROP_FPS = 5
CAP_PROP_FRAME_WIDTH = 3
CAP_PROP_FRAME_HEIGHT = 4
CAP_PROP_FRAME_COUNT = 7


class _ArraySource:
    def __init__(self, frames, fps: float):
        self._f = frames
        self._fps = float(fps)
        self._i = 0

    def isOpened(self) -> bool:
        return self._f is not None

    def get(self, prop: int) -> float:
        if prop == CAP_PROP_FPS:
            return self._fps
        if prop == CAP_PROP_FRAME_WIDTH:
            return float(self._f.shape[2])
        if prop == CAP_PROP_FRAME_HEIGHT:
            return float(self._f.shape[1])
        if prop == CAP_PROP_FRAME_COUNT:
            return float(len(self._f))
        return 0.0

    def read(self):
        if self._f is None or self._i >= len(self._f):
            return False, None
        fr = np.ascontiguousarray(self._f[self._i])
        self._i += 1
        return True, fr

    def release(self) -> None:
        self._f = None


class _SyntheticFrames:
    """Lazy sequence view over a SyntheticClip (frames generated on read)."""

    def __init__(self, clip, n):
        self._clip, self._n = clip, int(n)
        self.shape = (self._n, clip.H, clip.W, 3)

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        return self._clip.frame(int(i))


class Y4mReader:
    """cv2.VideoCapture-like reader of a YUV4MPEG2 file with 4:2:0 chroma
    (C420jpeg / C420 / C420paldv / C420mpeg2 / no C tag). Frames are memory-mapped;
    ``pixel_format`` is "I420". A Cmono file (what :class:`Y4mWriter` writes for a
    mask video) opens with ``pixel_format`` "GRAY": ``read`` gives its (H, W) frames."""

    pixel_format = "I420"

    def __init__(self, path: str, device: int = 0):
        self._mm, self._i, self.device = None, 0, int(device)
        try:
            with open(path, "rb") as f:
                head = f.readline(4096)
        except OSError:
            return
        tags = head.split()
        if not tags or tags[0] != b"YUV4MPEG2" or not head.endswith(b"\n"):
            return
        W = H = 0
        fps, chroma = 30.0, b"420jpeg"
        for t in tags[1:]:
            k, v = t[:1], t[1:]
            if k == b"W":
                W = int(v)
            elif k == b"H":
                H = int(v)
            elif k == b"F":
                num, den = v.split(b":")
                fps = int(num) / max(int(den), 1)
            elif k == b"C":
                chroma = v
        mono = chroma == b"mono"
        if W <= 0 or H <= 0 or not (mono or (W % 2 == 0 and H % 2 == 0 and chroma.startswith(b"420"))):
            return   # 4:4:4 / 4:2:2 sources are not 4:2:0 surfaces
        self.W, self.H, self.fps = W, H, fps
        if mono:
            self.pixel_format = "GRAY"
        self._frame_bytes = W * H if mono else W * H * 3 // 2
        raw = np.memmap(path, np.uint8, mode="r")
        off, frames = len(head), []
        while off < len(raw):   # FRAME[ params]\n + payload
            nl = off
            while nl < len(raw) and raw[nl] != 10:
                nl += 1
            if bytes(raw[off:off + 5]) != b"FRAME" or nl + 1 + self._frame_bytes > len(raw):
                break
            frames.append(nl + 1)
            off = nl + 1 + self._frame_bytes
        self._mm, self._offs = raw, frames

    def isOpened(self) -> bool:
        return self._mm is not None

    def get(self, prop: int) -> float:
        if self._mm is None:
            return 0.0
        return {CAP_PROP_FPS: self.fps, CAP_PROP_FRAME_WIDTH: float(self.W), CAP_PROP_FRAME_HEIGHT: float(self.H),
                CAP_PROP_FRAME_COUNT: float(len(self._offs))}.get(prop, 0.0)

    def read_yuv(self):
        """(ok, (H*3/2, W) uint8 I420 frame) — the decoder surface."""
        if self._mm is None or self._i >= len(self._offs):
            return False, None
        o = self._offs[self._i]
        self._i += 1
        return True, np.asarray(self._mm[o:o + self._frame_bytes]).reshape(self._frame_bytes // self.W, self.W)

    def read(self):
        """(ok, BGR frame) as cv2.VideoCapture.read() gives it (cvtColor on the GPU);
        a Cmono file's single-channel frame as it is."""
        ok, f = self.read_yuv()
        if not ok:
            return False, None
        if self.pixel_format == "GRAY":
            return True, f
        from ._native import yuv420_to_bgr
        return True, yuv420_to_bgr(f, "I420", self.device)

    def release(self) -> None:
        self._mm = None


class Y4mWriter:
    """cv2.VideoWriter-like YUV4MPEG2 writer: colour frames (BGR) as 4:2:0
    (C420jpeg, cvtColor BGR2YUV_I420 on the GPU), single-channel frames as Cmono."""

    def __init__(self, path: str, fps: float, size, is_color: bool = True, device: int = 0):
        self.path, self.W, self.H = path, int(size[0]), int(size[1])
        self.is_color, self.device, self.n = is_color, int(device), 0
        num, den = (int(round(float(fps) * 1000)), 1000) if float(fps) != int(fps) else (int(fps), 1)
        self._fp = None
        if is_color and (self.W % 2 or self.H % 2):
            return   # 4:2:0 needs even sides (cv2.VideoWriter would fail to open as well)
        self._fp = open(path, "wb")
        self._fp.write(b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s\n"
                       % (self.W, self.H, max(num, 1), den, b"C420jpeg" if is_color else b"Cmono"))

    def isOpened(self) -> bool:
        return self._fp is not None

    def write(self, frame: np.ndarray) -> None:
        if self._fp is None:
            return
        exp = (self.H, self.W, 3) if self.is_color else (self.H, self.W)
        if frame.shape != exp:   # cv2.VideoWriter silently drops mismatched frames
            return
        if self.is_color:
            from ._native import bgr_to_i420
            payload = bgr_to_i420(frame, self.device)
        else:
            payload = np.ascontiguousarray(frame, dtype=np.uint8)
        self._fp.write(b"FRAME\n")
        self._fp.write(payload.tobytes())
        self.n += 1

    def write_yuv(self, frame: np.ndarray) -> None:
        """A frame already in the stream's layout: (H*3/2, W) I420 for colour
        streams (e.g. the FD worker's DVC_FLAG_OUT_I420 outputs), (H, W) mono."""
        if self._fp is None:
            return
        exp = (self.H * 3 // 2, self.W) if self.is_color else (self.H, self.W)
        if frame.shape != exp:
            return
        self._fp.write(b"FRAME\n")
        self._fp.write(np.ascontiguousarray(frame, dtype=np.uint8).tobytes())
        self.n += 1

    def release(self) -> None:
        if self._fp is not None:
            self._fp.close()
            self._fp = None


def _box(kind: bytes, *payload: bytes) -> bytes:
    body = b"".join(payload)
    return struct.pack(">I4s", 8 + len(body), kind) + body


def _full(kind: bytes, version_flags: int, *payload: bytes) -> bytes:
    return _box(kind, struct.pack(">I", version_flags), *payload)


_MATRIX = struct.pack(">9I", 0x10000, 0, 0, 0, 0x10000, 0, 0, 0, 0x40000000)
_FTYP = _box(b"ftyp", b"isom", struct.pack(">I", 0x200), b"isom", b"iso2", b"mp41")


def fps_ratio(fps: float):
    """(timescale, ticks per frame) — the ratio Y4mWriter writes as F<num>:<den>."""
    num, den = (int(round(float(fps) * 1000)), 1000) if float(fps) != int(fps) else (int(fps), 1)
    return max(num, 1), den


class Mp4Muxer:
    """ISO BMFF writer of one Motion-JPEG video track: ``ftyp``, an ``mdat``
    streamed to disk (one sample = one chunk per frame; its 64-bit size patched
    at close), then ``moov`` with the sample tables. ``add_sample`` takes one
    complete JPEG image."""

    def __init__(self, path: str, fps: float, size):
        self.path, self.W, self.H = path, int(size[0]), int(size[1])
        self.timescale, self.delta = fps_ratio(fps)
        self.sizes, self.offsets = [], []
        self._fp = open(path, "wb")
        self._fp.write(_FTYP)
        self._mdat = self._fp.tell()
        self._fp.write(struct.pack(">I4sQ", 1, b"mdat", 16))   # largesize form

    def add_sample(self, data: bytes) -> None:
        self.offsets.append(self._fp.tell())
        self.sizes.append(len(data))
        self._fp.write(data)

    def add_samples(self, buffer, offsets) -> None:
        """Complete JPEG images back to back (dvc_jpeg_encode_stream's layout): sample t
        is ``buffer[offsets[t]:offsets[t + 1]]``. One ``write`` of the block."""
        offs = [int(o) for o in offsets]
        base = self._fp.tell() - offs[0]
        self.offsets.extend(base + o for o in offs[:-1])
        self.sizes.extend(b - a for a, b in zip(offs, offs[1:]))
        self._fp.write(memoryview(buffer)[offs[0]:offs[-1]])

    def _moov(self) -> bytes:
        n, dur = len(self.sizes), len(self.sizes) * self.delta
        # ES_Descriptor { ES_ID 1; DecoderConfigDescriptor { objectTypeIndication 0x6C = Visual
        # ISO/IEC 10918-1 (JPEG), streamType 4 (visual) }; SLConfigDescriptor { predefined 2 } }
        dcfg = struct.pack(">BBBB3sII", 0x04, 13, 0x6C, 0x11, b"\0\0\0", 0, 0)
        esds = _full(b"esds", 0, struct.pack(">BBHB", 0x03, 3 + len(dcfg) + 3, 1, 0), dcfg, b"\x06\x01\x02")
        mp4v = _box(b"mp4v", b"\0" * 6, struct.pack(">H", 1), b"\0" * 16, struct.pack(">HHIIIH", self.W, self.H,
                    0x480000, 0x480000, 0, 1), b"\0" * 32, struct.pack(">Hh", 24, -1), esds)
        stbl = _box(b"stbl",
                    _full(b"stsd", 0, struct.pack(">I", 1), mp4v),
                    _full(b"stts", 0, struct.pack(">III", 1, n, self.delta)),
                    _full(b"stsc", 0, struct.pack(">IIII", 1, 1, 1, 1)),
                    _full(b"stsz", 0, struct.pack(">II", 0, n), struct.pack(">%dI" % n, *self.sizes)),
                    _full(b"co64", 0, struct.pack(">I", n), struct.pack(">%dQ" % n, *self.offsets)))
        minf = _box(b"minf", _full(b"vmhd", 1, b"\0" * 8),
                    _box(b"dinf", _full(b"dref", 0, struct.pack(">I", 1), _full(b"url ", 1))), stbl)
        mdia = _box(b"mdia", _full(b"mdhd", 0, struct.pack(">IIIIHH", 0, 0, self.timescale, dur, 0x55C4, 0)),
                    _full(b"hdlr", 0, struct.pack(">I4s12s", 0, b"vide", b""), b"VideoHandler\0"), minf)
        tkhd = _full(b"tkhd", 3, struct.pack(">IIIII8sHHHH", 0, 0, 1, 0, dur, b"", 0, 0, 0, 0), _MATRIX,
                     struct.pack(">II", self.W << 16, self.H << 16))
        mvhd = _full(b"mvhd", 0, struct.pack(">IIIIIH10s", 0, 0, self.timescale, dur, 0x10000, 0x100, b""), _MATRIX,
                     b"\0" * 24, struct.pack(">I", 2))
        return _box(b"moov", mvhd, _box(b"trak", tkhd, mdia))

    def close(self) -> None:
        if self._fp is None:
            return
        end = self._fp.tell()
        self._fp.write(self._moov())
        self._fp.seek(self._mdat + 8)
        self._fp.write(struct.pack(">Q", end - self._mdat))
        self._fp.close()
        self._fp = None


class Mp4MjpegWriter:
    """cv2.VideoWriter-like writer of a Motion-JPEG ``.mp4``: frames (BGR, or
    single-channel when ``is_color`` is false) are JPEG-encoded on the GPU in
    batches of ``batch`` (the rest at release) and muxed by :class:`Mp4Muxer`.
    ``encoder``: anything with ``header`` and ``encode(frames) -> [bytes]``
    (default: :class:`_native.JpegEncoder` on ``device``; ``optimize=True``:
    with Huffman tables built on the GPU for every batch). ``bitrate_kbps``:
    no fixed ``quality`` but a target of ``bitrate_kbps * 125 / fps`` bytes a
    frame, met batch by batch with a quality of ``quality_range`` (DESIGN.md
    "Rate target": the target bounds the size before byte stuffing)."""

    def __init__(self, path: str, fps: float, size, is_color: bool = True, device: int = 0, quality: int = 75,
                 batch: int = 8, encoder=None, optimize: bool = False, bitrate_kbps=None, quality_range=(10, 95)):
        self.path, self.W, self.H, self.is_color = path, int(size[0]), int(size[1]), bool(is_color)
        self.target_bytes = None if bitrate_kbps is None else bitrate_target_bytes(bitrate_kbps, fps)
        self.quality_range = (int(quality_range[0]), int(quality_range[1]))
        self._rate_encoders = []
        self.n, self._batch, self._fill = 0, max(1, int(batch)), 0
        self.device, self.quality, self.optimize, self._own_encoder = int(device), int(quality), bool(optimize), \
            encoder is None
        if encoder is None:
            from ._native import JpegEncoder
            # (the keyword only when set: an encoder class put in JpegEncoder's place may know nothing of it)
            opt = {"optimize": True} if optimize else {}
            encoder = JpegEncoder(self.W, self.H, self.is_color, quality, self._batch, device, **opt, **self._rate_args())
            if self.target_bytes is not None and hasattr(encoder, "rate_stats"):
                self._rate_encoders.append(encoder)
        self._enc = encoder
        self._shape = (self.H, self.W, 3) if self.is_color else (self.H, self.W)
        # the pending batch; the GPU encoder hands out page-locked memory for it
        self._buf = getattr(encoder, "alloc", lambda s: np.empty(s, np.uint8))((self._batch,) + self._shape)
        self._mux = Mp4Muxer(path, fps, size)

    def isOpened(self) -> bool:
        return self._mux is not None

    def _rate_args(self) -> dict:
        if self.target_bytes is None:
            return {}
        return {"target_bytes": self.target_bytes, "quality_range": self.quality_range}

    def _flush(self) -> None:
        if self._fill:
            n, self._fill = self._fill, 0
            for payload in self._enc.encode(self._buf[:n]):
                self._mux.add_sample(self._enc.header + payload)

    def device_encoder(self, stream=None):
        """A second encoder with this writer's parameters that takes device frames on
        ``stream`` (``_native.JpegEncoder(device_ptrs=True)``) for :meth:`write_samples`;
        ``None`` when the writer's encoder is not this package's or its library has
        no ``dvc_jpeg_encode_stream``. Its table groups are this writer's batches."""
        from . import _native as N
        if not self._own_encoder or not hasattr(self._enc, "encode_stream") or \
                not hasattr(N.lib(), "dvc_jpeg_encode_stream"):
            return None
        enc = N.JpegEncoder(self.W, self.H, self.is_color, self.quality, self._batch, self.device,
                            optimize=self.optimize, device_ptrs=True, stream=stream, **self._rate_args())
        if self.target_bytes is not None:
            self._rate_encoders.append(enc)
        return enc

    def rate_line(self) -> str:
        """What the rate target came to, over this writer's encoders (closed ones included)."""
        st = [e.rate_stats() for e in self._rate_encoders]
        frames, groups = sum(s["frames"] for s in st), sum(s["groups"] for s in st)
        sizes = self._mux.sizes if self._mux is not None else []
        return (f"rate target {self.path}: {self.target_bytes} bytes/frame, quality {self.quality_range[0]}.."
                f"{self.quality_range[1]}: mean quality {sum(s['quality_frames'] for s in st) / max(frames, 1):.1f}, "
                f"{sum(s['missed_groups'] for s in st)} of {groups} groups missed, "
                f"{sum(s['est_bytes'] for s in st) / max(frames, 1):.0f} bytes/frame estimated, "
                f"{sum(sizes) / max(len(sizes), 1):.0f} written")

    def write_samples(self, buffer, offsets) -> None:
        """Frames already encoded (``device_encoder().encode_stream``): complete samples
        back to back in ``buffer``, sample t at ``offsets[t]:offsets[t + 1]``."""
        if self._mux is None or len(offsets) < 2:
            return
        self._flush()
        self._mux.add_samples(buffer, offsets)
        self.n += len(offsets) - 1

    def write(self, frame: np.ndarray) -> None:
        if self._mux is None:
            return
        if frame.shape != self._shape:   # cv2.VideoWriter silently drops mismatched frames
            return
        self._buf[self._fill] = frame
        self._fill += 1
        self.n += 1
        if self._fill >= self._batch:
            self._flush()

    def release(self) -> None:
        if self._mux is None:
            return
        try:
            self._flush()
            if self._rate_encoders:
                logging.info(self.rate_line())
        finally:
            self._mux.close()
            self._mux = None
            if hasattr(self._enc, "close"):
                self._enc.close()


def _child_boxes(buf, start, end):
    """(kind, payload start, box end) of the boxes in buf[start:end]."""
    p = start
    while p + 8 <= end:
        size, kind = struct.unpack_from(">I4s", buf, p)
        head = 8
        if size == 1:
            size, head = struct.unpack_from(">Q", buf, p + 8)[0], 16
        elif size == 0:
            size = end - p
        if size < head or p + size > end:
            return
        yield kind, p + head, p + size
        p += size


def _find(buf, start, end, *kinds):
    for k in kinds:
        hit = next(((a, b) for kind, a, b in _child_boxes(buf, start, end) if kind == k), None)
        if hit is None:
            return None
        start, end = hit
    return start, end


_GPU_DECODE = None


def _gpu_decode_available() -> bool:
    """Whether DVC_MJPEG_DECODE=auto decodes on the GPU: the library loads and a device exists."""
    global _GPU_DECODE
    if _GPU_DECODE is None:
        try:
            import ctypes
            from . import _native as N
            n = ctypes.c_int(0)
            _GPU_DECODE = N.lib().dvc_device_count(ctypes.byref(n)) == 0 and n.value > 0
        except Exception:
            _GPU_DECODE = False
    return _GPU_DECODE


class Mp4MjpegReader:
    """cv2.VideoCapture-like reader of the files :class:`Mp4MjpegWriter` writes
    (``ftyp``, one video track, an ``mp4v`` entry whose ``esds`` says 0x6C, one
    sample per chunk). Samples are demuxed here and decoded ``batch`` at a time
    on the GPU (:class:`_native.JpegDecoder` on ``device``) or one by one by
    Pillow — the same bytes either way: colour to BGR, a single-component
    stream to a 2-D array. ``DVC_MJPEG_DECODE`` chooses: ``gpu``, ``pillow``,
    or ``auto`` (the default): the GPU when the library loads and a device
    exists, Pillow otherwise and for a file whose JPEG streams the GPU decoder
    does not take. A sample that does not decode ends the stream. Without a
    decoder, or on any other file, the reader does not open."""

    def __init__(self, path: str, device: int = 0, batch: int = 8):
        self._fp, self._i, self.samples = None, 0, []
        self._device, self._batch, self._dec, self._ready = int(device), max(1, int(batch)), None, []
        try:
            self._mode = os.environ.get("DVC_MJPEG_DECODE", "auto")
            if self._mode not in ("auto", "gpu", "pillow"):
                raise ValueError(f"DVC_MJPEG_DECODE={self._mode}")
            self._gpu = self._mode == "gpu" or (self._mode == "auto" and _gpu_decode_available())
            try:
                from PIL import Image
                self._Image = Image
            except ImportError:
                self._Image = None
                if not self._gpu:
                    raise
            self._parse(path)
        except Exception:
            if self._fp is not None:
                self._fp.close()
            self._fp = None

    def _parse(self, path):
        fp = open(path, "rb")
        self._fp = fp
        head = fp.read(len(_FTYP) + 16)
        if head[:len(_FTYP)] != _FTYP or head[len(_FTYP) + 4:len(_FTYP) + 8] != b"mdat":
            raise ValueError("not a file of Mp4MjpegWriter")
        size = struct.unpack_from(">I", head, len(_FTYP))[0]
        if size == 1:
            size = struct.unpack_from(">Q", head, len(_FTYP) + 8)[0]
        fp.seek(len(_FTYP) + size)
        moov = fp.read()
        top = _find(moov, 0, len(moov), b"moov", b"trak", b"mdia")
        mdhd = _find(moov, *top, b"mdhd")
        stbl = _find(moov, *top, b"minf", b"stbl")
        timescale = struct.unpack_from(">I", moov, mdhd[0] + 12)[0]
        box = {k: _find(moov, *stbl, k) for k in (b"stsd", b"stts", b"stsc", b"stsz", b"co64")}
        entry = next(_child_boxes(moov, box[b"stsd"][0] + 8, box[b"stsd"][1]))
        if entry[0] != b"mp4v":
            raise ValueError("not an mp4v track")
        self.W, self.H = struct.unpack_from(">HH", moov, entry[1] + 24)
        esds = _find(moov, entry[1] + 78, entry[2], b"esds")
        e = moov[esds[0] + 4:esds[1]]
        if not (e[0] == 0x03 and e[5] == 0x04 and e[7] == 0x6C):
            raise ValueError("not objectTypeIndication 0x6C")
        count, nsamp, delta = struct.unpack_from(">III", moov, box[b"stts"][0] + 4)
        if struct.unpack_from(">IIII", moov, box[b"stsc"][0] + 4) != (1, 1, 1, 1) or count != 1:
            raise ValueError("unexpected sample tables")
        fixed, n = struct.unpack_from(">II", moov, box[b"stsz"][0] + 4)
        sizes = [fixed] * n if fixed else list(struct.unpack_from(">%dI" % n, moov, box[b"stsz"][0] + 12))
        offs = list(struct.unpack_from(">%dQ" % n, moov, box[b"co64"][0] + 8))
        if n != nsamp or len(offs) != n:
            raise ValueError("inconsistent sample tables")
        self.fps = timescale / delta if delta else 0.0
        self.samples = list(zip(offs, sizes))

    def isOpened(self) -> bool:
        return self._fp is not None

    def get(self, prop: int) -> float:
        if self._fp is None:
            return 0.0
        return {CAP_PROP_FPS: self.fps, CAP_PROP_FRAME_WIDTH: float(self.W), CAP_PROP_FRAME_HEIGHT: float(self.H),
                CAP_PROP_FRAME_COUNT: float(len(self.samples))}.get(prop, 0.0)

    def read_sample(self):
        """(ok, the next sample's bytes: one JPEG image). ``read()`` on the GPU takes
        its samples from here a batch ahead: use one of the two on a reader."""
        if self._fp is None or self._i >= len(self.samples):
            return False, None
        off, size = self.samples[self._i]
        self._i += 1
        self._fp.seek(off)
        return True, self._fp.read(size)

    def read_sample_into(self, dst) -> int:
        """The next sample's bytes into ``dst`` (a writable buffer of at least its size,
        ``samples[i][1]``) without a copy in between; the bytes read, -1 at the end."""
        if self._fp is None or self._i >= len(self.samples):
            return -1
        off, size = self.samples[self._i]
        self._i += 1
        self._fp.seek(off)
        return self._fp.readinto(memoryview(dst)[:size])

    def _pillow(self, data):
        import io
        im = self._Image.open(io.BytesIO(data))
        if im.mode == "L":
            return np.asarray(im)
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])

    def _fill(self) -> None:
        """Read ahead and decode the next batch on the GPU into self._ready."""
        from . import _native as N
        samples = []
        while len(samples) < self._batch:
            ok, data = self.read_sample()
            if not ok:
                break
            samples.append(data)
        if not samples:
            return
        if self._dec is None:
            self._dec = N.JpegDecoder(self.W, self.H, self._batch, self._device)
        try:
            self._ready = self._dec.decode(samples)
        except N.DvcError as e:
            if e.code != N.DVC_E_UNSUPPORTED or self._mode != "auto" or self._Image is None:
                raise
            self._gpu = False                      # a JPEG the GPU decoder does not take: this file goes to Pillow
            self._i -= len(samples)

    def read(self):
        if self._gpu:
            if not self._ready:
                self._fill()
            if self._gpu:
                if not self._ready or self._ready[0] is None:   # the end, or a damaged sample: the stream ends here
                    self._ready, self._i = [], len(self.samples)
                    return False, None
                return True, self._ready.pop(0)
        ok, data = self.read_sample()
        if not ok:
            return False, None
        return True, self._pillow(data)

    def release(self) -> None:
        if self._fp is not None:
            self._fp.close()
            self._fp = None
        if self._dec is not None:
            self._dec.close()
            self._dec = None


class _CameraMjpegReader(Mp4MjpegReader):
    """What :class:`AviMjpegReader` and :class:`MjpegStreamReader` share: the
    surface and the decoding of :class:`Mp4MjpegReader` over their own sample
    list, on a camera handle (``JpegDecoder(camera=True)``). A sample that does
    not decode, or whose frame size differs from the first sample's, ends the
    stream."""

    def __init__(self, path: str, device: int = 0, batch: int = 8):
        self._shape = None
        super().__init__(path, device, batch)

    def _fill(self) -> None:
        if self._dec is None:
            from . import _native as N
            self._dec = N.JpegDecoder(self.W, self.H, self._batch, self._device, camera=True)
        super()._fill()

    def read(self):
        try:
            ok, f = super().read()
        except (OSError, SyntaxError, ValueError):   # Pillow on a sample it cannot decode
            ok, f = False, None
        if ok and self._shape is None:
            self._shape = f.shape[:2]
        if not ok or f.shape[:2] != self._shape:
            self._ready, self._i = [], len(self.samples)
            return False, None
        return True, f


def jpeg_image_end(buf, start: int) -> int:
    """The end (one past EOI) of the JPEG image whose SOI is at ``buf[start]``, or
    -1 when it does not parse. The marker segments from SOI to SOS are walked by
    their lengths (an APP1 thumbnail holds SOI and EOI of its own); the entropy
    data is then scanned for the first 0xFF whose next byte is not 0x00 (a stuffed
    byte), 0xFF (fill) or 0xD0..0xD7 (a restart marker): that marker must be EOI."""
    n, p = len(buf), start + 2
    if n < start + 4 or buf[start] != 0xFF or buf[start + 1] != 0xD8:
        return -1
    while True:
        if p + 4 > n or buf[p] != 0xFF:
            return -1
        m = buf[p + 1]
        if m == 0xFF:   # fill byte
            p += 1
            continue
        if m in (0x00, 0x01, 0xD8, 0xD9) or 0xD0 <= m <= 0xD7:
            return -1   # no marker segment: not a header this reader can walk
        ln = (int(buf[p + 2]) << 8) | int(buf[p + 3])
        if ln < 2 or p + 2 + ln > n:
            return -1
        p += 2 + ln
        if m == 0xDA:
            break
    while p < n:
        w = np.frombuffer(buf, np.uint8, min(n - p, 1 << 20), p) if not isinstance(buf, np.ndarray) \
            else buf[p:p + (1 << 20)]
        nxt = w[1:]
        hit = np.flatnonzero((w[:-1] == 0xFF) & (nxt != 0x00) & (nxt != 0xFF) & ((nxt & 0xF8) != 0xD0))
        if len(hit):
            i = p + int(hit[0])
            return i + 2 if buf[i + 1] == 0xD9 else -1
        if len(w) < 2:
            break
        p += len(w) - 1   # the window's last byte starts the next one
    return -1


class MjpegStreamReader(_CameraMjpegReader):
    """cv2.VideoCapture-like reader of a raw Motion-JPEG stream (``.mjpeg``,
    ``.mjpg``: what ``ffmpeg -f mjpeg`` writes and an IP camera's HTTP stream
    carries): JPEG images end to end, split by :func:`jpeg_image_end`. Bytes
    between images are skipped up to the next SOI; an image that does not parse
    (a cut last one) ends the stream. The size is the first image's; the file
    carries no frame rate: ``DVC_MJPEG_FPS`` (default 25) gives it."""

    def _parse(self, path):
        self.fps = float(os.environ.get("DVC_MJPEG_FPS", 25))
        if not self.fps > 0:
            raise ValueError("DVC_MJPEG_FPS")
        self._fp = open(path, "rb")
        mm = np.memmap(path, np.uint8, mode="r")
        p, self.samples = 0, []
        while True:
            p = _next_soi(mm, p)
            if p < 0:
                break
            end = jpeg_image_end(mm, p)
            if end < 0:
                break
            self.samples.append((p, end - p))
            p = end
        if not self.samples:
            raise ValueError("no JPEG image")
        self.W, self.H = _jpeg_size(bytes(mm[self.samples[0][0]:sum(self.samples[0])]))
        del mm


def _next_soi(buf, p: int) -> int:
    """The first SOI marker at or after ``buf[p]`` (outside an image), or -1."""
    while p + 2 <= len(buf):
        w = buf[p:p + (1 << 20)]
        hit = np.flatnonzero((w[:-1] == 0xFF) & (w[1:] == 0xD8))
        if len(hit):
            return p + int(hit[0])
        p += len(w) - 1
    return -1


def _jpeg_size(jpg: bytes):
    """(W, H) of a JPEG image, from its first SOFn segment."""
    p = 2
    while p + 4 <= len(jpg) and jpg[p] == 0xFF:
        m, ln = jpg[p + 1], int.from_bytes(jpg[p + 2:p + 4], "big")
        if m == 0xFF:
            p += 1
            continue
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC) and ln >= 7:
            return int.from_bytes(jpg[p + 7:p + 9], "big"), int.from_bytes(jpg[p + 5:p + 7], "big")
        if m == 0xDA:
            break
        p += 2 + ln
    raise ValueError("no frame header")


class AviMjpegReader(_CameraMjpegReader):
    """cv2.VideoCapture-like reader of a RIFF ``AVI `` file's first ``vids``
    stream whose ``strf`` ``biCompression`` is ``MJPG`` (any case): what capture
    cards, UVC tools and surveillance recorders write. Width and height come from
    ``strf``, the frame rate is ``dwRate / dwScale`` of the stream's ``strh``. The
    samples are the ``##dc`` / ``##db`` chunks of that stream in the ``movi`` list,
    in file order (chunks padded to even sizes, ``LIST rec `` descended, other
    streams and ``JUNK`` skipped, ``idx1`` not needed); zero-length chunks (dropped
    frames) are skipped and not counted. The reader does not open a file without
    such a stream, or one continued in a second ``RIFF AVIX`` segment (OpenDML,
    files past 1 GiB, is out of scope). Interlaced files (two fields a chunk) are
    read as their first field only."""

    def _chunks(self, start, end):
        """(id, list type or None, payload start, payload size) of the chunks in [start, end)."""
        fp, p = self._fp, start
        while p + 8 <= end:
            fp.seek(p)
            cid, size = struct.unpack("<4sI", fp.read(8))
            kind = None
            if cid in (b"RIFF", b"LIST"):
                kind = fp.read(4)
            if p + 8 + size > end:
                size = end - p - 8   # a cut file: what is there
            yield cid, kind, p + 8, size
            p += 8 + size + (size & 1)

    def _parse(self, path):
        self._fp = open(path, "rb")
        flen = os.fstat(self._fp.fileno()).st_size
        top = list(self._chunks(0, flen))
        if not top or top[0][0] != b"RIFF" or top[0][1] != b"AVI ":
            raise ValueError("not a RIFF AVI file")
        if any(c[0] == b"RIFF" for c in top[1:]):
            raise ValueError("a second RIFF segment (OpenDML) is not read")
        _, _, a, n = top[0]
        stream, movi = None, None
        for cid, kind, q, m in self._chunks(a + 4, a + n):
            if cid == b"LIST" and kind == b"hdrl" and stream is None:
                index = 0
                for c2, k2, q2, m2 in self._chunks(q + 4, q + m):
                    if c2 != b"LIST" or k2 != b"strl":
                        continue
                    strh = strf = None
                    for c3, _, q3, m3 in self._chunks(q2 + 4, q2 + m2):
                        if c3 in (b"strh", b"strf"):
                            self._fp.seek(q3)
                            data = self._fp.read(m3)
                            strh, strf = (data, strf) if c3 == b"strh" else (strh, data)
                    if stream is None and strh and strf and len(strh) >= 28 and len(strf) >= 20 and \
                            strh[:4] == b"vids" and strf[16:20].upper() == b"MJPG":
                        scale, rate = struct.unpack_from("<II", strh, 20)
                        w, h = struct.unpack_from("<ii", strf, 4)
                        stream = (index, abs(w), abs(h), rate / scale if scale else 0.0)
                    index += 1
            elif cid == b"LIST" and kind == b"movi" and movi is None:
                movi = (q + 4, q + m)
        if stream is None or movi is None:
            raise ValueError("no MJPG video stream")
        index, self.W, self.H, self.fps = stream
        ids = (b"%02ddc" % index, b"%02ddb" % index)
        self.samples = []

        def walk(lo, hi):
            for cid, kind, q, m in self._chunks(lo, hi):
                if cid == b"LIST" and kind == b"rec ":
                    walk(q + 4, q + m)
                elif cid in ids and m > 0:
                    self.samples.append((q, m))

        walk(*movi)


def video_name(path: str) -> str:
    """<basename without extension> (fd:45, fd:177); a synthetic URI is named WxH."""
    if path.startswith("synthetic://"):
        return urlparse(path).netloc
    return os.path.splitext(os.path.basename(path))[0]


def open_source(path: str):
    """cv2.VideoCapture-like object for ``path`` (isOpened/get/read/release)."""
    if path.endswith(".y4m"):
        return Y4mReader(path, int(os.environ.get("DVC_DEVICE", os.environ.get("LOCAL_RANK", 0))))
    if path.startswith("synthetic://"):
        from .synthetic import SyntheticClip
        u = urlparse(path)
        w, h = (int(v) for v in u.netloc.lower().split("x"))
        q = {k: v[0] for k, v in parse_qs(u.query).items()}
        clip = SyntheticClip(w, h, seed=int(q.get("seed", 0)), noisy=q.get("noisy", "0") in ("1", "true"))
        return _ArraySource(_SyntheticFrames(clip, int(q.get("frames", 100))), float(q.get("fps", 30)))
    if not path.endswith(".npy") and cv2 is None and os.path.isfile(path):
        # a Motion-JPEG .mp4 of this package (DVC_VIDEO_SINK=mjpeg), or a camera's .avi / raw stream
        ext = os.path.splitext(path)[1].lower()
        cls = {".avi": AviMjpegReader, ".mjpeg": MjpegStreamReader, ".mjpg": MjpegStreamReader}.get(ext, Mp4MjpegReader)
        r = cls(path, int(os.environ.get("DVC_DEVICE", os.environ.get("LOCAL_RANK", 0))))
        if r.isOpened():
            return r
    if not path.endswith(".npy") and cv2 is None:
        # an .mp4 this package wrote without OpenCV is the .npy / .y4m stream next to it
        for ext in (".npy", ".y4m"):
            alt = os.path.splitext(path)[0] + ext
            if os.path.exists(alt):
                return open_source(alt)
    if path.endswith(".npy"):
        if not os.path.exists(path):
            return _ArraySource(None, 0)
        arr = np.load(path, mmap_mode="r")
        fps = 30.0
        meta = os.path.splitext(path)[0] + ".json"
        if os.path.exists(meta):
            with open(meta) as f:
                fps = float(json.load(f).get("fps", fps))
        # N x H x W x 3 BGR frames, or N x H x W single-channel frames (mask videos)
        if arr.dtype != np.uint8 or not (arr.ndim == 3 or (arr.ndim == 4 and arr.shape[3] == 3)):
            return _ArraySource(None, 0)
        return _ArraySource(arr, fps)
    if cv2 is not None:
        return cv2.VideoCapture(path)
    return _ArraySource(None, 0)


class NpyStreamWriter:
    """Append frames to an .npy file whose header is rewritten on release."""

    _HDR = 256

    def __init__(self, path: str, fps: float, size, is_color: bool = True):
        self.path = path
        self.fps = float(fps)
        self.W, self.H = int(size[0]), int(size[1])
        self.is_color = is_color
        self.n = 0
        self._fp = open(path, "wb")
        self._write_header()
        with open(os.path.splitext(path)[0] + ".json", "w") as f:
            json.dump({"fps": self.fps, "width": self.W, "height": self.H}, f)

    def _write_header(self):
        shape = (self.n, self.H, self.W, 3) if self.is_color else (self.n, self.H, self.W)
        d = "{'descr': '|u1', 'fortran_order': False, 'shape': %r, }" % (shape,)
        pad = self._HDR - 10 - len(d) - 1
        hdr = b"\x93NUMPY\x01\x00" + struct.pack("<H", self._HDR - 10) + d.encode() + b" " * pad + b"\n"
        self._fp.seek(0)
        self._fp.write(hdr)
        self._fp.seek(0, 2)

    def isOpened(self) -> bool:
        return self._fp is not None

    def write(self, frame: np.ndarray) -> None:
        exp = (self.H, self.W, 3) if self.is_color else (self.H, self.W)
        if frame.shape != exp:  # cv2.VideoWriter silently drops mismatched frames
            return
        self._fp.write(np.ascontiguousarray(frame, dtype=np.uint8).tobytes())
        self.n += 1

    def release(self) -> None:
        if self._fp is not None:
            self._write_header()
            self._fp.close()
            self._fp = None


def bitrate_target_bytes(bitrate_kbps, fps) -> int:
    """Bytes a frame of ``bitrate_kbps`` kbit/s at ``fps`` frames a second."""
    return max(1, int(float(bitrate_kbps) * 125 / float(fps)))


def _sink_rate_args() -> dict:
    """DVC_VIDEO_BITRATE (kbit/s, a positive number) and DVC_VIDEO_QUALITY_RANGE=lo:hi -> Mp4MjpegWriter's keywords."""
    rate, qr = os.environ.get("DVC_VIDEO_BITRATE"), os.environ.get("DVC_VIDEO_QUALITY_RANGE")
    out = {}
    if rate is not None:
        try:
            out["bitrate_kbps"] = float(rate)
        except ValueError:
            out["bitrate_kbps"] = -1.0
        if not 0 < out["bitrate_kbps"] < float("inf"):
            raise ValueError(f"DVC_VIDEO_BITRATE={rate!r}: a positive number of kbit/s")
    if qr is not None:
        lo, sep, hi = qr.partition(":")
        if not (sep and lo.isdigit() and hi.isdigit() and 1 <= int(lo) <= int(hi) <= 100):
            raise ValueError(f"DVC_VIDEO_QUALITY_RANGE={qr!r}: lo:hi with 1 <= lo <= hi <= 100")
        if rate is not None:
            out["quality_range"] = (int(lo), int(hi))
    return out


def open_sink(path: str, fps: float, size, is_color: bool = True):
    """cv2.VideoWriter(path, mp4v, fps, size)-like object."""
    root, ext = os.path.splitext(path)
    if ext == ".y4m" or (ext != ".npy" and cv2 is None and os.environ.get("DVC_VIDEO_SINK", "npy") == "y4m"):
        dev = int(os.environ.get("DVC_DEVICE", os.environ.get("LOCAL_RANK", 0)))
        return Y4mWriter(root + ".y4m", fps, size, is_color, dev)
    if ext != ".npy" and cv2 is None and os.environ.get("DVC_VIDEO_SINK", "npy") == "mjpeg":
        dev = int(os.environ.get("DVC_DEVICE", os.environ.get("LOCAL_RANK", 0)))
        huffman = os.environ.get("DVC_VIDEO_HUFFMAN", "fixed")
        if huffman not in ("fixed", "optimized"):
            raise ValueError(f"DVC_VIDEO_HUFFMAN={huffman!r}: fixed or optimized")
        return Mp4MjpegWriter(path, fps, size, is_color, dev, int(os.environ.get("DVC_VIDEO_QUALITY", 75)),
                              optimize=huffman == "optimized", **_sink_rate_args())
    if cv2 is not None and ext != ".npy":
        fourcc = cv2.VideoWriter_fourcc(*"mp4v")
        return cv2.VideoWriter(path, fourcc, fps, tuple(size), isColor=is_color)
    return NpyStreamWriter(root + ".npy" if ext != ".npy" else path, fps, size, is_color)
