"""The camera stream set's test streams and containers, shared by
tests/test_mjpeg_camera.py (CPU) and tests/test_mjpeg_camera_gpu.py.

Streams are Pillow's (libjpeg-turbo), in the three samplings, with and without
restart intervals; ``strip_dht`` removes every DHT segment, as an AVI MJPG frame
has none. The containers are built here from the formats' layouts: a raw
concatenated stream, and a RIFF AVI (no AVI written by another program is at
hand). Each stream and each expected frame is computed once.
"""
import functools
import io
import struct

import numpy as np

from tests import mjpeg_dec_cases as D
from tests import mjpeg_dec_ref as R

SUB = {"444": 0, "422": 1, "420": 2}           # Pillow's subsampling argument
MCU = {"444": (8, 8), "422": (16, 8), "420": (16, 16)}

GRID_SIZES = [(1, 1), (2, 3), (3, 2), (4, 4), (5, 1), (5, 9), (8, 8), (9, 17), (16, 8), (17, 9), (33, 7), (40, 24),
              (47, 31), (130, 50)]
# (content, quality, restart, optimised tables): every restart kind, quality and content of the grid
GRID_COMBOS = [("noise", 85, "none", False), ("gradient", 5, "dri1", False), ("flat", 100, "dri7", True),
               ("noise", 100, "row", False), ("gradient", 85, "dri7", True), ("flat", 5, "none", False)]


def _content(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":
        y, x = np.indices((h, w))
        a = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y + 13 * seed) * 5) % 256], -1)
        return a.astype(np.uint8)
    cells = rng.integers(0, 256, (-(-h // 4), -(-w // 4), 3), dtype=np.uint8)      # 4x4 flats
    return np.ascontiguousarray(np.repeat(np.repeat(cells, 4, 0), 4, 1)[:h, :w])


def _restart(kind):
    return {"none": {}, "dri1": dict(restart_marker_blocks=1), "dri7": dict(restart_marker_blocks=7),
            "row": dict(restart_marker_rows=1)}[kind]


@functools.lru_cache(maxsize=None)
def stream(w, h, sub, restart="none", variant=0, quality=75, content="noise", optimize=False):
    """A complete Pillow JPEG image, ``sub`` "420" | "422" | "444". variant: another image, the same header."""
    from PIL import Image
    a = _content(content, w, h, 1000 + 31 * variant + w + 7 * h)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling=SUB[sub], optimize=optimize, **_restart(restart))
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def gray_stream(w, h, variant=0):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(_content("noise", w, h, 77 + variant)[..., 0].copy()).save(buf, "JPEG", quality=75)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def rgb_stream(w=70, h=37):
    """An RGB-coded JPEG: an Adobe APP14 segment with transform 0, component ids R, G, B, no JFIF."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(_content("noise", w, h, 5)).save(buf, "JPEG", quality=75, keep_rgb=True)
    return buf.getvalue()


def segments(jpg):
    """[(marker, offset, end)] of the marker segments SOI .. SOS of a stream."""
    out, p = [], 2
    while True:
        m, ln = jpg[p + 1], int.from_bytes(jpg[p + 2:p + 4], "big")
        out.append((m, p, p + 2 + ln))
        p += 2 + ln
        if m == 0xDA:
            return out


def strip_dht(jpg):
    """The stream without its DHT (0xC4) segments: what an AVI MJPG frame looks like."""
    keep, p = bytearray(jpg[:2]), 2
    for m, a, b in segments(jpg):
        if m != 0xC4:
            keep += jpg[a:b]
        p = b
    return bytes(keep) + jpg[p:]


def dht_segments(jpg):
    """{(class, slot): (BITS, HUFFVAL)} of a stream's DHT segments."""
    out = {}
    for m, a, b in segments(jpg):
        body = jpg[a + 4:b]
        while m == 0xC4 and body:
            n = sum(body[1:17])
            out[(body[0] >> 4, body[0] & 15)] = (bytes(body[1:17]), bytes(body[17:17 + n]))
            body = body[17 + n:]
    return out


def patch_sampling(jpg, hv):
    """The stream with its first component's sampling byte replaced (a header for the parser only)."""
    for m, a, b in segments(jpg):
        if m == 0xC0:
            out = bytearray(jpg)
            out[a + 4 + 7] = hv
            return bytes(out)
    raise ValueError("no SOF0")


@functools.lru_cache(maxsize=None)
def pillow(jpg):
    f = D.pillow(jpg)
    f.setflags(write=False)
    return f


def header_len(jpg):
    return R.parse(jpg)["start"]


# ---- damaged data: cut short, one restart marker removed (D.DAMAGE's functions on the entropy data) -------------
DAMAGE = ("truncated", "no_rst")


@functools.lru_cache(maxsize=None)
def damaged(sub, kind, w=70, h=37):
    """(header, [entropy data of three frames, one MCU row a segment], the middle one damaged)."""
    jp = [stream(w, h, sub, "row", v) for v in (0, 1, 2)]
    hl = header_len(jp[0])
    assert all(j[:hl] == jp[0][:hl] for j in jp)
    data = [j[hl:] for j in jp]
    data[1] = D.DAMAGE[kind](data[1])
    return jp[0][:hl], data


# ---- containers ------------------------------------------------------------------------------------------------
def app1_with_thumbnail():
    """An APP1 segment whose payload holds a whole small JPEG: SOI and EOI inside a marker segment."""
    body = b"Exif\0\0" + stream(8, 8, "420")
    assert b"\xff\xd8" in body and b"\xff\xd9" in body
    return b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body


def with_app1(jpg):
    return jpg[:2] + app1_with_thumbnail() + jpg[2:]


def _chunk(cid, data):
    return cid + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def _list(kind, *parts):
    return _chunk(b"LIST", kind + b"".join(parts))


def avi(samples, w, h, rate=30000, scale=1001, fourcc=b"mjpg", audio=True, rec=True, junk=True, empty=True, avix=False):
    """A RIFF AVI from the format's layout: stream 0 audio (when ``audio``), then the MJPG video
    stream; a JUNK chunk; in ``movi`` the video chunks in order with audio chunks between them, a
    zero-length video chunk after the first sample, the third and fourth samples inside a
    ``LIST rec ``; no ``idx1``. Odd-sized chunks are padded."""
    vid = 1 if audio else 0
    avih = struct.pack("<14I", 1000000 * scale // rate, 0, 0, 0, len(samples), 0, 1 + vid, 0, w, h, 0, 0, 0, 0)
    strh_v = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", fourcc, 0, 0, 0, 0, scale, rate, 0, len(samples), 0, 0, 0, 0, 0, w, h)
    strf_v = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, fourcc, 3 * w * h, 0, 0, 0, 0)
    strls = [_list(b"strl", _chunk(b"strh", strh_v), _chunk(b"strf", strf_v))]
    if audio:
        strh_a = struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, 8000, 0, 0, 0, 0, 1, 0, 0, 0, 0)
        strf_a = struct.pack("<HHIIHH", 1, 1, 8000, 8000, 1, 8)
        strls.insert(0, _list(b"strl", _chunk(b"strh", strh_a), _chunk(b"strf", strf_a)))
    vid_id, aud_id = b"%02ddc" % vid, b"00wb"
    noise = b"\xff\xd8\xff\xd9" * 5 + b"\x80"          # audio bytes that look like JPEG markers, odd-sized
    body, pending = [], []
    for i, s in enumerate(samples):
        part = [_chunk(vid_id if i % 2 == 0 else b"%02ddb" % vid, s)]
        if audio:
            part.append(_chunk(aud_id, noise))
        if i == 0 and empty:
            part.append(_chunk(vid_id, b""))           # a dropped frame
        if rec and i in (2, 3):
            pending += part
            if i == 3 or i == len(samples) - 1:
                body.append(_list(b"rec ", *pending))
                pending = []
        else:
            body += part
    body += [_list(b"rec ", *pending)] if pending else []
    parts = [_list(b"hdrl", _chunk(b"avih", avih), *strls)]
    if junk:
        parts.append(_chunk(b"JUNK", b"\0" * 37))
    parts.append(_list(b"movi", *body))
    out = _chunk(b"RIFF", b"AVI " + b"".join(parts))
    if avix:
        out += _chunk(b"RIFF", b"AVIX" + _list(b"movi", _chunk(vid_id, samples[0])))
    return out
