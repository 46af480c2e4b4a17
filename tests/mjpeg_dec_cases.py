"""The Motion-JPEG decoder's test streams, shared by tests/test_mjpeg_decode.py
(CPU: the reference decoder against Pillow, the header parser, the host safety
program) and tests/test_mjpeg_decode_gpu.py (the GPU decoder byte for byte).

(a) every frame of tests/mjpeg_cases.ALL as tests/mjpeg_ref.encode writes it
    (the project's own stream layout), colour and the single-component variants;
(b) Pillow-encoded streams: sizes below one MCU and odd sizes, no restart
    interval, restart intervals of rows and of 1 and 7 MCUs, optimised Huffman
    tables, extreme quantisers;
(c) SIZE_CASES, for tests/test_mjpeg_sizes.py and tests/test_mjpeg_sizes_gpu.py: Pillow
    streams with hundreds of one-block segments (batches of up to 149 different frames)
    and a 1920x1080 one, whose expected frame is Pillow's own decode.
Each stream and each expected frame is computed once.
"""
import functools
import io

import numpy as np

from tests import mjpeg_cases as C
from tests import mjpeg_dec_ref as R


def _noise(w, h, seed, gray):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return a[..., 0] if gray else a


def _smooth(w, h, seed, gray):
    y, x = np.indices((h, w))
    base = (110 + 70 * np.sin((x + 3 * seed) / 5.0) + 60 * np.cos(y / 9.0))[:, :, None] + np.array([0, 25, -30])
    a = np.clip(base + np.random.default_rng(seed).integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)
    return a[..., 1] if gray else a


# name -> (W, H, content, gray, Pillow save options)
PIL_CASES = {}
for _w, _h in [(1, 1), (2, 5), (3, 5), (4, 16), (5, 3), (33, 17), (70, 37), (130, 50)]:
    PIL_CASES[f"pil{_w}x{_h}"] = (_w, _h, _noise, False, dict(quality=75))
    PIL_CASES[f"pil{_w}x{_h}_gray"] = (_w, _h, _noise, True, dict(quality=75))
PIL_CASES.update({
    "pil70x37_rows1": (70, 37, _noise, False, dict(quality=90, restart_marker_rows=1)),
    "pil70x37_blocks1": (70, 37, _noise, False, dict(quality=75, restart_marker_blocks=1)),
    "pil70x37_blocks7": (70, 37, _noise, False, dict(quality=75, restart_marker_blocks=7)),   # segments straddle MCU rows
    "pil70x37_blocks7_gray": (70, 37, _noise, True, dict(quality=75, restart_marker_blocks=7)),
    "pil70x37_q90": (70, 37, _noise, False, dict(quality=90)),
    "pil70x37_q100_smooth": (70, 37, _smooth, False, dict(quality=100)),
    "pil130x50_q20_smooth_rows1": (130, 50, _smooth, False, dict(quality=20, restart_marker_rows=1)),
    "pil33x17_opt": (33, 17, _noise, False, dict(quality=75, optimize=True)),                 # four custom DHT tables
    "pil70x37_opt_smooth": (70, 37, _smooth, False, dict(quality=90, optimize=True)),
    "pil33x17_opt_gray": (33, 17, _smooth, True, dict(quality=75, optimize=True)),
    "pil33x17_q1_q255": (33, 17, _noise, False, dict(qtables=[[1] * 64, [255] * 64])),
    "pil70x37_q255_q1_smooth": (70, 37, _smooth, False, dict(qtables=[[255] * 64, [1] * 64])),
    "pil4x16_rows1": (4, 16, _noise, False, dict(quality=90, restart_marker_rows=1)),
})

def _noisy_smooth(w, h, seed, gray):
    y, x = np.indices((h, w))
    base = (110 + 70 * np.sin((x + 3 * seed) / 37.0) + 60 * np.cos(y / 53.0))[:, :, None] + np.array([0, 25, -30])
    a = np.clip(base + np.random.default_rng(seed).integers(-24, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    return a[..., 1] if gray else a


# The sizes at which the decoder's loops and index expressions go past their first trip
# (tests/test_mjpeg_sizes.py asserts each property from the bytes; tests/test_mjpeg_sizes_gpu.py
# runs the kernels). Same layout as PIL_CASES; kept out of ids(): the parametrised tests do not grow.
SIZE_CASES = {
    # 17 x 13 = 221 segments of one block; 32 chunks of 263 (q75) and 462 (q95) bytes: two windows a
    # chunk, about 7 markers a chunk
    "pil136x104_gray_b1": (136, 104, _noise, True, dict(quality=75, restart_marker_blocks=1)),
    "pil136x104_gray_b1_q95": (136, 104, _noise, True, dict(quality=95, restart_marker_blocks=1)),
    "pil136x104_b1": (136, 104, _noise, False, dict(quality=75, restart_marker_blocks=1)),      # 9 x 7 = 63 segments
    "pil1920x1080_rows1": (1920, 1080, _noisy_smooth, False, dict(quality=75, restart_marker_rows=1)),
}
_EVERY = {**PIL_CASES, **SIZE_CASES}

REF_CASES = [(name, False) for name in C.ALL] + [(name, True) for name in (C.GRAY_CASE, "wide1120x32", "tiny5x3")]


def ids():
    """Every case: ("ref", name, gray) or ("pil", name, None)."""
    return [("ref", n, g) for n, g in REF_CASES] + [("pil", n, None) for n in PIL_CASES]


@functools.lru_cache(maxsize=None)
def stream(kind, name, gray=None, variant=0):
    """The complete JPEG image of a case. variant 1, 2: other frames of the same header (for batches)."""
    if kind == "ref":
        return C.reference(name, variant % 2, bool(gray))["jpeg"]
    from PIL import Image
    w, h, content, g, opts = _EVERY[name]
    a = content(w, h, 100 + 7 * variant + w, g)      # a different image for every variant
    buf = io.BytesIO()
    Image.fromarray(a if g else a[..., ::-1].copy()).save(buf, "JPEG", **dict(opts, subsampling=2) if not g else opts)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def expected(kind, name, gray=None, variant=0):
    """The reference decoder's frame (read-only)."""
    f = R.decode(stream(kind, name, gray, variant))
    f.setflags(write=False)
    return f


def pillow(jpg):
    from PIL import Image
    im = Image.open(io.BytesIO(jpg))
    if im.mode == "L":
        return np.asarray(im)
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def header_len(jpg):
    return R.parse(jpg)["start"]


# ---- damaged data: three 70x37 frames of the project's layout (3 restart segments), the middle one damaged ----
DAMAGE_CASE = "noise70x37_q90"


def _markers(data):
    return [i for i in range(len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


def _truncated(d):
    m = _markers(d)
    return d[:m[-1] + 2 + (len(d) - m[-1] - 2) // 2]        # the last segment cut in half: the right marker count


def _no_rst(d):
    m = _markers(d)
    return d[:m[0]] + d[m[0] + 2:]


def _ff00(d):
    m = _markers(d)
    return d[:m[0] + 2] + b"\xff\x00" * ((m[1] - m[0] - 2) // 2) + d[m[1]:]


DAMAGE = {"truncated": _truncated, "no_rst": _no_rst, "ff00_run": _ff00, "one_byte": lambda d: d[:1]}


@functools.lru_cache(maxsize=None)
def damaged(kind, case=("ref", DAMAGE_CASE, False), n=3, frame=1, also=()):
    """(header, [entropy data of the n frames, variants 0 .. n - 1, of `case`]) with `frame`
    damaged by DAMAGE[kind]; `also`: further (frame, kind) pairs. The default is three 70x37
    frames of the project's layout (variants 0, 1, 0), the middle one damaged."""
    jp = [stream(*case, v) for v in range(n)]
    hl = header_len(jp[0])
    assert all(j[:hl] == jp[0][:hl] for j in jp)
    data = [j[hl:] for j in jp]
    for t, k in ((frame, kind),) + tuple(also):
        data[t] = DAMAGE[k](data[t])
    return jp[0][:hl], data


@functools.lru_cache(maxsize=None)
def pillow_frame(name, variant=0):
    """Pillow's own decode of a Pillow-encoded case (read-only): the expected frame."""
    f = pillow(stream("pil", name, None, variant))
    f.setflags(write=False)
    return f


def rst_offsets(data):
    """Offsets of the restart markers' 0xFF bytes in a frame's entropy data."""
    return _markers(data)


def mcu_rows_jpeg(jpg, lo, hi):
    """A stream whose restart segments are MCU rows (DRI = MCUs a row) -> the complete JPEG image
    of its MCU rows lo .. hi alone: the same header with the frame height patched, and those
    segments. (The RSTn numbering no longer starts at 0: a decoder that checks it refuses this.)"""
    hl = header_len(jpg)
    hdr, data = bytearray(jpg[:hl]), jpg[hl:]
    sof = 2
    while hdr[sof + 1] != 0xC0:                                    # marker segments from SOI to SOF0
        sof += 2 + int.from_bytes(hdr[sof + 2:sof + 4], "big")
    H, nc = int.from_bytes(hdr[sof + 5:sof + 7], "big"), hdr[sof + 9]
    m = 16 if nc == 3 else 8
    hdr[sof + 5:sof + 7] = (min(H, (hi + 1) * m) - lo * m).to_bytes(2, "big")
    cuts = [0] + [p + 2 for p in _markers(data)] + [len(data)]     # the last segment ends with EOI
    assert len(cuts) - 1 == -(-H // m), "one segment an MCU row"
    body = data[cuts[lo]:cuts[hi + 1]]
    return bytes(hdr) + body[:-2] + b"\xff\xd9"
