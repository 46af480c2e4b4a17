#!/usr/bin/env python3
"""Generate csrc/jpeg_tables.h: the Motion-JPEG encoder's fixed tables.

    python tools/gen_jpeg_tables.py            # rewrites csrc/jpeg_tables.h
    python tools/gen_jpeg_tables.py --check    # exit 1 if the header is stale

The quantiser base tables are the usual perceptual pair; the two Huffman tables
(one DC, one AC, shared by every component) are built here from the symbol
counts of the package's synthetic clips (fixed seeds, a few qualities, colour
frames and thresholded single-channel masks), every symbol given one extra
count so that all 12 DC and all 162 AC symbols get a code. Code lengths follow
the JPEG standard's procedure (ISO/IEC 10918-1 Annex K.2): a Huffman tree with
one reserved pseudo-symbol, so that no code is all ones, and the length
adjustment to at most 16 bits. CPU only (numpy); DESIGN.md "Motion-JPEG
stream" is the normative text of the arithmetic restated here.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "dynamic-video-compression-surveillance_amd", "csrc", "jpeg_tables.h")

BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
QUALITIES = (30, 50, 75, 90, 100)


def zigzag():
    """Natural index of zigzag position k."""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return order


def dct_matrix():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    a = np.where(k == 0, np.sqrt(1 / 8), np.sqrt(2 / 8))
    return np.rint(8192 * a * np.cos((2 * n + 1) * k * np.pi / 16)).astype(np.int64)


def quant_table(base, q):
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.asarray(base, np.int64) * s + 50) // 100, 1, 255)


def _blocks(plane):
    """(H, W) plane with H, W multiples of 8 -> (H/8, W/8, 8, 8)."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)


def _levels(plane, Q):
    M = dct_matrix()
    x = _blocks(plane.astype(np.int64) - 128)
    R = (np.einsum("kn,abyn->abyk", M, x) + 512) >> 10
    F = (np.einsum("vy,abyk->abvk", M, R) + 32768) >> 16
    q = Q.reshape(8, 8)
    lv = np.sign(F) * ((np.abs(F) + q // 2) // q)
    lv = lv.reshape(*lv.shape[:2], 64)[..., zigzag()]
    lv[..., 1:] = np.clip(lv[..., 1:], -1023, 1023)
    return lv


def _pad(plane, m):
    h, w = plane.shape
    return np.pad(plane, ((0, -h % m), (0, -w % m)), mode="edge")


def _count(seq, dc, ac):
    """seq: the (n, 64) zigzag levels of one component in one restart segment."""
    pred = 0
    for b in seq:
        d = int(np.clip(int(b[0]) - pred, -2047, 2047))
        pred = int(b[0])
        dc[abs(d).bit_length()] += 1
        nz = np.nonzero(b[1:])[0] + 1
        prev = 0
        for k in nz:
            run = int(k) - prev - 1
            ac[0xF0] += run >> 4
            ac[((run & 15) << 4) | abs(int(b[k])).bit_length()] += 1
            prev = int(k)
        if prev != 63:
            ac[0x00] += 1


def count_frame(frame, quality, dc, ac):
    if frame.ndim == 2:
        lv = _levels(_pad(frame, 8), quant_table(BASE_LUMA, quality))
        for row in lv:
            _count(row, dc, ac)
        return
    b, g, r = (frame[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    y, cb, cr = (_pad(p, 16) for p in (y, cb, cr))
    cb, cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (cb, cr))
    ly = _levels(y, quant_table(BASE_LUMA, quality))
    lc = [_levels(p, quant_table(BASE_CHROMA, quality)) for p in (cb, cr)]
    for m in range(ly.shape[0] // 2):
        ys = np.stack([ly[2 * m, 0::2], ly[2 * m, 1::2], ly[2 * m + 1, 0::2], ly[2 * m + 1, 1::2]], 1)
        _count(ys.reshape(-1, 64), dc, ac)
        _count(lc[0][m], dc, ac)
        _count(lc[1][m], dc, ac)


def symbol_counts():
    from dvc_amd.synthetic import SyntheticClip
    dc, ac = np.zeros(12, np.int64), np.zeros(256, np.int64)
    for seed, noisy in ((1, False), (2, True)):
        clip = SyntheticClip(320, 192, seed=seed, noisy=noisy)
        frames = [clip.frame(t) for t in (0, 5)]
        for q in QUALITIES:
            for f in frames:
                count_frame(f, q, dc, ac)
        # mask videos: the pixels that moved between the two frames, {0, 255}
        mask = ((frames[0] != frames[1]).any(-1) * 255).astype(np.uint8)
        for q in QUALITIES:
            count_frame(mask, q, dc, ac)
    return dc, ac


def code_lengths(freq_by_symbol):
    """ISO/IEC 10918-1 K.2: {symbol: count} -> (bits[1..16], symbols in code order)."""
    freq = [0] * 257
    for s, c in freq_by_symbol.items():
        freq[s] = int(c) + 1          # every symbol present
    freq[256] = 1                      # reserved: takes the all-ones code
    size, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        for i in range(257):
            if freq[i] and (c1 < 0 or freq[i] <= freq[c1]):
                c1 = i
        for i in range(257):
            if freq[i] and i != c1 and (c2 < 0 or freq[i] <= freq[c2]):
                c2 = i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        for c, tail in ((c1, c2), (c2, None)):
            size[c] += 1
            while others[c] >= 0:
                c = others[c]
                size[c] += 1
            if tail is not None:
                others[c] = tail
    assert max(size) <= 32
    bits = [0] * 33
    for s in size:
        if s:
            bits[s] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                       # the reserved symbol leaves
    vals = [s for ln in range(1, 33) for s in range(256) if size[s] == ln]
    assert sum(bits[1:17]) == len(vals)
    return bits[1:17], vals


def canonical(bits, vals):
    """{symbol: (code, length)} as a decoder derives it from BITS / HUFFVAL."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def _rows(name, ctype, vals, per=16):
    body = ",\n".join("    " + ", ".join(str(v) for v in vals[i:i + per]) for i in range(0, len(vals), per))
    return f"static const {ctype} {name}[{len(vals)}] = {{\n{body}}};\n"


def render():
    dc, ac = symbol_counts()
    ac_syms = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
    dcb, dcv = code_lengths({s: dc[s] for s in range(12)})
    acb, acv = code_lengths({s: ac[s] for s in ac_syms})
    for bits, vals, n in ((dcb, dcv, 12), (acb, acv, 162)):
        codes = canonical(bits, vals)
        assert len(codes) == n and all(c != (1 << ln) - 1 for c, ln in codes.values())
    out = ["// jpeg_tables.h — the Motion-JPEG encoder's fixed tables (DESIGN.md \"Motion-JPEG stream\").\n"
           "// GENERATED by tools/gen_jpeg_tables.py from the synthetic clips' symbol counts; do not edit.\n"
           "#pragma once\n#include <stdint.h>\n\nnamespace dvc_jpeg_tab {\n\n"
           "// quantiser base tables, natural (row-major) order; scaled by quality at create\n",
           _rows("kBaseLuma", "uint8_t", BASE_LUMA), _rows("kBaseChroma", "uint8_t", BASE_CHROMA),
           "\n// natural index of zigzag position k\n", _rows("kZigzag", "uint8_t", zigzag()),
           "\n// DHT contents: codes per length 1..16, then the symbols in code order\n",
           _rows("kDcBits", "uint8_t", dcb), _rows("kDcVals", "uint8_t", dcv),
           _rows("kAcBits", "uint8_t", acb), _rows("kAcVals", "uint8_t", acv),
           "\n}  // namespace dvc_jpeg_tab\n"]
    return "".join(out)


def main(argv):
    text = render()
    if "--check" in argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("jpeg_tables.h is", "current" if same else "STALE")
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", HEADER)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
