"""Independent restatement of the Motion-JPEG stream with optimised Huffman
tables (DESIGN.md "Motion-JPEG stream", "Optimised Huffman tables"), built on
``tests/mjpeg_ref.py``: the quantised levels of every frame of a table group
come from ``mjpeg_ref.encode``; the symbols are counted per table class here,
the tables are built by this file's own ISO/IEC 10918-1 K.2 (linked lists, as
the standard's figure K.1 draws it, and any code depth), the short header is
the fixed header without its DHT and SOS segments, and every frame is coded
again with ``mjpeg_ref._code_block``. Nothing here shares code with the library.
"""
import functools

from tests import mjpeg_ref

AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
TABLE_IDS = (0x00, 0x10, 0x01, 0x11)       # rows of counts[4][256]: DC class 0, AC class 0, DC class 1, AC class 1
PREFIX_MAX = 2 + 2 + 2 * (17 + 12) + 2 * (17 + 162) + 14


def _count_block(zz, pred, dc, ac):
    d = max(-2047, min(2047, zz[0] - pred))
    dc[abs(d).bit_length()] += 1
    run = 0
    for v in zz[1:]:
        if v == 0:
            run += 1
            continue
        ac[0xF0] += run // 16                          # one count per ZRL emitted
        ac[((run % 16) << 4) | abs(v).bit_length()] += 1
        run = 0
    if run:
        ac[0x00] += 1
    return zz[0]


def count_symbols(levels_of_frames):
    """[mjpeg_ref.encode(...)["levels"] of each frame] -> counts[4][256] (Python ints)."""
    counts = [[0] * 256 for _ in range(4)]
    for levels in levels_of_frames:
        gray = len(levels) == 1
        rows, cols = levels[0].shape[:2] if gray else levels[1].shape[:2]
        for my in range(rows):
            pred = [0, 0, 0]
            for mx in range(cols):
                where = [(0, my, mx)] if gray else \
                    [(0, 2 * my + dy, 2 * mx + dx) for dy in (0, 1) for dx in (0, 1)] + [(1, my, mx), (2, my, mx)]
                for c, by, bx in where:
                    zz = [int(levels[c][by, bx].reshape(64)[i]) for i in mjpeg_ref.ZIGZAG]
                    cls = 0 if c == 0 else 1
                    pred[c] = _count_block(zz, pred[c], counts[2 * cls], counts[2 * cls + 1])
    return counts


def code_lengths(counts):
    """K.2 on counts[0..255] (no extra count; the reserved symbol 256 has 1):
    (BITS[1..16], HUFFVAL, code size of every symbol before the limit to 16)."""
    freq = [int(c) for c in counts] + [1]
    assert len(freq) == 257 and min(freq) >= 0
    size, nxt = [0] * 257, [None] * 257
    while True:
        live = [i for i in range(257) if freq[i]]
        if len(live) < 2:
            break
        c1 = min(live, key=lambda i: (freq[i], -i))        # least, the largest index among equals
        c2 = min((i for i in live if i != c1), key=lambda i: (freq[i], -i))
        freq[c1] += freq[c2]
        freq[c2] = 0
        i = c1
        while True:
            size[i] += 1
            if nxt[i] is None:
                break
            i = nxt[i]
        nxt[i] = c2
        i = c2
        while i is not None:
            size[i] += 1
            i = nxt[i]
    deepest = max(size)
    bits = [0] * (max(deepest, 16) + 1)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(deepest, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    if sum(bits) == 0:
        return [0] * 16, [], size
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = sorted((s for s in range(256) if size[s]), key=lambda s: (size[s], s))
    assert sum(bits[1:17]) == len(vals) and not any(bits[17:])
    return bits[1:17], vals, size


def codes(bits, vals):
    """{symbol: (code, length)} as a decoder derives it."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def dht_segment(counts):
    """counts[4][256] -> the one DHT segment: tables 00, 10, 01, 11; one without counts is omitted."""
    body = b""
    for row, tid in zip(counts, TABLE_IDS):
        bits, vals, _ = code_lengths(row)
        if vals:
            body += bytes([tid]) + bytes(bits) + bytes(vals)
    return b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body


def sos_segment(nc):
    sel = b"".join(bytes([c + 1, 0x11 if c else 0x00]) for c in range(nc))
    return b"\xff\xda" + (6 + 2 * nc).to_bytes(2, "big") + bytes([nc]) + sel + b"\x00\x3f\x00"


def short_header(hdr):
    """The fixed-table header without its DHT and SOS segments."""
    assert hdr[:2] == b"\xff\xd8"
    out, p = bytearray(hdr[:2]), 2
    while p < len(hdr):
        assert hdr[p] == 0xFF
        ln = int.from_bytes(hdr[p + 2:p + 4], "big")
        if hdr[p + 1] not in (0xC4, 0xDA):
            out += hdr[p:p + 2 + ln]
        p += 2 + ln
    assert p == len(hdr)
    return bytes(out)


def _recode(ref, tabs):
    """One frame's entropy data from the reference's levels with tabs[class] = (dc, ac)."""
    levels, info = ref["levels"], ref["info"]
    gray = len(levels) == 1
    rows, cols = levels[0].shape[:2] if gray else levels[1].shape[:2]
    out = bytearray()
    for my in range(rows):
        bits, pred = mjpeg_ref._Bits(), [0, 0, 0]
        for mx in range(cols):
            where = [(0, my, mx)] if gray else \
                [(0, 2 * my + dy, 2 * mx + dx) for dy in (0, 1) for dx in (0, 1)] + [(1, my, mx), (2, my, mx)]
            for c, by, bx in where:
                pred[c] = mjpeg_ref._code_block(bits, levels[c][by, bx], pred[c], *tabs[0 if c == 0 else 1])
        out += bits.segment()[0]
        out += bytes([0xFF, 0xD0 + my % 8]) if my < rows - 1 else b"\xff\xd9"
    assert info["dri"] == cols
    return bytes(out)


def encode_group(refs):
    """refs: mjpeg_ref.encode(...) of every frame of one table group ->
    dict(header, prefix, frames = [prefix + entropy data + EOI], counts)."""
    counts = count_symbols([r["levels"] for r in refs])
    nc = len(refs[0]["levels"])
    prefix = dht_segment(counts) + sos_segment(nc)
    assert len(prefix) <= PREFIX_MAX
    tabs = []
    for cls in (0, 1):
        t = []
        for row in (counts[2 * cls], counts[2 * cls + 1]):
            bits, vals, _ = code_lengths(row)
            t.append(codes(bits, vals))
        tabs.append(t)
    return {"header": short_header(refs[0]["header"]), "prefix": prefix, "counts": counts,
            "frames": [prefix + _recode(r, tabs) for r in refs]}


def encode(refs, max_batch):
    """A call's frames in table groups of max_batch, in order -> (short header, [frame bytes])."""
    out = []
    for t in range(0, len(refs), max_batch):
        out += encode_group(refs[t:t + max_batch])["frames"]
    return short_header(refs[0]["header"]), out


@functools.lru_cache(maxsize=None)
def case_group(name, variants=(0,), gray=False):
    """encode_group of frames of tests/mjpeg_cases.py (computed once)."""
    from tests import mjpeg_cases
    return encode_group([mjpeg_cases.reference(name, v, gray) for v in variants])


@functools.lru_cache(maxsize=None)
def clip_refs(width, height, seed, n, quality):
    """mjpeg_ref.encode of the first n frames of a synthetic clip."""
    from dvc_amd.synthetic import SyntheticClip
    clip = SyntheticClip(width, height, seed=seed)
    return tuple(mjpeg_ref.encode(clip.frame(t), quality) for t in range(n))


def file_bytes(header, frames):
    """What a file holds of these frames: the header in front of each."""
    return sum(len(header) + len(f) for f in frames)


# ---- count vectors for the table builder alone ------------------------------------------------
def _fib(n):
    a, b, out = 1, 1, []
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def count_vectors():
    """name -> (components, counts[4][256]): what tools/jpeg_huff_host_check.cc and
    dvc_jpeg_opt_tables are run on. Row 1 (AC class 0) carries the case; the DC
    rows hold a plain table so that the segment is a usable one."""
    def base():
        c = [[0] * 256 for _ in range(4)]
        c[0][0] = 5
        return c
    out = {}
    c = base(); c[1][0x00] = 9; out["one_symbol"] = (1, c)
    c = base(); c[1][0x00] = 7; c[1][0x01] = 7; out["two_equal"] = (1, c)
    c = base()
    for s in AC_SYMBOLS:
        c[1][s] = 3
    out["all162_equal"] = (1, c)
    c = base()
    for s, f in zip(AC_SYMBOLS[::-1], _fib(20)):      # the least counts on the largest symbols: with the
        c[1][s] = f                                   # tie-breaks the reserved symbol joins the chain, 20 deep
    out["fib20"] = (1, c)
    c = base()
    for s, f in zip(AC_SYMBOLS[::-1], _fib(40)):
        c[1][s] = f
    for s, f in zip(AC_SYMBOLS, _fib(40)):            # colour: class 1 the same counts the other way round, which
        c[3][s] = f                                   # the reserved symbol's tie pairs up into a shallower tree
    c[2][3] = 2
    out["fib40"] = (3, c)
    c = base()
    for k, s in enumerate(AC_SYMBOLS[:32]):           # powers of two, each twice: a tie at every merge
        c[1][s] = 1 << (k // 2)
    for s in range(12):
        c[0][s] = 1 + s % 2
        c[2][s] = 4
    c[3][0x00] = 1
    out["ties"] = (3, c)
    return out
