"""Independent numpy restatement of DESIGN.md "Motion-JPEG decoder", in the
manner of ``tests/mjpeg_ref.py``: nothing here shares code or tables with the
library. ``decode(jpeg_bytes)`` returns what Pillow returns for a baseline
stream of one component or of three with 4:2:0 sampling: (H, W, 3) BGR or
(H, W) uint8. ``Damaged`` is raised where the library reports a damaged frame.
"""
import numpy as np


class Damaged(ValueError):
    pass


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return order          # natural index of zigzag position k


ZZ = _zigzag()


def parse(jpg):
    """SOI..SOS -> dict(W, H, comps [(id, h, v, tq)], q {id: natural int64[64]}, huff {(cls, id): {(len, code): sym}},
    dri, scan [(td, ta)], start)."""
    if jpg[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    o = {"q": {}, "huff": {}, "dri": 0}
    p = 2
    while True:
        if jpg[p] != 0xFF:
            raise ValueError("marker expected")
        m = jpg[p + 1]
        ln = int.from_bytes(jpg[p + 2:p + 4], "big")
        b = jpg[p + 4:p + 2 + ln]
        p += 2 + ln
        if m == 0xDB:
            while b:
                assert b[0] >> 4 == 0
                nat = np.zeros(64, np.int64)
                nat[ZZ] = np.frombuffer(b[1:65], np.uint8)
                o["q"][b[0] & 15] = nat
                b = b[65:]
        elif m == 0xC4:
            while b:
                bits, n = list(b[1:17]), sum(b[1:17])
                vals, tab, code, k = b[17:17 + n], {}, 0, 0
                for ln_ in range(1, 17):
                    for _ in range(bits[ln_ - 1]):
                        tab[(ln_, code)] = vals[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                o["huff"][(b[0] >> 4, b[0] & 15)] = tab
                b = b[17 + n:]
        elif m == 0xC0:
            assert b[0] == 8
            o["H"], o["W"] = int.from_bytes(b[1:3], "big"), int.from_bytes(b[3:5], "big")
            o["comps"] = [(b[6 + 3 * i], b[7 + 3 * i] >> 4, b[7 + 3 * i] & 15, b[8 + 3 * i]) for i in range(b[5])]
        elif m == 0xDD:
            o["dri"] = int.from_bytes(b, "big")
        elif m == 0xDA:
            o["scan"] = [(b[2 + 2 * i] >> 4, b[2 + 2 * i] & 15) for i in range(b[0])]
            o["start"] = p
            return o
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        else:
            raise ValueError(f"marker {m:#x} outside the contract")


def split_segments(data):
    """Entropy data through EOI -> the unstuffed bytes of each restart segment."""
    segs, cur, i = [], bytearray(), 0
    while i < len(data):
        v = data[i]
        if v != 0xFF:
            cur.append(v)
            i += 1
        elif i + 1 < len(data) and data[i + 1] == 0:
            cur.append(0xFF)
            i += 2
        elif i + 1 < len(data) and 0xD0 <= data[i + 1] <= 0xD7:
            segs.append(bytes(cur))
            cur = bytearray()
            i += 2
        else:
            break                      # EOI (or any other marker) ends the data
    segs.append(bytes(cur))
    return segs


class _Reader:
    def __init__(self, raw):
        self.v, self.n, self.pos = int.from_bytes(raw, "big") if raw else 0, 8 * len(raw), 0

    def bits(self, k):
        if self.pos + k > self.n:
            raise Damaged("data ran out")
        r = (self.v >> (self.n - self.pos - k)) & ((1 << k) - 1)
        self.pos += k
        return r

    def symbol(self, tab):
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | self.bits(1)
            s = tab.get((ln, code))
            if s is not None:
                return s
        raise Damaged("invalid code")

    def value(self, s):
        v = self.bits(s)
        return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def _idct_pass(x, axis):
    """The 1-D pass along `axis` of int64 blocks (..., 8, 8), unrounded."""
    i = [np.take(x, k, axis=axis) for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack(out, axis=axis)


def idct(coef):
    """Dequantised int64 blocks (..., 8, 8) [row][column] -> uint8 samples."""
    ws = (_idct_pass(coef, -2) + 1024) >> 11           # columns first: along the row index
    px = (_idct_pass(ws, -1) + 131072) >> 18
    return np.clip(px + 128, 0, 255).astype(np.uint8)


def _upsample(p, dw, dh):
    """Chroma plane (real size dh x dw in its top left) -> (2*dh, 2*dw) int64."""
    p = p[:dh, :dw].astype(np.int64)
    if dw <= 2:
        return np.repeat(np.repeat(p, 2, 0), 2, 1)
    top = 3 * p + np.vstack([p[:1], p[:-1]])
    bot = 3 * p + np.vstack([p[1:], p[-1:]])
    s = np.empty((2 * dh, dw), np.int64)
    s[0::2], s[1::2] = top, bot
    left = np.hstack([s[:, :1], s[:, :-1]])
    right = np.hstack([s[:, 1:], s[:, -1:]])
    out = np.empty((2 * dh, 2 * dw), np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out


def decode(jpg):
    h = parse(jpg)
    W, H, nc = h["W"], h["H"], len(h["comps"])
    if nc == 3:
        assert [(c[1], c[2]) for c in h["comps"]] == [(2, 2), (1, 1), (1, 1)], "4:2:0 only"
    else:
        assert nc == 1
    mpx = 16 if nc == 3 else 8
    mx, my = -(-W // mpx), -(-H // mpx)
    mcus = mx * my
    ri = min(h["dri"], mcus) if h["dri"] else mcus
    segs = split_segments(jpg[h["start"]:])
    if len(segs) != -(-mcus // ri):
        raise Damaged(f"{len(segs)} segments, {-(-mcus // ri)} expected")
    layout = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (2, 0, 0)] if nc == 3 else [(0, 0, 0)]
    per = 2 if nc == 3 else 1
    blocks = [np.zeros((my * per, mx * per, 64), np.int64)] + [np.zeros((my, mx, 64), np.int64) for _ in range(nc - 1)]
    tabs = [(h["huff"][(0, td)], h["huff"][(1, ta)]) for td, ta in h["scan"]]
    for s, raw in enumerate(segs):
        rd, pred = _Reader(raw), [0] * nc
        for m in range(s * ri, min((s + 1) * ri, mcus)):
            y, x = divmod(m, mx)
            for c, dy, dx in layout:
                blk = blocks[c][y * (per if c == 0 else 1) + dy, x * (per if c == 0 else 1) + dx]
                sz = rd.symbol(tabs[c][0])
                if sz > 15:
                    raise Damaged("DC size")
                pred[c] += rd.value(sz) if sz else 0
                blk[0] = pred[c]
                k = 1
                while k < 64:
                    rs = rd.symbol(tabs[c][1])
                    r, sz = rs >> 4, rs & 15
                    if sz == 0:
                        if r != 15:
                            break
                        k += 16
                        if k > 64:
                            raise Damaged("run past 63")
                        continue
                    k += r
                    if k > 63:
                        raise Damaged("run past 63")
                    blk[ZZ[k]] = rd.value(sz)
                    k += 1
    planes = []
    for c in range(nc):
        q = h["q"][h["comps"][c][3]]
        px = idct((blocks[c] * q).reshape(blocks[c].shape[0], blocks[c].shape[1], 8, 8))
        planes.append(px.swapaxes(1, 2).reshape(px.shape[0] * 8, px.shape[1] * 8))
    if nc == 1:
        return np.ascontiguousarray(planes[0][:H, :W])
    dw, dh = (W + 1) // 2, (H + 1) // 2
    Y = planes[0][:H, :W].astype(np.int64)
    cb = _upsample(planes[1], dw, dh)[:H, :W] - 128
    cr = _upsample(planes[2], dw, dh)[:H, :W] - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([B, G, R], -1), 0, 255).astype(np.uint8)
