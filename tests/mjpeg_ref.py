"""Independent numpy restatement of the Motion-JPEG stream format (DESIGN.md
"Motion-JPEG stream"), in the manner of ``tests/farneback_ref.py``: nothing
here shares code or tables with the library. The quantiser and Huffman tables,
the frame size, the sampling factors and the restart interval are parsed out
of the bytes ``dvc_jpeg_header`` returns (a host-only handle: no GPU).

``encode(frame, quality)`` returns the entropy-coded data with its RST markers
and EOI (what ``dvc_jpeg_encode`` must produce byte for byte), the whole JFIF
image, and a float64 inverse-DCT reconstruction of the Y, Cb and Cr planes
(Cb, Cr at half size) for comparison with a decoder that is not ours.
"""
import ctypes

import numpy as np

FMT_BGR, FMT_GRAY = 0, 3


def header_bytes(width, height, fmt, quality):
    """dvc_jpeg_header of a host-only handle (device -1)."""
    from dvc_amd import _native as N
    L = N.lib()
    h = ctypes.c_void_p()
    N.check(L.dvc_jpeg_create(width, height, fmt, quality, 1, -1, None, 0, ctypes.byref(h)))
    try:
        n = ctypes.c_size_t()
        N.check(L.dvc_jpeg_header(h, None, 0, ctypes.byref(n)))
        buf = (ctypes.c_uint8 * n.value)()
        N.check(L.dvc_jpeg_header(h, buf, n.value, ctypes.byref(n)))
        return bytes(buf)
    finally:
        L.dvc_jpeg_destroy(h)


def _zigzag():
    """Natural (row-major) index of each zigzag position, walked along the anti-diagonals."""
    out, r, c, up = [], 0, 0, True
    for _ in range(64):
        out.append(r * 8 + c)
        if up:
            if c == 7:
                r, up = r + 1, False
            elif r == 0:
                c, up = c + 1, False
            else:
                r, c = r - 1, c + 1
        else:
            if r == 7:
                c, up = c + 1, True
            elif c == 0:
                r, up = r + 1, True
            else:
                r, c = r + 1, c - 1
    return out


ZIGZAG = _zigzag()


def parse_header(hdr):
    """Markers SOI .. SOS -> dict(order, q, huff, W, H, comps, dri, scan, length)."""
    assert hdr[:2] == b"\xff\xd8", "no SOI"
    info = {"order": ["SOI"], "q": {}, "huff": {}, "bits": {}}
    p = 2
    while p < len(hdr):
        assert hdr[p] == 0xFF, f"marker expected at {p}"
        m = hdr[p + 1]
        ln = int.from_bytes(hdr[p + 2:p + 4], "big")
        body = hdr[p + 4:p + 2 + ln]
        p += 2 + ln
        if m == 0xE0:
            info["order"].append("APP0")
            info["jfif"] = body
        elif m == 0xDB:
            info["order"].append("DQT")
            assert len(body) == 65 and body[0] >> 4 == 0      # 8-bit entries
            nat = np.zeros(64, np.int64)
            nat[ZIGZAG] = np.frombuffer(body[1:], np.uint8)
            info["q"][body[0] & 15] = nat
        elif m == 0xC0:
            info["order"].append("SOF0")
            assert body[0] == 8
            info["H"], info["W"] = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            info["comps"] = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i])
                             for i in range(body[5])]
        elif m == 0xC4:
            info["order"].append("DHT")
            bits, vals = list(body[1:17]), list(body[17:])
            assert sum(bits) == len(vals)
            table, code, k = {}, 0, 0
            for ln_ in range(1, 17):
                for _ in range(bits[ln_ - 1]):
                    table[vals[k]] = (code, ln_)
                    code, k = code + 1, k + 1
                code <<= 1
            info["huff"][(body[0] >> 4, body[0] & 15)] = table
            info["bits"][(body[0] >> 4, body[0] & 15)] = bits
        elif m == 0xDD:
            info["order"].append("DRI")
            info["dri"] = int.from_bytes(body, "big")
        elif m == 0xDA:
            info["order"].append("SOS")
            info["scan"] = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(body[0])]
            assert tuple(body[1 + 2 * body[0]:]) == (0, 63, 0)
        else:
            raise AssertionError(f"unexpected marker {m:#x}")
    info["length"] = p
    assert p == len(hdr)
    return info


def _dct_int_matrix():
    M = np.zeros((8, 8), np.int64)
    for k in range(8):
        a = np.sqrt(1 / 8) if k == 0 else np.sqrt(2 / 8)
        for n in range(8):
            M[k, n] = int(np.rint(8192 * a * np.cos((2 * n + 1) * k * np.pi / 16)))
    return M


def _idct_f64(coef):
    """Orthonormal float64 inverse DCT of (..., 8, 8) coefficient blocks, + 128."""
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    C = np.where(k == 0, np.sqrt(1 / 8), np.sqrt(2 / 8)) * np.cos((2 * n + 1) * k * np.pi / 16)
    return C.T @ coef.astype(np.float64) @ C + 128.0


def _edge_pad(p, m):
    h, w = p.shape
    hh, ww = -(-h // m) * m, -(-w // m) * m
    out = np.empty((hh, ww), p.dtype)
    out[:h, :w] = p
    out[:h, w:] = p[:, w - 1:w]
    out[h:, :] = out[h - 1:h, :]
    return out


def _component_levels(plane, Q):
    """Padded plane (multiples of 8) -> levels [by][bx][8][8] (natural order, AC clamped) ."""
    M = _dct_int_matrix()
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    lv = np.zeros((hb, wb, 8, 8), np.int64)
    q = Q.reshape(8, 8)
    for by in range(hb):
        for bx in range(wb):
            x = plane[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].astype(np.int64) - 128
            R = (x @ M.T + 512) >> 10          # rows: R[y][k]
            F = (M @ R + 32768) >> 16          # columns: F[v][k]
            l = np.sign(F) * ((np.abs(F) + q // 2) // q)
            dc = l[0, 0]
            l = np.clip(l, -1023, 1023)
            l[0, 0] = dc
            lv[by, bx] = l
    return lv


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, n):
        self.acc = (self.acc << n) | code
        self.n += n

    def segment(self):
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        raw = self.acc.to_bytes(self.n // 8, "big")
        return raw.replace(b"\xff", b"\xff\x00"), raw.count(b"\xff")


def _mag(v, size):
    return v if v >= 0 else v + (1 << size) - 1


def _code_block(bits, lv_nat, pred, dc_tab, ac_tab):
    zz = [int(lv_nat.reshape(64)[i]) for i in ZIGZAG]
    d = max(-2047, min(2047, zz[0] - pred))
    s = abs(d).bit_length()
    bits.put(*dc_tab[s])
    bits.put(_mag(d, s), s)
    run = 0
    for k in range(1, 64):
        v = zz[k]
        if v == 0:
            run += 1
            continue
        while run >= 16:
            bits.put(*ac_tab[0xF0])
            run -= 16
        s = abs(v).bit_length()
        bits.put(*ac_tab[(run << 4) | s])
        bits.put(_mag(v, s), s)
        run = 0
    if run:
        bits.put(*ac_tab[0x00])
    return zz[0]


def encode(frame, quality):
    """frame: (H, W, 3) BGR or (H, W) uint8 -> dict(stream, jpeg, header, Y, Cb, Cr, stuffed, info)."""
    frame = np.asarray(frame, np.uint8)
    gray = frame.ndim == 2
    H, W = frame.shape[:2]
    hdr = header_bytes(W, H, FMT_GRAY if gray else FMT_BGR, quality)
    info = parse_header(hdr)
    assert (info["W"], info["H"]) == (W, H)
    if gray:
        assert [(c[1], c[2]) for c in info["comps"]] == [(1, 1)]
        planes = [_edge_pad(frame.astype(np.int64), 8)]
    else:
        assert [(c[1], c[2]) for c in info["comps"]] == [(2, 2), (1, 1), (1, 1)]
        b, g, r = (frame[..., i].astype(np.int64) for i in range(3))
        y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
        cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
        cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
        planes = [_edge_pad(y, 16)]
        for c in (cb, cr):
            c = _edge_pad(c, 16)
            planes.append((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2)
    Q = [info["q"][c[3]] for c in info["comps"]]
    levels = [_component_levels(p, q) for p, q in zip(planes, Q)]
    tabs = {cid: (info["huff"][(0, td)], info["huff"][(1, ta)]) for cid, td, ta in info["scan"]}
    tabs = [tabs[c[0]] for c in info["comps"]]
    mcu_rows, mcus_x = (levels[0].shape[0], levels[0].shape[1]) if gray else (levels[1].shape[0], levels[1].shape[1])
    assert info["dri"] == mcus_x
    out, stuffed = bytearray(), 0
    for my in range(mcu_rows):
        bits, pred = _Bits(), [0, 0, 0]
        for mx in range(mcus_x):
            if gray:
                pred[0] = _code_block(bits, levels[0][my, mx], pred[0], *tabs[0])
                continue
            for dy in (0, 1):
                for dx in (0, 1):
                    pred[0] = _code_block(bits, levels[0][2 * my + dy, 2 * mx + dx], pred[0], *tabs[0])
            pred[1] = _code_block(bits, levels[1][my, mx], pred[1], *tabs[1])
            pred[2] = _code_block(bits, levels[2][my, mx], pred[2], *tabs[2])
        seg, nff = bits.segment()
        stuffed += nff
        out += seg
        out += bytes([0xFF, 0xD0 + my % 8]) if my < mcu_rows - 1 else b"\xff\xd9"
    recon = []
    for lv, q in zip(levels, Q):
        px = _idct_f64(lv * q.reshape(8, 8))                  # [by][bx][8][8]
        recon.append(px.swapaxes(1, 2).reshape(lv.shape[0] * 8, lv.shape[1] * 8))
    res = {"levels": levels, "stream": bytes(out), "header": hdr, "jpeg": hdr + bytes(out), "stuffed": stuffed, "info": info,
           "Y": recon[0][:H, :W]}
    if not gray:
        res["Cb"], res["Cr"] = recon[1][:(H + 1) // 2, :(W + 1) // 2], recon[2][:(H + 1) // 2, :(W + 1) // 2]
    return res
