"""Independent numpy decoder for the camera stream set of DESIGN.md "Motion-JPEG
decoder": three components with 4:2:0, 4:2:2 (luma 2x1) or 4:4:4 sampling, or
one component, with or without DHT segments. It shares nothing with the library;
the entropy reader, the IDCT and the 4:2:0 upsampling are those of
``tests/mjpeg_dec_ref.py``. ``decode(jpeg_bytes)`` returns what Pillow returns:
(H, W, 3) BGR or (H, W) uint8. The Huffman tables a DHT-less stream means are
taken from a default Pillow (libjpeg-turbo) stream, not from the library's
Annex K arrays.
"""
import functools
import io

import numpy as np

from tests import mjpeg_dec_ref as R

Damaged = R.Damaged


@functools.lru_cache(maxsize=None)
def std_huff():
    """{(class, slot): {(length, code): symbol}} of the tables libjpeg writes by default."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, "JPEG", quality=75)
    h = R.parse(buf.getvalue())["huff"]
    assert sorted(h) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    return h


def sampling(jpg):
    """(hs, vs) of the luma component; (1, 1) for a single component."""
    comps = R.parse(jpg)["comps"]
    return (comps[0][1], comps[0][2]) if len(comps) == 3 else (1, 1)


def _upsample_h2v1(p, dw, H):
    """Chroma plane (real size H x dw in its top left) -> (H, 2*dw) int64: no vertical step."""
    p = p[:H, :dw].astype(np.int64)
    if dw <= 2:
        return np.repeat(p, 2, 1)
    left = np.hstack([p[:, :1], p[:, :-1]])
    right = np.hstack([p[:, 1:], p[:, -1:]])
    out = np.empty((H, 2 * dw), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    return out


def decode(jpg):
    h = R.parse(jpg)
    W, H, nc = h["W"], h["H"], len(h["comps"])
    hs, vs = 1, 1
    if nc == 3:
        hs, vs = h["comps"][0][1], h["comps"][0][2]
        assert (hs, vs) in ((2, 2), (2, 1), (1, 1)) and all(c[1:3] == (1, 1) for c in h["comps"][1:]), "sampling"
    else:
        assert nc == 1
    huff = dict(std_huff())
    huff.update(h["huff"])                       # a DHT that is present wins
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    mcus = mx * my
    ri = min(h["dri"], mcus) if h["dri"] else mcus
    segs = R.split_segments(jpg[h["start"]:])
    if len(segs) != -(-mcus // ri):
        raise Damaged(f"{len(segs)} segments, {-(-mcus // ri)} expected")
    layout = [(0, dy, dx) for dy in range(vs) for dx in range(hs)] + [(1, 0, 0), (2, 0, 0)] if nc == 3 else [(0, 0, 0)]
    blocks = [np.zeros((my * vs, mx * hs, 64), np.int64)] + [np.zeros((my, mx, 64), np.int64) for _ in range(nc - 1)]
    tabs = [(huff[(0, td)], huff[(1, ta)]) for td, ta in h["scan"]]
    for s, raw in enumerate(segs):
        rd, pred = R._Reader(raw), [0] * nc
        for m in range(s * ri, min((s + 1) * ri, mcus)):
            y, x = divmod(m, mx)
            for c, dy, dx in layout:
                blk = blocks[c][y * (vs if c == 0 else 1) + dy, x * (hs if c == 0 else 1) + dx]
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
                    blk[R.ZZ[k]] = rd.value(sz)
                    k += 1
    planes = []
    for c in range(nc):
        q = h["q"][h["comps"][c][3]]
        px = R.idct((blocks[c] * q).reshape(blocks[c].shape[0], blocks[c].shape[1], 8, 8))
        planes.append(px.swapaxes(1, 2).reshape(px.shape[0] * 8, px.shape[1] * 8))
    if nc == 1:
        return np.ascontiguousarray(planes[0][:H, :W])
    dw, dh = -(-W // hs), -(-H // vs)
    Y = planes[0][:H, :W].astype(np.int64)
    if (hs, vs) == (2, 2):
        up = [R._upsample(p, dw, dh) for p in planes[1:]]
    elif (hs, vs) == (2, 1):
        up = [_upsample_h2v1(p, dw, H) for p in planes[1:]]
    else:
        up = [p.astype(np.int64) for p in planes[1:]]   # 4:4:4: the samples as they are
    cb, cr = up[0][:H, :W] - 128, up[1][:H, :W] - 128
    Rr = Y + ((91881 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([B, G, Rr], -1), 0, 255).astype(np.uint8)
