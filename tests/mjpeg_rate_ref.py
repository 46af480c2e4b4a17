"""Independent restatement of the Motion-JPEG rate target (DESIGN.md
"Motion-JPEG stream", "Rate target"), written over ``tests/mjpeg_ref.py`` and
``tests/mjpeg_opt_ref.py``. The base quantiser tables are read out of the DQT
segments of a quality-50 header (there the IJG scale is 100, so the entries
are the base); the IJG formula is applied here and checked against the tables
of every fixed-quality header the estimate is taken from. ``E(q)`` of a group
is the sum over its frames of ``len(mjpeg_ref.encode(frame, q)["jpeg"])`` less
the stuffed bytes; the search is the procedure of the normative text, walked
in plain Python; the expected header, prefix and data are put together from
the fixed-quality (or optimised-table) reference at the quality found.
Nothing here shares code with the library.
"""
import functools

import numpy as np

from tests import mjpeg_opt_ref, mjpeg_ref

PREFIX_MAX = 2 * 69 + mjpeg_opt_ref.PREFIX_MAX        # DQT, DQT and the longest DHT + SOS
STATS = ("groups", "frames", "missed_groups", "est_bytes", "budget_bytes", "quality_frames", "q_lowest", "q_highest",
         "q_last")


@functools.lru_cache(maxsize=None)
def base_tables():
    """(luma, chroma) base tables, natural order, as tuples."""
    info = mjpeg_ref.parse_header(mjpeg_ref.header_bytes(16, 16, mjpeg_ref.FMT_BGR, 50))
    return tuple(int(v) for v in info["q"][0]), tuple(int(v) for v in info["q"][1])


def quant(base, q):
    """The IJG scaling of a base table to quality q, 8-bit entries."""
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [min(255, max(1, (b * scale + 50) // 100)) for b in base]


def dqt_pair(q):
    """DQT id 0 and DQT id 1 of quality q (both, also for one component)."""
    out = b""
    for tid, base in enumerate(base_tables()):
        nat = quant(base, q)
        out += b"\xff\xdb\x00\x43" + bytes([tid]) + bytes(nat[i] for i in mjpeg_ref.ZIGZAG)
    return out


def level(F, Q, ac):
    """Round half away from zero; an AC level stays inside +-1023."""
    l = (abs(F) + Q // 2) // Q
    if ac:
        l = min(l, 1023)
    return -l if F < 0 else l


def rounds(q_min, q_max):
    """1 + ceil(log2(q_max - q_min + 1))."""
    return 1 + (q_max - q_min).bit_length()


_REFS = {}


def ref(frame, q):
    """mjpeg_ref.encode(frame, q), computed once; its tables are the IJG ones of q."""
    frame = np.ascontiguousarray(frame, np.uint8)
    key = (frame.shape, frame.tobytes(), q)
    if key not in _REFS:
        r = mjpeg_ref.encode(frame, q)
        for tid, base in enumerate(base_tables()):
            assert [int(v) for v in r["info"]["q"][tid]] == quant(base, q), (tid, q)
        _REFS[key] = r
    return _REFS[key]


def estimate(frames, q):
    """E(q) of a group: the fixed-table samples' bytes before stuffing."""
    return sum(len(ref(f, q)["jpeg"]) - ref(f, q)["stuffed"] for f in frames)


def search(E, budget, q_min, q_max):
    """The search over a function E(q): (q*, miss, E(q*), [qualities evaluated])."""
    tried = [q_min]
    e = E(q_min)
    if e > budget:
        return q_min, 1, e, tried
    lo, hi, e_lo = q_min, q_max, e
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        tried.append(mid)
        e = E(mid)
        if e <= budget:
            lo, e_lo = mid, e
        else:
            hi = mid - 1
    assert len(tried) <= rounds(q_min, q_max)
    return lo, 0, e_lo, tried


def _strip(hdr, drop):
    """A header without the segments whose marker is in ``drop``."""
    out, p = bytearray(hdr[:2]), 2
    while p < len(hdr):
        ln = int.from_bytes(hdr[p + 2:p + 4], "big")
        if hdr[p + 1] not in drop:
            out += hdr[p:p + 2 + ln]
        p += 2 + ln
    assert p == len(hdr)
    return bytes(out)


def _sos(hdr):
    p = hdr.rindex(b"\xff\xda")
    assert p + 2 + int.from_bytes(hdr[p + 2:p + 4], "big") == len(hdr)
    return hdr[p:]


def encode(frames, target_bytes, q_min, q_max, max_batch, optimize=False):
    """A call's frames in rate groups of max_batch -> dict(header, frames = [prefix +
    entropy data + EOI], groups = [(q*, miss, E(q*), frames in the group)], stats)."""
    frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    out, groups = [], []
    fixed = ref(frames[0], q_min)["header"]
    header = _strip(fixed, (0xDB, 0xDA, 0xC4) if optimize else (0xDB, 0xDA))
    for t in range(0, len(frames), max_batch):
        grp = frames[t:t + max_batch]
        q, miss, e, _ = search(lambda x: estimate(grp, x), len(grp) * target_bytes, q_min, q_max)
        groups.append((q, miss, e, len(grp)))
        refs = [ref(f, q) for f in grp]
        if optimize:
            g = mjpeg_opt_ref.encode_group(refs)
            out += [dqt_pair(q) + f for f in g["frames"]]
        else:
            out += [dqt_pair(q) + _sos(r["header"]) + r["stream"] for r in refs]
    st = dict.fromkeys(STATS, 0)
    for q, miss, e, m in groups:
        st["q_lowest"] = q if not st["groups"] else min(st["q_lowest"], q)
        st["q_highest"] = max(st["q_highest"], q)
        st["q_last"] = q
        st["groups"] += 1
        st["frames"] += m
        st["missed_groups"] += miss
        st["est_bytes"] += e
        st["budget_bytes"] += m * target_bytes
        st["quality_frames"] += q * m
    return {"header": header, "frames": out, "groups": groups, "stats": st}


def add_stats(a, b):
    """The counters of two calls on one handle, a before b."""
    if not a["groups"]:
        return dict(b)
    out = {k: a[k] + b[k] for k in STATS}
    out.update(q_lowest=min(a["q_lowest"], b["q_lowest"]), q_highest=max(a["q_highest"], b["q_highest"]),
               q_last=b["q_last"] if b["groups"] else a["q_last"])
    return out


def segments(data):
    """[(marker, whole segment bytes)] of the marker segments at the start of ``data``
    through SOS (or to its end, if there is none); the rest is returned second."""
    out, p = [], 0
    while p < len(data):
        assert data[p] == 0xFF, p
        m = data[p + 1]
        ln = int.from_bytes(data[p + 2:p + 4], "big")
        out.append((m, data[p:p + 2 + ln]))
        p += 2 + ln
        if m == 0xDA:
            break
    return out, data[p:]


# ---- the fixtures of the tests ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture(name):
    """Frames of a named fixture (a tuple of arrays)."""
    from dvc_amd.synthetic import clip
    if name == "clean48x32":
        return tuple(clip(48, 32, 3, seed=1))
    if name == "noisy40x24":
        return tuple(clip(40, 24, 3, seed=1, noisy=True))
    if name == "gray33x17":
        return tuple(np.ascontiguousarray(f[..., 1]) for f in clip(33, 17, 3, seed=1, noisy=True))
    if name == "flat_then_noise40x24":                   # frames 0-1 flat, 2-4 noise
        rng = np.random.default_rng(5)
        flat = [np.full((24, 40, 3), v, np.uint8) for v in (90, 91)]
        return tuple(flat + [rng.integers(0, 256, (24, 40, 3), dtype=np.uint8) for _ in range(3)])
    if name in ("wide688x16", "tall16x48"):              # one segment of 258 blocks; three segments
        W, H = (688, 16) if name == "wide688x16" else (16, 48)
        rng = np.random.default_rng(W)
        ramp = (np.arange(W)[None, :, None] * 3 + np.arange(H)[:, None, None] * 5 + np.arange(3)[None, None, :] * 40) % 256
        return (np.clip(ramp + rng.integers(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8),)
    if name == "clip64x48":
        return tuple(clip(64, 48, 12, seed=2, noisy=True))
    raise KeyError(name)
