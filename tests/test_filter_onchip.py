"""GPU parity of the contour filter's on-chip masks (fd_kernels.hip).

k_resolve keeps the filled rows of a workgroup's 16 (row groups of 16 lanes) or
32 (groups of 8 lanes, launches of >= 96 x 1080 rows) consecutive image rows in
LDS and takes row y+1 from the neighbouring group, the row after the
workgroup's last one from a halo it resolves again. The cases below put what
can go wrong there on the seams between two workgroups: rows 15/16 and 31/32
(groups of 16 lanes), 31/32 and 63/64 (groups of 8). For block sizes 4 and 8
k_paint_dilate paints the kept rows of 32-row groups (and the dilation window's
rows around them) into LDS and dilates from there; every device run is repeated
with DVC_FLAG_FD_KEPT_PLANE (kept_plane=True), the form through the kept mask's
bit plane, which a dilation window taller than 64 rows takes by itself.

Inputs are hand-drawn pictures (flat rectangles on a flat background) that
alternate with blank frames, so every frame's motion mask is the drawn shapes
grown by the 5x5 blur's two pixels; each case checks on the ORACLE's motion
mask that the shapes lie where it needs them, then every frame's overlay and
compressed frame and the counters against oracle.OracleFD stepped frame by
frame, through the C-ABI as tests/test_fd_gpu.py does.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BG, FG = 40, 200
MOTION, FILTERED = 1, 2


# ---------------------------------------------------------------- pictures ---
# Shapes are given in MASK coordinates (inclusive pixel ranges of the motion
# mask); the picture is drawn two pixels smaller / its holes two pixels larger,
# except at the image border, where the picture reaches the border.
def _pic(W, H):
    return np.full((H, W), BG, np.uint8)


def _rect(p, x0, y0, x1, y1, v=FG):
    H, W = p.shape
    px0, py0 = (0 if x0 == 0 else x0 + 2), (0 if y0 == 0 else y0 + 2)
    px1, py1 = (W - 1 if x1 == W - 1 else x1 - 2), (H - 1 if y1 == H - 1 else y1 - 2)
    assert px0 <= px1 and py0 <= py1, "a mask rectangle is at least 5 px wide and high"
    p[py0:py1 + 1, px0:px1 + 1] = v


def _hole(p, x0, y0, x1, y1):
    p[y0 - 2:y1 + 3, x0 - 2:x1 + 3] = BG


def _ring(p, outer, hole):
    _rect(p, *outer)
    _hole(p, *hole)


def _bgr(pics):
    """blank, picture 0, blank, picture 1, ...: frame 0 primes, every later frame's mask is a picture's."""
    H, W = pics[0].shape
    out = [np.full((H, W), BG, np.uint8)]
    for p in pics:
        out += [p, out[0]]
    return np.repeat(np.stack(out)[..., None], 3, axis=3)


def _hole_rows(mask, x, y_in):
    """first and last row of the background column segment of ``mask`` through (x, y_in)"""
    assert mask[y_in, x] == 0
    a = b = y_in
    while mask[a - 1, x] == 0:
        a -= 1
    while mask[b + 1, x] == 0:
        b += 1
    return a, b


def _rows_of(mask, x0, x1):
    r = np.flatnonzero(mask[:, x0:x1 + 1].any(1))
    return int(r[0]), int(r[-1])


def seam_picture(W, H, s):
    """The seam cases around rows s-1 / s (s = 16, 32 or 64), in columns 0..199.
    Returns (picture, checks); checks(motion mask, filtered mask) asserts the geometry."""
    p = _pic(W, H)
    _ring(p, (4, s - 10, 44, s + 12), (12, s, 36, s + 5))             # a hole whose top row is s
    _ring(p, (50, s - 14, 90, s + 7), (58, s - 7, 82, s - 1))         # a hole whose bottom row is s - 1
    _ring(p, (96, s - 16, 146, s + 15), (102, s - 10, 140, s + 9))    # a component nested in a hole,
    _rect(p, 112, s - 4, 130, s + 3)                                  # ... across the seam
    _rect(p, 152, s - 12, 196, s - 1)                                 # kept, bottom row s - 1
    _rect(p, 160, s + 2, 166, s + 6)                                  # dropped, two rows below it

    def checks(m, f):
        assert _hole_rows(m, 24, s + 2) == (s, s + 5)
        assert _hole_rows(m, 70, s - 3) == (s - 7, s - 1)
        assert _rows_of(m[s - 9:s + 9], 112, 130) == (5, 12)          # rows s - 4 .. s + 3
        assert m[s - 5, 120] == 0 and m[s + 4, 120] == 0
        assert _rows_of(m, 170, 196) == (s - 12, s - 1)
        assert _rows_of(m[s:], 160, 166) == (2, 6)
        assert f[s - 1, 180] and not f[s + 2:s + 7, 160:167].any() and m[s + 4, 163]
        assert f[s + 2, 24] and f[s - 3, 70]                          # holes are filled (drawContours FILLED)
    return p, checks


def border_picture(W, H):
    p = _pic(W, H)
    _rect(p, 100, 0, 130, 8)              # touches row 0
    _rect(p, 10, H - 10, 60, H - 1)       # touches row H - 1
    _rect(p, W - 30, 20, W - 1, 30)       # and the right border, in the partial last word
    return p


def _device_run(gpu_lib, frames, sizes, monkeypatch, graph=True, out_format="BGR", **kw):
    """frames[0] primes; frames[1:] go through step_batch in calls of ``sizes`` frames (device pointers)."""
    import torch
    monkeypatch.setenv("DVC_FD_GRAPH", "1" if graph else "0")
    H, W = frames.shape[1:3]
    dev = torch.device("cuda", 0)
    seq = torch.from_numpy(frames).to(dev)
    n = sum(sizes)
    assert n == len(frames) - 1
    oshape = (n, H, W, 3) if out_format == "BGR" else (n, H * 3 // 2, W)
    ov = torch.zeros(oshape, dtype=torch.uint8, device=dev)
    cp = torch.zeros_like(ov)
    w = gpu_lib.FDWorker(W, H, device=0, device_ptrs=True, max_batch=max(sizes), out_format=out_format, **kw)
    w.prime(seq[0])
    j = 0
    for m in sizes:
        w.step_batch(seq[1 + j:1 + j + m], ov[j:j + m], cp[j:j + m])   # no sync between the calls
        j += m
    w.sync()
    res = ov.cpu().numpy(), cp.cpu().numpy(), w.stats(), w.graph_stats()
    w.close()
    return res


def _oracle_run(oracle, frames, out_format="BGR", **kw):
    """(overlays, compressed, stats, motion masks, filtered masks) of the oracle stepped frame by frame"""
    H, W = frames.shape[1:3]
    ref = oracle.OracleFD(W, H, **kw)
    ref.prime(frames[0])
    ov, cp, mo, fi = [], [], [], []
    for f in frames[1:]:
        o, c, _ = ref.step(f)
        if out_format == "I420":
            o, c = oracle.bgr_to_i420(o), oracle.bgr_to_i420(c)
        ov.append(o)
        cp.append(c)
        mo.append(ref.plane(MOTION))
        fi.append(ref.plane(FILTERED))
    st = ref.stats()
    ref.close()
    return np.stack(ov), np.stack(cp), st, mo, fi


def _same(got, ref, what=""):
    for t in range(len(ref[0])):
        assert np.array_equal(got[0][t], ref[0][t]), f"{what}: overlay differs at frame {t + 1}"
        assert np.array_equal(got[1][t], ref[1][t]), f"{what}: compressed differs at frame {t + 1}"
    assert got[2] == ref[2], (what, got[2], ref[2])


KW = dict(min_area=30)


# ------------------------------------------------------------------- seams ---
@pytest.fixture(scope="module")
def seams16(oracle_lib):
    """200 x 70: WW = 4 with a partial last word, H no multiple of 4, 16 or 32, a
    partial last block row. Seams 15/16 and 31/32 of the 16-row workgroups."""
    W, H = 200, 70
    pa, ca = seam_picture(W, H, 16)
    pb, cb = seam_picture(W, H, 32)
    frames = _bgr([pa, pb, border_picture(W, H), pa])
    ref = _oracle_run(oracle_lib, frames, **KW)
    for t, c in ((0, ca), (1, ca), (2, cb), (3, cb)):
        c(ref[3][t], ref[4][t])
    m = ref[3][4]
    assert m[0, 115] and m[H - 1, 30] and m[25, W - 1] and ref[4][4][0, 115] and ref[4][4][H - 1, 30]
    return frames, ref


def test_seams_per_frame_planes(gpu_lib, oracle_lib, seams16):
    """Host steps with the planes kept: motion, filtered, dilated and accumulated masks per frame."""
    from tests.test_fd_gpu import _run_pair
    st = _run_pair(gpu_lib, oracle_lib, seams16[0], **KW)
    assert st == seams16[1][2]


@pytest.mark.parametrize("sizes", [[1] * 8, [8], [3, 5]])
def test_seams_16_row_groups(gpu_lib, seams16, monkeypatch, sizes):
    frames, ref = seams16
    g = _device_run(gpu_lib, frames, sizes, monkeypatch, **KW)
    assert g[3]["batches"] == len(sizes)
    _same(g, ref, f"graph {sizes}")
    _same(_device_run(gpu_lib, frames, sizes, monkeypatch, graph=False, **KW), ref, f"streams {sizes}")
    _same(_device_run(gpu_lib, frames, sizes, monkeypatch, kept_plane=True, **KW), ref, f"kept plane {sizes}")


def test_seams_32_row_groups(gpu_lib, oracle_lib, monkeypatch):
    """512 frames of 200 x 206 in one launch: 105 k rows, so launch_ccl takes the
    groups of 8 lanes (32 rows a workgroup: seams 31/32 and 63/64; H = 206 leaves
    the last workgroup 14 rows and no halo). Shared filter set (> 128 frames)."""
    W, H, n = 200, 206, 512
    assert n * H >= 96 * 1080
    pa, ca = seam_picture(W, H, 32)
    pb, cb = seam_picture(W, H, 64)
    pc = border_picture(W, H)
    for s in (96, 160, 192):               # more seams of both group heights further down
        q, _ = seam_picture(W, H, s)
        pc = np.maximum(pc, q)
    frames = _bgr(([pa, pb, pc] * (n // 6 + 1))[:n // 2])
    assert len(frames) == n + 1
    ref = _oracle_run(oracle_lib, frames, **KW)
    for t, c in ((0, ca), (1, ca), (2, cb), (3, cb)):
        c(ref[3][t], ref[4][t])
    assert ref[3][4][H - 1, 30] and ref[4][4][H - 1, 30]
    g = _device_run(gpu_lib, frames, [n], monkeypatch, **KW)
    _same(g, ref, "one launch of 512")
    _same(_device_run(gpu_lib, frames, [n], monkeypatch, kept_plane=True, **KW), ref, "kept plane")


# ---------------------------------------------------------- area threshold ---
@pytest.mark.parametrize("holed", [False, True])
def test_area_threshold_exact(gpu_lib, oracle_lib, monkeypatch, holed):
    """contourArea > min_area: a component whose area is exactly min_area is
    dropped, the next larger one kept — side by side in one mask, the threshold
    taken from the oracle's own contour filter, the pair across the seam 15/16."""
    W, H = 200, 70
    p = _pic(W, H)
    small, large = (10, 6, 40, 26), (60, 6, 91, 26)
    for r in (small, large):
        _rect(p, *r)
        if holed:                                   # RETR_EXTERNAL: a hole does not change the area
            _hole(p, r[0] + 8, 12, r[2] - 8, 18)
    frames = _bgr([p, p])
    probe = _oracle_run(oracle_lib, frames, min_area=0)
    m = probe[3][0]
    assert _rows_of(m, 10, 40) == (6, 26) and m[:, 41:60].sum() == 0
    # 2 * area of the smaller component: the largest threshold that still keeps it, plus one
    a2 = next(a for a in range(1, 4000) if not oracle_lib.contour_filter(m[:, :50], a)[0].any())
    assert oracle_lib.contour_filter(m[:, 50:], a2)[0].any(), "the larger component has a larger area"
    assert a2 % 2 == 0
    kw = dict(min_area=a2 / 2)
    ref = _oracle_run(oracle_lib, frames, **kw)
    for t in range(len(frames) - 1):
        assert not ref[4][t][:, :50].any() and ref[4][t][15, 75] and ref[4][t][16, 75]
    _same(_device_run(gpu_lib, frames, [4], monkeypatch, **kw), ref, "exact area")
    # one below the threshold keeps both
    kw = dict(min_area=(a2 - 1) / 2)
    ref = _oracle_run(oracle_lib, frames, **kw)
    assert ref[4][0][16, 25] and ref[4][0][16, 75]
    _same(_device_run(gpu_lib, frames, [4], monkeypatch, **kw), ref, "one below")


# ---------------------------------------------------------------- dilation ---
def _dilation_frames():
    W, H = 200, 70
    pa, _ = seam_picture(W, H, 16)
    pb, _ = seam_picture(W, H, 32)
    dots = _pic(W, H)                      # only components below min_area: nothing kept
    for x in (20, 90, 150):
        _rect(dots, x, 30, x + 5, 35)
    return _bgr([pa, dots, pb, border_picture(W, H)])


@pytest.mark.parametrize("kw", [
    dict(kernel_size=7, block_size=4),
    dict(kernel_size=10, block_size=8),    # an even kernel: the anchor is off centre
    dict(kernel_size=3, block_size=4),
    dict(kernel_size=3, block_size=8),
    dict(kernel_size=64, block_size=4),    # a window taller than 64 rows
    dict(kernel_size=7, block_size=6),     # the generic back end
], ids=lambda k: f"k{k['kernel_size']}b{k['block_size']}")
def test_dilation_windows(gpu_lib, oracle_lib, monkeypatch, kw):
    """The kept mask into the dilated block fields, with frames that keep nothing
    (frames 3 and 4: no dilated bit anywhere) between frames that keep some."""
    frames = _dilation_frames()
    kw = dict(kw, **KW)
    ref = _oracle_run(oracle_lib, frames, **kw)
    assert ref[4][0].any() and not ref[4][2].any() and not ref[4][3].any() and ref[4][4].any()
    assert ref[3][2].any()
    for sizes in ([1] * 8, [8]):
        _same(_device_run(gpu_lib, frames, sizes, monkeypatch, **kw), ref, f"graph {sizes}")
    _same(_device_run(gpu_lib, frames, [8], monkeypatch, graph=False, **kw), ref, "streams")
    _same(_device_run(gpu_lib, frames, [3, 5], monkeypatch, kept_plane=True, **kw), ref, "kept plane")
    from tests.test_fd_gpu import _run_pair
    _run_pair(gpu_lib, oracle_lib, frames, **kw)      # the dilated plane itself, frame by frame


# ---------------------------------------------------------------- batching ---
@pytest.fixture(scope="module")
def long_clip(oracle_lib):
    W, H = 200, 70
    pa, _ = seam_picture(W, H, 16)
    pb, _ = seam_picture(W, H, 32)
    pics = [pa, pb, border_picture(W, H)]
    frames = _bgr([pics[i % 3] for i in range(74)])      # 148 frames after the priming one
    return frames, _oracle_run(oracle_lib, frames, **KW)


def test_batches_own_and_shared_filter_sets(gpu_lib, long_clip, monkeypatch):
    """n = 1 and n = 9 (graph path, the slot's own filter set), n = 130 (the
    shared set), consecutive calls with no sync between them."""
    frames, ref = long_clip
    sizes = [1, 9, 130, 1, 7]
    g = _device_run(gpu_lib, frames, sizes, monkeypatch, **KW)
    assert g[3]["batches"] == len(sizes)
    _same(g, ref, "graph")
    _same(_device_run(gpu_lib, frames, sizes, monkeypatch, graph=False, **KW), ref, "streams")
    _same(_device_run(gpu_lib, frames, sizes, monkeypatch, kept_plane=True, **KW), ref, "kept plane")


def test_two_long_batches_without_sync(gpu_lib, long_clip, monkeypatch):
    frames, ref = long_clip
    f = frames[:141]
    r = tuple(x[:140] for x in ref[:2])
    for graph in (True, False):
        g = _device_run(gpu_lib, f, [70, 70], monkeypatch, graph=graph, **KW)
        for t in range(140):
            assert np.array_equal(g[0][t], r[0][t]) and np.array_equal(g[1][t], r[1][t]), (graph, t)


def test_i420_outputs(gpu_lib, oracle_lib, monkeypatch):
    """I420 frames are whole 4x4 blocks: 200 x 72."""
    W, H = 200, 72
    pics = [seam_picture(W, H, 16)[0], seam_picture(W, H, 32)[0], border_picture(W, H)]
    frames = _bgr(pics * 2)
    ref = _oracle_run(oracle_lib, frames, out_format="I420", **KW)
    _same(_device_run(gpu_lib, frames, [1, 9, 2], monkeypatch, out_format="I420", **KW), ref, "I420")


def test_one_word_one_row_group(gpu_lib, oracle_lib, monkeypatch):
    """64 x 16: one 64-px word a row, one row group, no seam and no halo."""
    W, H = 64, 16
    p = _pic(W, H)
    _ring(p, (2, 0, 40, 15), (10, 6, 32, 9))
    _rect(p, 46, 3, 63, 12)
    frames = _bgr([p, p])
    kw = dict(min_area=20)
    ref = _oracle_run(oracle_lib, frames, **kw)
    assert _hole_rows(ref[3][0], 20, 7) == (6, 9) and ref[4][0][7, 20] and ref[4][0][8, 60]
    _same(_device_run(gpu_lib, frames, [1, 3], monkeypatch, **kw), ref, "64x16")
    from tests.test_fd_gpu import _run_pair
    _run_pair(gpu_lib, oracle_lib, frames, **kw)
