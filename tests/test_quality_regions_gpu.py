"""GPU: dvc_quality_compare_regions equals tests/quality_regions_ref.py in all
sixteen integers of every record — every shape, block size, partial-block rule,
mask and content of tests/quality_regions_cases.py, padded pitches and strides,
host and device pointers, batches split over calls — adds up to
dvc_quality_compare on the same handle and leaves that call as it was; its
refusals; and the drivers' outputs end to end: every pixel the report calls
static is one the workers flattened to grey."""
import csv
import ctypes
import os

import numpy as np
import pytest

from tests import quality_cases as C
from tests import quality_ref as R
from tests import quality_regions_cases as RC
from tests import quality_regions_ref as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N(gpu_lib):
    return gpu_lib._native


def _handle(N, W, H, max_batch, stream=None, flags=0):
    h = ctypes.c_void_p()
    N.check(N.lib().dvc_quality_create(W, H, max_batch, 0, stream, flags, ctypes.byref(h)))
    return h


def _laid_out(frames, pitch, stride, lead=0, fill=0x5A):
    """`frames` (n, H, row bytes...) in a byte buffer: frame t at lead + t*stride, rows of `pitch`
    bytes; the padding holds `fill`, which a mask must not count."""
    n, H = frames.shape[:2]
    rows = frames.reshape(n, H, -1)
    buf = np.full(lead + n * stride + 8, fill, np.uint8)
    for t in range(n):
        for y in range(H):
            o = lead + t * stride + y * pitch
            buf[o:o + rows.shape[2]] = rows[t, y]
    return buf


def _want(names, W, H, B, ps):
    return [RC.expected(k, c, W, H, B, ps) for k, c in names]


@pytest.mark.parametrize("ps", [0, 1])
@pytest.mark.parametrize("B", RC.BLOCKS)
@pytest.mark.parametrize("W,H", RC.SHAPES)
def test_every_mask_and_content(N, W, H, B, ps):
    """The four masks with the three contents as one batch of packed host frames;
    the identities against dvc_quality_compare on the same handle, and that call
    after a regions call still gives its old record."""
    ref, test, masks, names = RC.batch(W, H, B)
    m = N.QualityMeter(W, H, max_batch=len(names))
    try:
        before = m.compare(ref, test)
        got = m.compare_regions(ref, test, masks, B, ps)
        after = m.compare(ref, test)
    finally:
        m.close()
    assert got.dtype == RR.REGIONS and not got["reserved"].any()
    assert [RR.as_tuple(r) for r in got] == _want(names, W, H, B, ps)
    assert [RR.folded(RR.as_tuple(r)) for r in got] == [tuple(C.as_tuple(r)) for r in before]
    assert np.array_equal(before, after)
    assert [tuple(C.as_tuple(r)) for r in after] == [C.expected(c, W, H) for _, c in names]


@pytest.mark.parametrize("B,ps", [(5, 1), (8, 0), (128, 1)])
@pytest.mark.parametrize("W,H", RC.SHAPES)
def test_host_pointers_pitch_and_stride(N, W, H, B, ps):
    """A mask pitch of W + 3 and frame pitches of 3 W + 5 (rows that are not 4-byte
    aligned take the byte loads), frames 13 bytes apart; the padding is not 0."""
    ref, test, masks, names = RC.batch(W, H, B)
    ref, test, masks, names = ref[3:9], test[3:9], masks[3:9], names[3:9]
    fp, mp = 3 * W + 5, W + 3
    fs, ms = fp * H + 13, mp * H + 13
    ba, bb, bm = _laid_out(ref, fp, fs), _laid_out(test, fp, fs), _laid_out(masks, mp, ms)
    h = _handle(N, W, H, 6)
    try:
        for n in (6, 1):
            out = np.zeros(n, RR.REGIONS)
            N.check(N.lib().dvc_quality_compare_regions(h, ba.ctypes.data, fp, fs, bb.ctypes.data, fp, fs, bm.ctypes.data,
                                                        mp, ms, B, ps, n, out.ctypes.data))
            assert [RR.as_tuple(r) for r in out] == _want(names[:n], W, H, B, ps)
    finally:
        N.lib().dvc_quality_destroy(h)


@pytest.mark.parametrize("pad,gap,lead", [(0, 0, 0), (3, 13, 1), (4, 8, 0)])
@pytest.mark.parametrize("B,ps", [(1, 0), (5, 0), (8, 1), (16, 1)])
@pytest.mark.parametrize("W,H", [(11, 13), (130, 34), (264, 72)])
def test_device_pointers_on_a_callers_stream(N, W, H, B, ps, pad, gap, lead):
    """Device frames and masks at any pitch, stride and alignment, read in place,
    asynchronous on the caller's stream; a second call with other masks into the
    same records, and the whole-frame call between the two."""
    import torch
    ref, test, masks, names = RC.batch(W, H, B)
    sel = [2, 6, 7, 9]                                        # zero, random, random, corner
    ref, test, masks, names = ref[sel], test[sel], masks[sel], [names[i] for i in sel]
    fp, mp = 3 * W + pad, W + pad
    fs, ms = fp * H + gap, mp * H + gap
    s = torch.cuda.Stream()
    h = _handle(N, W, H, 4, ctypes.c_void_p(s.cuda_stream), N.DVC_FLAG_DEVICE_PTRS)
    try:
        with torch.cuda.stream(s):
            da = torch.from_numpy(_laid_out(ref, fp, fs, lead)).to("cuda")
            db = torch.from_numpy(_laid_out(test, fp, fs, lead)).to("cuda")
            dm = torch.from_numpy(_laid_out(masks, mp, ms, lead)).to("cuda")
            rm = torch.from_numpy(_laid_out(masks[::-1], mp, ms, lead)).to("cuda")
            res = torch.full((4 * RR.REGIONS.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
            whole = torch.full((4 * R.FRAME.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
            frames = (da.data_ptr() + lead, fp, fs, db.data_ptr() + lead, fp, fs)
            N.check(N.lib().dvc_quality_compare_regions(h, *frames, dm.data_ptr() + lead, mp, ms, B, ps, 4,
                                                        res.data_ptr()))
            first = res.cpu().numpy().view(RR.REGIONS).copy()
            N.check(N.lib().dvc_quality_compare(h, *frames, 4, whole.data_ptr()))
            N.check(N.lib().dvc_quality_compare_regions(h, *frames, rm.data_ptr() + lead, mp, ms, B, ps, 3,
                                                        res.data_ptr()))
        N.check(N.lib().dvc_quality_sync(h))
        second = res.cpu().numpy().view(RR.REGIONS)
        assert [RR.as_tuple(r) for r in first] == _want(names, W, H, B, ps)
        assert [tuple(C.as_tuple(r)) for r in whole.cpu().numpy().view(R.FRAME)] == [C.expected(c, W, H) for _, c in names]
        swapped = [RR.frame(ref[t], test[t], masks[3 - t], B, ps) for t in range(3)]
        assert [RR.as_tuple(r) for r in second[:3]] == swapped
        assert RR.as_tuple(second[3]) == RR.as_tuple(first[3])            # n = 3 leaves the fourth record alone
    finally:
        N.lib().dvc_quality_destroy(h)


@pytest.mark.parametrize("max_batch", [2, 4])
def test_three_masks_on_handles_of_two_and_four(N, max_batch):
    """n = 3 with three different masks: one call with frame strides on a handle of 4,
    two calls (2 + 1) on a handle of 2; masks taken in place from a wider array."""
    W, H, B = 130, 34, 5
    names = [("random", "noise"), ("corner", "noise"), ("full", "noise")]
    a, b = C.pair("noise", W, H)
    ref, test = np.stack([a, a, a]), np.stack([b, b, b])
    wide = np.full((3, H + 1, W + 7), 9, np.uint8)
    wide[:, :H, 3:W + 3] = np.stack([RC.mask(k, W, H, B) for k, _ in names])
    view = wide[:, :H, 3:W + 3]
    assert not view.flags.c_contiguous
    m = N.QualityMeter(W, H, max_batch=max_batch)
    try:
        for ps in (0, 1):
            assert [RR.as_tuple(r) for r in m.compare_regions(ref, test, view, B, ps)] == _want(names, W, H, B, ps)
        with pytest.raises(ValueError):
            m.compare_regions(ref, test, view[:2], B, 1)
        with pytest.raises(ValueError):
            m.compare_regions(ref, test, view[:, :, :-1], B, 1)
    finally:
        m.close()


def test_refusals(N):
    W, H = 12, 9
    a, b = C.pair("noise", W, H)
    a3, b3, m3 = np.stack([a, a, a]), np.stack([b, b, b]), np.zeros((3, H, W), np.uint8)
    out = np.zeros(3, RR.REGIONS)
    cmp_ = N.lib().dvc_quality_compare_regions
    h = _handle(N, W, H, 2)
    try:
        fr = (a3.ctypes.data, 3 * W, 3 * W * H, b3.ctypes.data, 3 * W, 3 * W * H)
        mk = (m3.ctypes.data, W, W * H)
        o = out.ctypes.data
        for block in (0, -1, 129):
            assert cmp_(h, *fr, *mk, block, 1, 1, o) == N.DVC_E_INVALID
        for ps in (-1, 2):
            assert cmp_(h, *fr, *mk, 8, ps, 1, o) == N.DVC_E_INVALID
        assert cmp_(h, *fr, m3.ctypes.data, W - 1, W * H, 8, 1, 1, o) == N.DVC_E_INVALID      # mask_pitch < W
        assert cmp_(h, *fr, m3.ctypes.data, W, W * H - 1, 8, 1, 2, o) == N.DVC_E_INVALID      # masks overlap
        assert cmp_(h, a3.ctypes.data, 3 * W - 1, 3 * W * H, *fr[3:], *mk, 8, 1, 1, o) == N.DVC_E_INVALID
        for n in (0, 3):
            assert cmp_(h, *fr, *mk, 8, 1, n, o) == N.DVC_E_INVALID
        assert cmp_(h, None, *fr[1:], *mk, 8, 1, 1, o) == N.DVC_E_INVALID
        assert cmp_(h, *fr[:3], None, *fr[4:], *mk, 8, 1, 1, o) == N.DVC_E_INVALID
        assert cmp_(h, *fr, None, W, W * H, 8, 1, 1, o) == N.DVC_E_INVALID
        assert cmp_(h, *fr, *mk, 8, 1, 1, None) == N.DVC_E_INVALID
        assert not out.view(np.uint8).any()
        N.check(cmp_(h, *fr, *mk, 128, 0, 2, o))                                              # the handle still works
        assert [RR.as_tuple(r) for r in out[:2]] == [RR.frame(a, b, m3[0], 128, 0)] * 2
    finally:
        N.lib().dvc_quality_destroy(h)
    hd = _handle(N, W, H, 2, None, N.DVC_FLAG_DEVICE_PTRS)
    try:   # device pointers: the records are 8-byte aligned (refused before anything is read)
        assert cmp_(hd, *fr, *mk, 8, 1, 1, out.ctypes.data + 4) == N.DVC_E_INVALID
    finally:
        N.lib().dvc_quality_destroy(hd)


# ---- end to end: the pixels the report calls static are the ones the workers flattened ------

# 64x48 x 12 frames, seed 0. On the CPU oracle (the same bytes) this clip gives, with the OF
# driver, kept and static pixels in every one of the 11 frames; with the FD driver's defaults
# (min_area 500 on so small a frame) frames that are all kept and, from output frame 8 on,
# frames that are all static; with FD_BOTH kept and static pixels in output frames 6..10.
SOURCE = "synthetic://64x48?frames=12"
FD_BOTH = dict(block_size=8, min_area=20, kernel_size=3, release_factor=0.3)


def _not_grey(frames, static):
    """The pixels of `static` whose B, G and R differ."""
    return int((((frames[..., 0] != frames[..., 1]) | (frames[..., 1] != frames[..., 2])) & static).sum())


def _row(folder):
    with open(os.path.join(folder, "performance", "quality_regions.csv"), newline="") as f:
        rows = list(csv.DictReader(f))
    assert [r["video"] for r in rows] == ["64x48"] and int(rows[0]["frames"]) == 11
    return rows[0]


def _check_row(row, rec):
    from dvc_amd import quality
    px = rec["pixels"].sum(axis=0)
    assert float(row["static_pixel_share"]) == int(px[1]) / (11 * 64 * 48)
    assert float(row["psnr_y_kept (dB)"]) == quality.psnr(int(rec["sse"][:, 0, 3].sum()), int(px[0]))
    assert float(row["psnr_y_static (dB)"]) == quality.psnr(int(rec["sse"][:, 1, 3].sum()), int(px[1]))
    assert [int(row[k + "_windows"]) for k in ("kept", "static", "mixed")] == [int(v) for v in rec["windows"].sum(axis=0)]


def test_of_driver_static_pixels_are_grey(gpu_lib, tmp_path, monkeypatch):
    from dvc_amd import motion_compression_opt, quality_analysis
    from dvc_amd.synthetic import clip
    monkeypatch.delenv("DVC_VIDEO_SINK", raising=False)
    motion_compression_opt.process_single_video_of(SOURCE, str(tmp_path))
    quality_analysis.main(["quality_analysis", str(tmp_path), SOURCE])
    comp = np.load(os.path.join(str(tmp_path), "64x48", "compressed.npy"))
    masks = np.load(os.path.join(str(tmp_path), "64x48", "mask.npy"))
    assert comp.shape == (11, 48, 64, 3) and masks.shape[:3] == (11, 48, 64)
    static = np.stack([RR.class_map(m, 8, 0) for m in masks.reshape(11, 48, 64, -1)[..., 0]])
    assert _not_grey(comp, static) == 0
    assert any(s.any() and not s.all() for s in static)                    # a frame with both classes
    # one frame later or one block aside, static pixels are not all grey: the pairing is pinned
    assert _not_grey(comp[1:], static[:-1]) > 0 and _not_grey(comp[:, :, 8:], static[:, :, :-8]) > 0
    rec = RR.records(clip(64, 48, 12, seed=0)[1:], comp, masks.reshape(11, 48, 64, -1)[..., 0], 8, 0)
    assert np.array_equal(rec["pixels"][:, 1], static.sum(axis=(1, 2)))
    _check_row(_row(str(tmp_path)), rec)


@pytest.mark.parametrize("params", [{}, FD_BOTH], ids=["defaults", "both_classes"])
def test_fd_driver_static_pixels_are_grey(gpu_lib, tmp_path, monkeypatch, params):
    from dvc_amd import frame_differencing, quality, quality_analysis
    from dvc_amd.synthetic import clip
    monkeypatch.delenv("DVC_VIDEO_SINK", raising=False)
    frame_differencing.process_single_video_fd(SOURCE, str(tmp_path), **params)
    option = ["--fd"] + ([",".join(f"{k}={v}" for k, v in params.items())] if params else [])
    quality_analysis.main(["quality_analysis"] + option + [str(tmp_path), SOURCE])
    comp = np.load(os.path.join(str(tmp_path), "64x48", "compressed_final_video.npy"))
    masks = np.stack(list(quality.fd_static_masks(SOURCE, **params)))
    assert comp.shape == (11, 48, 64, 3) and masks.shape == (11, 48, 64)
    B = params.get("block_size", 4)
    static = np.stack([RR.class_map(m, B, 1) for m in masks])
    assert _not_grey(comp, static) == 0
    assert static.any() and not static.all()
    if params:
        assert any(s.any() and not s.all() for s in static)
        assert _not_grey(comp[:, :, B:], static[:, :, :-B]) > 0
    rec = RR.records(clip(64, 48, 12, seed=0)[1:], comp, masks, B, 1)
    _check_row(_row(str(tmp_path)), rec)
    with pytest.raises(ValueError):
        next(quality.fd_static_masks(SOURCE, scale_factor=0.5))
