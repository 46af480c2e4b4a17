"""CPU: the quality meter's split into kept and static regions (DESIGN.md "Quality
metrics", "Kept and static regions"). tests/quality_regions_ref.py against the
whole-frame reference (the identities) and against answers worked by hand;
tools/quality_regions_host_check.cc — csrc/quality_core.h, the text the GPU
kernels compile, built for the host under ASan and UBSan as a stand-alone
program — against the reference on every case of the GPU test; the C-ABI's
declaration; quality.compare_videos_regions and the quality_analysis report with
a meter backed by the reference."""
import csv
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import quality_cases as C
from tests import quality_ref as R
from tests import quality_regions_cases as RC
from tests import quality_regions_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(W, H, B, ps) for W, H in RC.SHAPES for B in RC.BLOCKS for ps in (0, 1)]


@pytest.mark.parametrize("W,H", RC.SHAPES)
def test_reference_adds_up_to_the_whole_frame(W, H):
    for B in RC.BLOCKS:
        for ps in (0, 1):
            for kind in RC.MASKS:
                for content in RC.CONTENTS:
                    got = RC.expected(kind, content, W, H, B, ps)
                    sse, q, windows, pixels = C.expected(content, W, H)
                    assert RR.folded(got) == (sse, q, windows, pixels), (B, ps, kind, content)
                    assert sum(got[3]) == W * H


def test_cases_hold_what_they_are_there_for():
    # both classes and all three window classes in one frame, block edges inside cells
    sse, q, windows, pixels = RC.expected("random", "noise", 264, 72, 5, 1)
    assert min(windows) > 0 and min(pixels) > 0 and min(min(s) for s in sse) > 0
    # block 128 is partial everywhere at these shapes: partial_static decides every pixel
    for W, H in RC.SHAPES:
        assert RC.expected("zero", "noise", W, H, 128, 0)[3] == [W * H, 0]
        assert RC.expected("zero", "noise", W, H, 128, 1)[3] == [0, W * H]
    assert set(np.unique(RC.mask("random", 130, 34, 8))) == {0, 1, 128, 255}


@pytest.mark.parametrize("W,H,B", [(8, 8, 8), (11, 13, 8), (11, 13, 5), (130, 34, 16), (264, 72, 128), (264, 72, 1)])
def test_all_zero_mask_is_all_static_with_partial_static(W, H, B):
    for content in RC.CONTENTS:
        got = RC.expected("zero", content, W, H, B, 1)
        sse, q, windows, pixels = C.expected(content, W, H)
        assert got == ([[0, 0, 0, 0], sse], [0, q, 0], [0, windows, 0], [0, pixels])
        full = RC.expected("full", content, W, H, B, 1)
        assert full == ([sse, [0, 0, 0, 0]], [q, 0, 0], [windows, 0, 0], [pixels, 0])


def test_partial_blocks_are_kept_without_partial_static():
    W, H, B = 11, 13, 8
    a, b = C.pair("noise", W, H)
    sse, q, windows, pixels = RC.expected("zero", "noise", W, H, B, 0)
    assert pixels == [W * H - 64, 64]                        # the one full block is static, the rest kept
    assert np.array_equal(RR.class_map(RC.mask("zero", W, H, B), B, 0),
                          (np.arange(H)[:, None] < 8) & (np.arange(W)[None, :] < 8))
    block = R.frame(np.ascontiguousarray(a[:8, :8]), np.ascontiguousarray(b[:8, :8]))
    assert sse[1] == block[0]                                # its squared error is the 8x8 frame's
    # the windows are at (0, 0) and (0, 4): the first is the static block, the second holds both classes
    assert windows == [0, 1, 1] and q[1] == block[1] and q[0] == 0
    assert q[1] + q[2] == C.expected("noise", W, H)[1]


@pytest.mark.parametrize("W,H,B,ps,kept", [(11, 13, 8, 1, 3 * 5), (11, 13, 8, 0, 11 * 13 - 64), (130, 34, 16, 1, 2 * 2),
                                           (264, 72, 8, 1, 64), (264, 72, 8, 0, 64), (264, 72, 5, 1, 4 * 2),
                                           (264, 72, 1, 0, 1), (130, 34, 128, 1, 2 * 34)])
def test_one_byte_of_value_one_keeps_its_block(W, H, B, ps, kept):
    sse, q, windows, pixels = RC.expected("corner", "black_white", W, H, B, ps)
    assert pixels == [kept, W * H - kept]
    assert sse[0] == [65025 * kept] * 4 and sse[1] == [65025 * (W * H - kept)] * 4
    static = RR.class_map(RC.mask("corner", W, H, B), B, ps)
    assert not static[H - 1, W - 1] and static[0, 0] == (ps == 1 or (B <= W and B <= H))


def test_reference_refusals():
    a, b = C.pair("noise", 11, 13)
    m = np.zeros((13, 11), np.uint8)
    for args in ((m, 0, 1), (m, 129, 1), (m, 8, 2), (m.astype(np.int32), 8, 1), (m[:, :10], 8, 1)):
        with pytest.raises(ValueError):
            RR.frame(a, b, *args)


def test_host_program_under_sanitizers(tmp_path):
    """quality_core.h compiled for the host with ASan and UBSan into a stand-alone
    program: the reference's sixteen integers on every case of the GPU test."""
    exe = tmp_path / "quality_regions_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tools", "quality_regions_host_check.cc")], check=True)
    src = tmp_path / "in"
    src.mkdir()
    cases = [(W, H, B, ps, kind, content) for W, H, B, ps in ALL for kind in RC.MASKS for content in RC.CONTENTS]
    for i, (W, H, B, ps, kind, content) in enumerate(cases):
        a, b = C.pair(content, W, H)
        (src / f"case{i:03d}.dim").write_text(f"{W} {H} {B} {ps}\n")
        (src / f"case{i:03d}.ref").write_bytes(a.tobytes())
        (src / f"case{i:03d}.test").write_bytes(b.tobytes())
        (src / f"case{i:03d}.mask").write_bytes(RC.mask(kind, W, H, B).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines()}
    assert len(lines) == len(cases) == 576
    for i, (W, H, B, ps, kind, content) in enumerate(cases):
        sse, q, windows, pixels = RC.expected(kind, content, W, H, B, ps)
        assert lines[f"case{i:03d}"] == sse[0] + sse[1] + q + windows + pixels, (W, H, B, ps, kind, content)


def _regions_header():
    src = open(os.path.join(ROOT, "include", "dvc_quality_regions.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_abi_declares_the_regions_call():
    """The prototype and the record are declared in include/dvc_quality_regions.h, a
    header of its own over dvc.h, and bound from _native.REGION_SIGNATURES: dvc.h's
    prototypes and _native.EXPORTS are pinned (tests/test_host.py counts 55), so
    they are as they were, and the header still says ABI 10."""
    from dvc_amd import _native as N
    from tests import test_host as TH
    src, code = _regions_header()
    assert '#include "dvc.h"' in code and "fd:117-120" in src and "of:156-161" in src
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(dvc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code):
        protos[name] = [TH._c_class(ret, False)] + [TH._c_class(p, True) for p in params.split(",")]
    assert list(protos) == list(N.REGION_SIGNATURES) == ["dvc_quality_compare_regions"]
    assert TH._signature_mismatches(protos, N.REGION_SIGNATURES) == []
    assert protos["dvc_quality_compare_regions"] == ["i32"] + ["ptr", "ptr", "u64", "u64"] + ["ptr", "u64", "u64"] * 2 \
        + ["i32"] * 3 + ["ptr"]
    assert not set(N.REGION_SIGNATURES) & set(N.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "dvc.h")).read()
    assert "#define DVC_ABI_VERSION 10" in hdr and N.ABI_VERSION == 10 and "dvc_quality_regions.h" in hdr
    # the record: the header's fields in its order, the natural offsets, 112 bytes
    body = re.search(r"typedef\s+struct\s+dvc_quality_regions\s*\{(.*?)\}\s*dvc_quality_regions\s*;", code, re.S).group(1)
    fields = [re.fullmatch(r"(\w+)\s+(\w+)((?:\[\d+\])*)", d.strip()).groups() for d in body.split(";") if d.strip()]
    np_type = {"uint64_t": "<u8", "int64_t": "<i8", "uint32_t": "<u4"}
    want = [(n, np_type[t]) + ((tuple(int(v) for v in re.findall(r"\d+", dims)),) if dims else ()) for t, n, dims in fields]
    assert [tuple(f) for f in N.QUALITY_REGIONS] == want
    dt = np.dtype(N.QUALITY_REGIONS)
    assert dt == RR.REGIONS and dt.itemsize == 112
    assert list(dt.names) == ["sse", "ssim_q32", "windows", "pixels", "reserved"]
    assert [dt.fields[n][1] for n in dt.names] == [0, 64, 88, 100, 108]
    assert dt["sse"].shape == (2, 4) and dt["ssim_q32"].shape == (3,) and dt["pixels"].shape == (2,)


def test_library_exports_the_call_and_refuses_a_null_handle():
    from dvc_amd import _native as N
    N.build()
    out = np.zeros(1, N.QUALITY_REGIONS)
    buf = np.zeros(8 * 8 * 3, np.uint8)
    rc = N.lib().dvc_quality_compare_regions(None, buf.ctypes.data, 24, 192, buf.ctypes.data, 24, 192, buf.ctypes.data,
                                             8, 64, 8, 1, 1, out.ctypes.data)
    assert rc == N.DVC_E_INVALID and not out.view(np.uint8).any()
    assert N.lib().dvc_abi_version() == 10


# ---- the host derivations ---------------------------------------------------------------

def _rec(sse, q, windows, pixels):
    out = np.zeros(1, RR.REGIONS)
    out[0] = (sse, q, windows, pixels, 0)
    return out[0]


def test_region_metrics_and_empty_classes():
    from dvc_amd import quality
    m = quality.region_metrics(_rec([[10, 20, 30, 40], [0, 0, 0, 0]], [3 << 31, 5 << 32, 0], [3, 5, 0], [100, 28]))
    assert m["psnr_y_kept"] == 10 * math.log10(255.0 ** 2 * 100 / 40)
    assert m["psnr_bgr_kept"] == 10 * math.log10(255.0 ** 2 * 300 / 60)
    assert m["psnr_y_static"] == math.inf == m["psnr_bgr_static"]
    assert (m["ssim_y_kept"], m["ssim_y_static"]) == (0.5, 1.0) and math.isnan(m["ssim_y_mixed"])
    assert m["static_pixel_share"] == 28 / 128
    none = quality.region_metrics(_rec([[1, 1, 1, 1], [0, 0, 0, 0]], [1 << 32, 0, 0], [1, 0, 0], [64, 0]))
    assert math.isnan(none["psnr_y_static"]) and math.isnan(none["psnr_bgr_static"])
    assert math.isnan(none["ssim_y_static"]) and none["static_pixel_share"] == 0.0


def test_summarize_regions_pools_and_averages():
    from dvc_amd import quality
    recs = np.zeros(3, RR.REGIONS)
    recs[0] = ([[8, 0, 0, 2], [4, 4, 4, 4]], [1 << 32, 1 << 31, 0], [1, 1, 0], [30, 10], 0)
    recs[1] = ([[0, 0, 0, 6], [0, 0, 0, 0]], [3 << 31, 0, 0], [3, 0, 0], [40, 0], 0)
    recs[2] = ([[0, 0, 0, 0], [0, 0, 0, 12]], [0, 1 << 32, 1 << 30], [0, 2, 1], [0, 40], 0)
    s = quality.summarize_regions(recs)
    assert s["frames"] == 3 and s["static_pixel_share"] == 50 / 120
    assert s["psnr_y_kept"] == R.psnr(8, 70) and s["psnr_y_static"] == R.psnr(16, 50)
    assert s["psnr_bgr_kept"] == R.psnr(8, 210) and s["psnr_bgr_static"] == R.psnr(12, 150)
    assert s["ssim_y_kept"] == (1.0 + 0.5) / 2          # frames 0 and 1 have kept windows
    assert s["ssim_y_static"] == (0.5 + 0.5) / 2 and s["ssim_y_mixed"] == 0.25
    assert (s["kept_windows"], s["static_windows"], s["mixed_windows"]) == (4, 3, 1)
    empty = quality.summarize_regions(np.zeros(0, RR.REGIONS))
    assert empty["frames"] == 0 and math.isnan(empty["psnr_y_kept"]) and math.isnan(empty["static_pixel_share"])


# ---- compare_videos_regions and the report, with the reference as the meter ------------------

def _clip(n, W=24, H=16, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _degrade(frames, k=9):
    return (frames // k * k).astype(np.uint8)


def _masks(n, W=24, H=16, seed=0, block=8):
    rng = np.random.default_rng([seed, 77])
    live = rng.random((n, -(-H // block), -(-W // block))) < 0.5
    return (np.repeat(np.repeat(live, block, axis=1), block, axis=2)[:, :H, :W] * 255).astype(np.uint8)


def test_compare_videos_regions_pairs_masks_with_outputs(tmp_path):
    from dvc_amd import quality
    src, masks = _clip(12), _masks(11)
    out = _degrade(src[1:])
    np.save(tmp_path / "src.npy", src)
    np.save(tmp_path / "out.npy", out)
    np.save(tmp_path / "mask.npy", masks)
    paths = str(tmp_path / "src.npy"), str(tmp_path / "out.npy")
    rec, s = quality.compare_videos_regions(*paths, str(tmp_path / "mask.npy"), 8, 0, 1, RR.RefMeter(max_batch=4))
    want = RR.records(src[1:], out, masks, 8, 0)
    assert rec.dtype == RR.REGIONS and len(rec) == 11 and np.array_equal(rec, want)
    assert (s["frames"], s["width"], s["height"]) == (11, 24, 16)
    assert s["psnr_y_kept"] == R.psnr(int(want["sse"][:, 0, 3].sum()), int(want["pixels"][:, 0].sum()))
    assert s["psnr_bgr_static"] == R.psnr(int(want["sse"][:, 1, :3].sum()), 3 * int(want["pixels"][:, 1].sum()))
    assert s["static_pixel_share"] == int(want["pixels"][:, 1].sum()) / (11 * 24 * 16)
    # the whole-frame records of the same pairing are what the regions add up to
    whole, _ = quality.compare_videos(*paths, 1, R.RefMeter(max_batch=4))
    assert np.array_equal(rec["sse"].sum(axis=1), whole["sse"])
    assert np.array_equal(rec["ssim_q32"].sum(axis=1), whole["ssim_q32"])
    assert np.array_equal(rec["windows"].sum(axis=1), whole["windows"])
    # an iterable of masks, another offset, another block rule; the shortest stream ends the run
    rec2, s2 = quality.compare_videos_regions(*paths, iter(masks[:7]), 4, 1, 2, RR.RefMeter(max_batch=3))
    assert len(rec2) == 7 and np.array_equal(rec2, RR.records(src[2:9], out[:7], masks[:7], 4, 1))
    rec3, _ = quality.compare_videos_regions(*paths, list(masks) + list(masks), 8, 0, 1, RR.RefMeter())
    assert np.array_equal(rec3, want)


def test_compare_videos_regions_grays_three_channel_masks(tmp_path):
    from dvc_amd import quality
    src, masks = _clip(5), _masks(4)
    np.save(tmp_path / "src.npy", src)
    np.save(tmp_path / "out.npy", _degrade(src[1:]))
    colour = np.zeros(masks.shape + (3,), np.uint8)
    colour[..., 0] = masks // 255 * 5              # blue 5 alone grays to (1868 * 5 + 8192) >> 14 = 1: it counts
    colour[0, :8, :8] = (4, 0, 0)                  # blue 4 alone grays to 0: that block stays static
    masks = masks.copy()
    masks[0, :8, :8] = 0
    np.save(tmp_path / "mask.npy", colour)
    assert set(np.unique(np.stack([quality.mask_gray(f) for f in colour]))) == {0, 1}
    rec, _ = quality.compare_videos_regions(str(tmp_path / "src.npy"), str(tmp_path / "out.npy"),
                                            str(tmp_path / "mask.npy"), 8, 0, 1, RR.RefMeter())
    assert np.array_equal(rec, RR.records(src[1:], _degrade(src[1:]), masks, 8, 0))


def test_compare_videos_regions_refuses_other_sizes(tmp_path):
    from dvc_amd import quality
    np.save(tmp_path / "a.npy", _clip(3, 24, 16))
    np.save(tmp_path / "b.npy", _clip(3, 16, 24))
    np.save(tmp_path / "m.npy", _masks(3, 16, 24))
    a, b = str(tmp_path / "a.npy"), str(tmp_path / "b.npy")
    with pytest.raises(ValueError, match="sizes differ"):
        quality.compare_videos_regions(a, b, _masks(3), 8, 0, 0, RR.RefMeter())
    with pytest.raises(ValueError, match="sizes differ"):
        quality.compare_videos_regions(a, a, str(tmp_path / "m.npy"), 8, 0, 0, RR.RefMeter())
    with pytest.raises(ValueError, match="unable to open"):
        quality.compare_videos_regions(a, a, str(tmp_path / "absent.npy"), 8, 0, 0, RR.RefMeter())
    with pytest.raises(ValueError, match="scale_factor"):
        next(quality.fd_static_masks(a, scale_factor=0.5))


def _write_feed(out, name, src, masks, fd):
    """An output folder as a driver leaves it, with .npy streams for the .mp4 names."""
    from dvc_amd import frame_differencing, motion_compression_opt
    sub = out / name
    sub.mkdir(parents=True)
    comp = _degrade(src[1:])
    if fd:
        np.save(sub / "dilated_motion_mask_video.npy", src[1:])
        np.save(sub / "compressed_final_video.npy", comp)
        frame_differencing.write_execution_times(str(sub / "execution_times.txt"), len(comp), 1.5, 0.1)
    else:
        np.save(sub / "overlay.npy", src[1:])
        np.save(sub / "mask.npy", masks)
        np.save(sub / "compressed.npy", comp)
        motion_compression_opt.write_execution_times(str(sub / "execution_times.txt"), (len(comp), 1.0, 0.1),
                                                     (len(comp), 0.5, 0.05))
    return comp


def _rows(path):
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        return rd.fieldnames, {r["video"]: r for r in rd}


def test_quality_analysis_writes_the_regions_report(tmp_path, capsys):
    from dvc_amd import quality_analysis
    out, vids = tmp_path / "out", tmp_path / "videos"
    vids.mkdir()
    feeds = {"cam_fd": (_clip(7, 24, 16, 1), _masks(6, 24, 16, 1, 4), True),
             "cam_of": (_clip(5, 32, 24, 2), _masks(4, 32, 24, 2), False),
             "cam_still": (_clip(4, 16, 16, 3), np.zeros((3, 16, 16), np.uint8), False)}   # nothing moves: no kept pixel
    comps = {}
    for name, (src, masks, fd) in feeds.items():
        np.save(vids / f"{name}.npy", src)
        comps[name] = _write_feed(out, name, src, masks, fd)
    asked = []

    def fd_masks(source, **kw):
        asked.append((os.path.basename(source), kw))
        return iter(feeds["cam_fd"][1])

    # without --fd: the OF rows alone, and quality_data.csv as it always was
    quality_analysis.main(["quality_analysis", str(out), str(vids)], meter=RR.RefMeter(max_batch=3), fd_masks=fd_masks)
    data = (out / "performance" / "quality_data.csv").read_bytes()
    fields, rows = _rows(out / "performance" / "quality_regions.csv")
    assert fields == ["video", "frames", "static_pixel_share", "psnr_y_kept (dB)", "psnr_y_static (dB)",
                      "psnr_bgr_kept (dB)", "psnr_bgr_static (dB)", "ssim_y_kept", "ssim_y_static", "ssim_y_mixed",
                      "kept_windows", "static_windows", "mixed_windows"]
    assert sorted(rows) == ["cam_of", "cam_still"] and asked == []
    os.remove(out / "performance" / "quality_regions.csv")
    os.remove(out / "performance" / "quality_data.csv")

    # with --fd and parameters: the FD row too, from the masks the replay gives
    quality_analysis.main(["quality_analysis", "--fd", "block_size=4,release_factor=0.3", str(out), str(vids)],
                          meter=RR.RefMeter(max_batch=3), fd_masks=fd_masks)
    assert (out / "performance" / "quality_data.csv").read_bytes() == data
    assert asked == [("cam_fd.npy", {"block_size": 4, "release_factor": 0.3})]
    fields, rows = _rows(out / "performance" / "quality_regions.csv")
    assert sorted(rows) == ["cam_fd", "cam_of", "cam_still"]
    for name, (src, masks, fd) in feeds.items():
        want = RR.records(src[1:], comps[name], masks, 4 if fd else 8, 1 if fd else 0)
        row, px = rows[name], want["pixels"].sum(axis=0)
        assert int(row["frames"]) == len(src) - 1
        assert float(row["static_pixel_share"]) == int(px[1]) / int(px.sum())
        if name == "cam_still":      # 16x16 in blocks of 8: every pixel static, no kept or mixed window
            assert row["psnr_y_kept (dB)"] == row["psnr_bgr_kept (dB)"] == row["ssim_y_kept"] == row["ssim_y_mixed"] == ""
            assert (row["kept_windows"], row["mixed_windows"], row["static_pixel_share"]) == ("0", "0", "1.0")
        else:
            assert float(row["psnr_y_kept (dB)"]) == R.psnr(int(want["sse"][:, 0, 3].sum()), int(px[0]))
            assert float(row["psnr_bgr_kept (dB)"]) == R.psnr(int(want["sse"][:, 0, :3].sum()), 3 * int(px[0]))
        assert float(row["psnr_y_static (dB)"]) == R.psnr(int(want["sse"][:, 1, 3].sum()), int(px[1]))
        assert float(row["psnr_bgr_static (dB)"]) == R.psnr(int(want["sse"][:, 1, :3].sum()), 3 * int(px[1]))
        for k, key in enumerate(("kept", "static", "mixed")):
            assert int(row[key + "_windows"]) == int(want["windows"][:, k].sum())
            per = [int(r["ssim_q32"][k]) / (int(r["windows"][k]) * 2.0 ** 32) for r in want if r["windows"][k]]
            if per:
                assert float(row["ssim_y_" + key]) == pytest.approx(sum(per) / len(per), rel=1e-15)
            else:
                assert row["ssim_y_" + key] == ""

    # plain --fd: the driver's defaults (block 4), wherever the option stands
    asked.clear()
    quality_analysis.main(["quality_analysis", str(out), str(vids), "--fd"], meter=RR.RefMeter(), fd_masks=fd_masks)
    assert asked == [("cam_fd.npy", {})] and (out / "performance" / "quality_data.csv").read_bytes() == data
    assert sorted(_rows(out / "performance" / "quality_regions.csv")[1]) == ["cam_fd", "cam_of", "cam_still"]
    with pytest.raises(SystemExit):
        quality_analysis.main(["quality_analysis", "--fd", "blocks=4", str(out), str(vids)], meter=RR.RefMeter())


def test_quality_analysis_without_masks_writes_no_regions_report(tmp_path):
    from dvc_amd import quality_analysis
    out, vids = tmp_path / "out", tmp_path / "videos"
    vids.mkdir()
    src = _clip(5, 24, 16, 4)
    np.save(vids / "cam.npy", src)
    _write_feed(out, "cam", src, None, True)
    quality_analysis.main(["quality_analysis", str(out), str(vids)], meter=RR.RefMeter())
    assert os.path.isfile(out / "performance" / "quality_data.csv")
    assert not os.path.exists(out / "performance" / "quality_regions.csv")
    with pytest.raises(SystemExit):      # no quality data at all: as before
        quality_analysis.main(["quality_analysis", str(out), str(tmp_path)], meter=RR.RefMeter())
