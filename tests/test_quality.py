"""CPU: the quality meter's specification (DESIGN.md "Quality metrics").
tests/quality_ref.py against values worked by hand; tools/quality_host_check.cc —
csrc/quality_core.h, the text the GPU kernels compile, built for the host under
ASan and UBSan as a stand-alone program — against the reference on every shape
and content of the GPU test; the C-ABI's refusals that need no device;
quality.compare_videos and the quality_analysis report with a meter backed by
the reference."""
import csv
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import quality_cases as C
from tests import quality_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gray(v, W=8, H=8):
    """A frame whose B = G = R = v: its luma is v (1868 + 9617 + 4899 = 2^14)."""
    return np.full((H, W, 3), v, np.uint8)


def test_reference_one_window_of_constants():
    # luma 100 against 110: s1 = 6400, s2 = 7040, ss = 64 (100^2 + 110^2), s12 = 64 * 11000, so
    # vars = cov = 0 and A = 2 * 6400 * 7040 + 416, B = D = 235963, C = 6400^2 + 7040^2 + 416
    sse, q, windows, pixels = R.frame(_gray(100), _gray(110))
    assert sse == [6400, 6400, 6400, 6400] and (windows, pixels) == (1, 64)
    v = (90112416.0 * 235963.0) / (90522016.0 * 235963.0)
    assert q == int(np.rint(v * 2.0 ** 32)) and abs(q / 2.0 ** 32 - 0.995475) < 1e-6


@pytest.mark.parametrize("d", [1, 7, 255])
def test_reference_constant_difference(d):
    a = np.random.default_rng(d).integers(0, 256 - d, (13, 22, 3), dtype=np.uint8)
    sse, _, windows, pixels = R.frame(a, a + np.uint8(d))
    assert pixels == 13 * 22 and windows == 4 * 2
    assert sse[:3] == [d * d * pixels] * 3
    # the luma of (b + d, g + d, r + d) is the luma + d exactly: the weights sum to 2^14
    assert sse[3] == d * d * pixels


def test_reference_identical_frames():
    a = np.random.default_rng(0).integers(0, 256, (21, 34, 3), dtype=np.uint8)
    sse, q, windows, pixels = R.frame(a, a)
    assert sse == [0, 0, 0, 0] and windows == 4 * 7 and q == windows << 32
    assert R.psnr(sse[3], pixels) == math.inf


def test_reference_half_block_against_its_complement():
    a = _gray(0)
    a[:, :4] = 255
    sse, q, windows, pixels = R.frame(a, 255 - a)
    # s1 = s2 = 32 * 255, ss = 64 * 255^2, s12 = 0: A = C, so the value is B / D
    B, D = 2 * (0 - 8160 * 8160) + 235963, 64 * 4161600 - 2 * 8160 * 8160 + 235963
    assert (B, D) == (-132935237, 133407163)
    assert q == int(np.rint((133171616.0 * B) / (133171616.0 * D) * 2.0 ** 32))
    assert abs(q / 2.0 ** 32 + 0.9965) < 1e-4 and sse == [65025 * 64] * 4


def test_reference_refuses_small_and_unequal_frames():
    for shape in ((7, 8, 3), (8, 7, 3)):
        with pytest.raises(ValueError):
            R.frame(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8))
    with pytest.raises(ValueError):
        R.frame(_gray(0, 8, 8), _gray(0, 12, 8))


def test_host_program_under_sanitizers(tmp_path):
    """quality_core.h compiled for the host with ASan and UBSan into a stand-alone
    program: the reference's seven integers on every shape and content."""
    exe = tmp_path / "quality_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), os.path.join(ROOT, "tools", "quality_host_check.cc")],
                   check=True)
    src = tmp_path / "in"
    src.mkdir()
    cases = [(c, W, H) for c in C.CONTENTS for W, H in C.SHAPES]
    for i, (c, W, H) in enumerate(cases):
        a, b = C.pair(c, W, H)
        (src / f"case{i:03d}.dim").write_text(f"{W} {H}\n")
        (src / f"case{i:03d}.ref").write_bytes(a.tobytes())
        (src / f"case{i:03d}.test").write_bytes(b.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines()}
    assert len(lines) == len(cases)
    for i, (c, W, H) in enumerate(cases):
        sse, q, windows, pixels = C.expected(c, W, H)
        assert lines[f"case{i:03d}"] == sse + [q, windows, pixels], (c, W, H)
    # the cases hold what they are there for
    assert C.expected("black_white", 264, 256)[0][0] > 2 ** 32
    assert C.expected("identical", 11, 13)[1] == 2 << 32 and C.expected("halves", 8, 8)[1] < 0


def test_abi_declares_the_meter():
    from dvc_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "dvc.h")).read()
    for name in ("dvc_quality_create", "dvc_quality_compare", "dvc_quality_sync", "dvc_quality_destroy"):
        assert name in N.EXPORTS and name + "(" in hdr
    assert "#define DVC_ABI_VERSION 10" in hdr and N.ABI_VERSION == 10
    assert np.dtype(N.QUALITY_FRAME) == R.FRAME and R.FRAME.itemsize == 48


def test_create_refusals_need_no_device():
    from dvc_amd import _native as N
    N.build()
    h = ctypes.c_void_p()
    create = N.lib().dvc_quality_create
    assert create(7, 8, 1, 0, None, 0, ctypes.byref(h)) == N.DVC_E_UNSUPPORTED
    assert create(8, 7, 1, 0, None, 0, ctypes.byref(h)) == N.DVC_E_UNSUPPORTED
    assert create(64, 48, 0, 0, None, 0, ctypes.byref(h)) == N.DVC_E_INVALID
    assert create(64, 48, N.MAX_BATCH + 1, 0, None, 0, ctypes.byref(h)) == N.DVC_E_INVALID
    assert create(64, 48, 1, 0, None, N.DVC_FLAG_KTIMING, ctypes.byref(h)) == N.DVC_E_INVALID
    assert create(64, 48, 1, 0, None, 0, None) == N.DVC_E_INVALID
    assert h.value is None


# ---- compare_videos and the report, with the reference as the meter ------------------

def _clip(n, W=24, H=16, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _degrade(frames, k=9):
    return (frames // k * k).astype(np.uint8)


def test_compare_videos_streams_and_honours_ref_skip(tmp_path):
    from dvc_amd import quality
    src = _clip(12)
    np.save(tmp_path / "src.npy", src)
    np.save(tmp_path / "out.npy", _degrade(src[1:]))          # frame k of the output is source frame k + 1
    rec, s = quality.compare_videos(str(tmp_path / "src.npy"), str(tmp_path / "out.npy"), 1, R.RefMeter(max_batch=4))
    want = R.records(src[1:], _degrade(src[1:]))
    assert rec.dtype == R.FRAME and np.array_equal(rec, want) and len(rec) == 11
    assert (s["frames"], s["width"], s["height"]) == (11, 24, 16)
    px = 11 * 24 * 16
    assert s["psnr_y"] == R.psnr(int(want["sse"][:, 3].sum()), px)
    assert s["psnr_bgr"] == R.psnr(int(want["sse"][:, :3].sum()), 3 * px)
    assert s["psnr_y_min"] == min(R.psnr(int(r["sse"][3]), 24 * 16) for r in want) <= s["psnr_y"]
    per = [int(r["ssim_q32"]) / (int(r["windows"]) * 2.0 ** 32) for r in want]
    assert s["ssim_y"] == pytest.approx(sum(per) / 11, rel=1e-15) and s["ssim_y_min"] == min(per)
    # the wrong offset pairs unrelated noise frames, and stops at the shorter stream
    rec0, s0 = quality.compare_videos(str(tmp_path / "src.npy"), str(tmp_path / "out.npy"), 0, R.RefMeter(max_batch=4))
    assert np.array_equal(rec0, R.records(src[:11], _degrade(src[1:]))) and s0["psnr_y"] < s["psnr_y"] - 10
    rec2, _ = quality.compare_videos(str(tmp_path / "src.npy"), str(tmp_path / "out.npy"), 2, R.RefMeter(max_batch=8))
    assert len(rec2) == 10 and np.array_equal(rec2, R.records(src[2:], _degrade(src[1:11])))
    # identical streams
    _, same = quality.compare_videos(str(tmp_path / "src.npy"), str(tmp_path / "src.npy"), 0, R.RefMeter())
    assert same["psnr_y"] == math.inf and same["psnr_bgr"] == math.inf and same["ssim_y"] == 1.0 == same["ssim_y_min"]


def test_compare_videos_refuses_other_sizes(tmp_path):
    from dvc_amd import quality
    np.save(tmp_path / "a.npy", _clip(3, 24, 16))
    np.save(tmp_path / "b.npy", _clip(3, 16, 24))
    np.save(tmp_path / "mask.npy", _clip(3, 24, 16)[..., 0])
    with pytest.raises(ValueError, match="sizes differ"):
        quality.compare_videos(str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), 0, R.RefMeter())
    with pytest.raises(ValueError):
        quality.compare_videos(str(tmp_path / "a.npy"), str(tmp_path / "mask.npy"), 0, R.RefMeter())
    with pytest.raises(ValueError, match="unable to open"):
        quality.compare_videos(str(tmp_path / "a.npy"), str(tmp_path / "absent.npy"), 0, R.RefMeter())


def _write_feed(out, name, src, fd):
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
        np.save(sub / "compressed.npy", comp)
        motion_compression_opt.write_execution_times(str(sub / "execution_times.txt"), (len(comp), 1.0, 0.1),
                                                     (len(comp), 0.5, 0.05))
    return comp


def test_quality_analysis_report(tmp_path, capsys):
    from dvc_amd import performance_analysis, quality_analysis
    out, vids = tmp_path / "out", tmp_path / "videos"
    vids.mkdir()
    feeds = {"cam_fd": (_clip(7, 24, 16, 1), True), "cam_of": (_clip(5, 32, 24, 2), False)}
    comps = {}
    for name, (src, fd) in feeds.items():
        np.save(vids / f"{name}.npy", src)
        comps[name] = _write_feed(out, name, src, fd)
    (out / "unpaired").mkdir()
    np.save(out / "unpaired" / "compressed.npy", _clip(2))
    np.save(out / "unpaired" / "overlay.npy", _clip(2))

    performance_analysis.main(["performance_analysis", str(out)])
    perf_csv = out / "performance" / "performance_data.csv"
    before = perf_csv.read_bytes()
    quality_analysis.main(["quality_analysis", str(out), str(vids)], meter=R.RefMeter(max_batch=3))
    assert perf_csv.read_bytes() == before
    assert "no source named unpaired" in capsys.readouterr().out

    with open(out / "performance" / "quality_data.csv", newline="") as f:
        rd = csv.DictReader(f)
        assert rd.fieldnames == ["video", "frames", "psnr_y (dB)", "psnr_y_min (dB)", "psnr_bgr (dB)", "ssim_y",
                                 "ssim_y_min", "compressed_size_bytes", "bits_per_pixel"]
        rows = {r["video"]: r for r in rd}
    assert sorted(rows) == ["cam_fd", "cam_of"]
    for name, (src, fd) in feeds.items():
        n, H, W = comps[name].shape[:3]
        want = R.records(src[1:], comps[name])
        size = os.path.getsize(out / name / ("compressed_final_video.npy" if fd else "compressed.npy"))
        row = rows[name]
        assert int(row["frames"]) == n == len(src) - 1 and int(row["compressed_size_bytes"]) == size
        assert float(row["bits_per_pixel"]) == size * 8 / (n * W * H)
        assert float(row["psnr_y (dB)"]) == R.psnr(int(want["sse"][:, 3].sum()), n * W * H)
        assert float(row["psnr_bgr (dB)"]) == R.psnr(int(want["sse"][:, :3].sum()), 3 * n * W * H)
        assert float(row["psnr_y_min (dB)"]) == min(R.psnr(int(r["sse"][3]), W * H) for r in want)
        per = [int(r["ssim_q32"]) / (int(r["windows"]) * 2.0 ** 32) for r in want]
        assert float(row["ssim_y"]) == pytest.approx(sum(per) / n, rel=1e-15) and float(row["ssim_y_min"]) == min(per)

    # a single video as the source, and the command line's refusals
    quality_analysis.main(["quality_analysis", str(out), str(vids / "cam_of.npy")], meter=R.RefMeter())
    with open(out / "performance" / "quality_data.csv", newline="") as f:
        assert [r["video"] for r in csv.DictReader(f)] == ["cam_of"]
    for argv in (["quality_analysis", str(out)], ["quality_analysis", str(out / "absent"), str(vids)],
                 ["quality_analysis", str(out), str(tmp_path)]):
        with pytest.raises(SystemExit):
            quality_analysis.main(argv, meter=R.RefMeter())
