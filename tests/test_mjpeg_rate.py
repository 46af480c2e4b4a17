"""CPU tests of the Motion-JPEG rate target (DESIGN.md "Motion-JPEG stream",
"Rate target"): tools/jpeg_rate_host_check.cc — csrc/jpeg_rate_core.h, the text
the rate kernels and jpeg_api.hip compile, built for the host under ASan and
UBSan — against the restatement of tests/mjpeg_rate_ref.py; the header of a
host-only rate handle and the reference's prefix, segment by segment; what
dvc_jpeg_create_rate refuses; include/dvc_jpeg_rate.h against _native's table;
the bitrate conversion and the drivers' environment; and, from the reference
alone, that every fixture of tests/test_mjpeg_rate_gpu.py is monotone and hits
the case it is there for. The search itself is a GPU kernel chain."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mjpeg_opt_ref as O
from tests import mjpeg_rate_ref as RR
from tests import mjpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the shared arithmetic under the host sanitizers ---------------------------------------------
def _search_cases():
    rng = np.random.default_rng(11)
    cases = {}

    def add(name, m, target, fixed, q_min, q_max, sums):
        assert len(sums) == q_max - q_min + 1
        cases[name] = (m, target, fixed, q_min, q_max, [int(v) for v in sums])

    mono = np.cumsum(rng.integers(1, 60, 100)) + 500
    add("mono_interior", 3, 1500, 623, 1, 100, mono)
    add("mono_miss", 3, 700, 623, 1, 100, mono)                       # E(q_min) over the budget
    add("mono_all_fit", 3, 10 ** 6, 623, 1, 100, mono)                # q* = q_max
    add("mono_exact", 1, 623 + int(mono[41]), 623, 1, 100, mono)      # E(42) == B: it fits
    add("mono_exact_less1", 1, 622 + int(mono[41]), 623, 1, 100, mono)
    add("one_quality", 2, 900, 300, 37, 37, [400])                    # one round
    add("one_quality_miss", 2, 300, 300, 37, 37, [400])
    add("two", 1, 1000, 100, 50, 51, [800, 950])
    add("range20_90", 5, 1300, 331, 20, 90, mono[19:90])
    bumpy = mono.copy()
    bumpy[45:55] += 10 ** 6                                           # not monotone: the procedure decides, not "the largest"
    add("bumpy", 3, 10 ** 5, 623, 1, 100, bumpy)
    zig = mono + (np.arange(100) % 2) * 700
    add("zigzag", 3, 2000, 623, 1, 100, zig)
    big = (np.cumsum(rng.integers(1, 2 ** 20, 100)).astype(object) + 2 ** 33)
    add("past_2_32", 512, 2 ** 24 + 100000, 623, 1, 100, big)         # sums and budgets past 2^32
    add("past_2_32_miss", 512, 2 ** 20, 623, 1, 100, big)
    for lo, hi in ((1, 2), (1, 3), (1, 4), (1, 5), (10, 95), (99, 100), (33, 64), (33, 65)):
        n = hi - lo + 1
        s = np.cumsum(rng.integers(1, 50, n)) + 100
        for k, b in enumerate((int(s[0]) + 99, int(s[n // 2]) + 100, int(s[-1]) + 100)):
            add(f"r{lo}_{hi}_{k}", 1, b, 100, lo, hi, s)
    return cases


def test_host_program_under_sanitizers(tmp_path):
    """jpeg_rate_core.h compiled for the host with ASan and UBSan into a stand-alone
    program: the quantisers of all qualities for both base tables, every DQT pair,
    every (q_min, q_max) pair's round count, levels on either side of every
    rounding step, searches over monotone and non-monotone estimates, estimates
    past 2^32, the counters, and the proof that a coefficient fits int16."""
    exe = tmp_path / "jpeg_rate_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), os.path.join(ROOT, "tools", "jpeg_rate_host_check.cc")], check=True)
    cases = _search_cases()
    level_q = (1, 2, 3, 16, 17, 99, 254, 255)
    seg_bits = (0, 1, 7, 8, 9, 2 ** 31, 2 ** 32 - 8, 2 ** 32 - 1)
    estimates = ((3, 623, 2000), (512, 623, 2 ** 40 + 5), (1, 2 ** 32 - 1, 2 ** 63))
    text = "".join(f"levels {q}\n" for q in level_q) + "".join(f"segbytes {b}\n" for b in seg_bits)
    text += "".join(f"estimate {m} {f} {s}\n" for m, f, s in estimates)
    for name, (m, target, fixed, lo, hi, sums) in cases.items():
        text += f"search {name} {m} {target} {fixed} {lo} {hi} {' '.join(map(str, sums))}\n"
    text += "stats\n"
    (tmp_path / "cases.txt").write_text(text)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    by = {}
    for ln in lines:
        by.setdefault(ln[0], []).append(ln[1:])

    # a coefficient fits int16: the bound from the matrix's row sums, restated
    M = R._dct_int_matrix()
    worst = int(np.abs(M).sum(axis=1).max())
    bound = (((128 * worst + 512) >> 10) * worst + 32768 >> 16) + 1
    assert [int(by["range"][0][0])] == [bound] and bound < 2 ** 15

    base = RR.base_tables()
    want = {(t, q): RR.quant(base[t], q) for t in (0, 1) for q in range(1, 101)}
    assert {(int(v[0]), int(v[1])): [int(x) for x in v[2:]] for v in by["quant"]} == want
    assert {int(v[0]): bytes.fromhex(v[1]) for v in by["dqt"]} == {q: RR.dqt_pair(q) for q in range(1, 101)}
    assert {int(v[0]): [int(x) for x in v[1:]] for v in by["rounds"]} == \
        {lo: [RR.rounds(lo, hi) for hi in range(lo, 101)] for lo in range(1, 101)}
    assert max(RR.rounds(lo, hi) for lo in range(1, 101) for hi in range(lo, 101)) == RR.rounds(1, 100) == 8

    for q, v in zip(level_q, by["levels"]):
        assert int(v[0]) == q
        ac, dc = (" ".join(v[1:]).split("|")[1:])
        assert [int(x) for x in ac.split()] == [RR.level(F, q, True) for F in range(-1100, 1101)], q
        assert [int(x) for x in dc.split()] == [RR.level(F, q, False) for F in range(-1100, 1101)], q
    assert [(int(a), int(b)) for a, b in by["segbytes"]] == [(b, -(-b // 8) + 2) for b in seg_bits]
    assert [int(v[0]) for v in by["estimate"]] == [m * f + s for m, f, s in estimates]

    got = {v[0]: v[1:] for v in by["search"]}
    assert sorted(got) == sorted(cases)
    stats = dict.fromkeys(RR.STATS, 0)
    for name, (m, target, fixed, lo, hi, sums) in cases.items():
        q, miss, e, tried = RR.search(lambda x: m * fixed + sums[x - lo], m * target, lo, hi)
        head, tail = " ".join(got[name]).split("|")
        assert [int(x) for x in head.split()] == [q, miss, e, len(tried)], name
        assert [int(x) for x in tail.split()] == tried, name
        one = {"groups": 1, "frames": m, "missed_groups": miss, "est_bytes": e, "budget_bytes": m * target,
               "quality_frames": q * m, "q_lowest": q, "q_highest": q, "q_last": q}
        stats = RR.add_stats(stats, one)
    assert [int(x) for x in by["stats"][0]] == [stats[k] for k in RR.STATS]
    # the cases reach what they are for
    res = {n: RR.search(lambda x, c=c: c[0] * c[2] + c[5][x - c[3]], c[0] * c[1], c[3], c[4]) for n, c in cases.items()}
    assert res["mono_miss"][:2] == (1, 1) and res["mono_all_fit"][:2] == (100, 0) and 1 < res["mono_interior"][0] < 100
    assert res["mono_exact"][0] == 42 and res["mono_exact_less1"][0] == 41
    assert res["one_quality"][3] == [37] and res["one_quality_miss"][:2] == (37, 1)
    m, target, fixed, lo, hi, sums = cases["bumpy"]
    largest = max(q for q in range(1, 101) if m * fixed + sums[q - 1] <= m * target)
    assert res["bumpy"][0] != largest                       # the procedure is the definition
    assert res["past_2_32"][2] > 2 ** 32 and res["past_2_32"][1] == 0 and res["past_2_32_miss"][1] == 1


# ---- bytes -----------------------------------------------------------------------------------------
def _rate_header(W, H, fmt, flags=0, target=1000, lo=10, hi=95):
    from dvc_amd import _native as N
    L, h, n = N.lib(), ctypes.c_void_p(), ctypes.c_size_t()
    N.check(L.dvc_jpeg_create_rate(W, H, fmt, target, lo, hi, 1, -1, None, flags, ctypes.byref(h)))
    try:
        N.check(L.dvc_jpeg_header(h, None, 0, ctypes.byref(n)))
        buf = (ctypes.c_uint8 * n.value)()
        N.check(L.dvc_jpeg_header(h, buf, n.value, ctypes.byref(n)))
        st = (ctypes.c_uint64 * 9)()
        assert L.dvc_jpeg_rate_stats(h, st) == N.DVC_E_STATE            # no device
        return bytes(buf)
    finally:
        L.dvc_jpeg_destroy(h)


@pytest.mark.parametrize("fmt,W,H", [(R.FMT_BGR, 48, 32), (R.FMT_GRAY, 33, 17), (R.FMT_BGR, 1920, 1080)])
def test_host_only_rate_handle_returns_the_header_without_dqt_and_sos(fmt, W, H):
    from dvc_amd import _native as N
    fixed = R.header_bytes(W, H, fmt, 75)
    hdr = _rate_header(W, H, fmt)
    assert hdr == RR._strip(fixed, (0xDB, 0xDA))
    assert R.parse_header(hdr)["order"] == ["SOI", "APP0", "SOF0", "DHT", "DHT", "DRI"]
    opt = _rate_header(W, H, fmt, N.DVC_FLAG_JPEG_OPT_HUFFMAN)
    assert opt == RR._strip(fixed, (0xDB, 0xDA, 0xC4))
    assert R.parse_header(opt)["order"] == ["SOI", "APP0", "SOF0", "DRI"]
    # the range does not show in the header
    assert _rate_header(W, H, fmt, lo=1, hi=100, target=5) == hdr


@pytest.mark.parametrize("name,optimize", [("clean48x32", False), ("gray33x17", False), ("clean48x32", True)])
def test_reference_sample_is_a_permutation_of_the_fixed_sample_s_segments(name, optimize):
    """header + frame: the segments of the fixed-quality sample at q* in another order,
    the entropy data byte for byte; with optimised tables the group's DHT and the
    optimised reference's data. Pillow reads it."""
    import io
    from PIL import Image
    frames = RR.fixture(name)
    lo, hi = (20, 90) if name == "gray33x17" else (1, 100)
    target = RR.estimate(frames, 60) // len(frames)
    g = RR.encode(frames, target, lo, hi, 3, optimize)
    q = g["groups"][0][0]
    assert g["groups"] == [(q, 0, RR.estimate(frames, q), 3)] and 55 <= q <= 65
    nc = 1 if name == "gray33x17" else 3
    for f, payload in zip(frames, g["frames"]):
        fixed = RR.ref(f, q)
        segs, data = RR.segments(payload)
        assert [m for m, _ in segs] == ([0xDB, 0xDB, 0xC4, 0xDA] if optimize else [0xDB, 0xDB, 0xDA])
        assert [s[4] for _, s in segs[:2]] == [0, 1] and all(len(s) == 69 for _, s in segs[:2])
        assert len(payload) - len(data) == (len(RR.dqt_pair(q)) + len(O.sos_segment(nc)) + (len(segs[2][1]) if optimize
                                                                                              else 0))
        assert len(payload) - len(data) <= RR.PREFIX_MAX and len(RR.dqt_pair(q)) + 8 + 2 * nc == (148 if nc == 1 else 152)
        hsegs, rest = RR.segments(g["header"][2:])
        assert rest == b""
        fsegs, frest = RR.segments(fixed["jpeg"][2:])
        if optimize:
            assert sorted(s for m, s in hsegs + segs if m not in (0xC4, 0xDA)) == \
                sorted(s for m, s in fsegs if m not in (0xC4, 0xDA))
        else:
            assert sorted(s for _, s in hsegs + segs) == sorted(s for _, s in fsegs)
            assert data == frest == fixed["stream"]
        im = Image.open(io.BytesIO(g["header"] + payload))
        im.load()
        want = Image.open(io.BytesIO(fixed["jpeg"]))
        want.load()
        assert np.array_equal(np.asarray(im), np.asarray(want))


def test_prefix_bound():
    from dvc_amd import _native as N
    assert N.JPEG_RATE_PREFIX_MAX == RR.PREFIX_MAX == 572 == 138 + N.JPEG_OPT_PREFIX_MAX
    src = open(os.path.join(ROOT, "include", "dvc_jpeg_rate.h")).read()
    assert "#define DVC_JPEG_RATE_PREFIX_MAX (138 + DVC_JPEG_OPT_PREFIX_MAX)" in src


# ---- the C-ABI -------------------------------------------------------------------------------------
def test_create_rate_refuses_what_the_header_says():
    from dvc_amd import _native as N
    L = N.lib()

    def rc(W=48, H=32, fmt=R.FMT_BGR, target=1000, lo=10, hi=95, mb=1, flags=0):
        h = ctypes.c_void_p()
        code = L.dvc_jpeg_create_rate(W, H, fmt, target, lo, hi, mb, -1, None, flags, ctypes.byref(h))
        if code == N.DVC_OK:
            L.dvc_jpeg_destroy(h)
        else:
            assert not h.value
        return code

    assert rc() == N.DVC_OK
    assert rc(target=0) == N.DVC_E_INVALID
    for lo, hi in ((0, 95), (10, 101), (60, 59), (-5, 5), (101, 101)):
        assert rc(lo=lo, hi=hi) == N.DVC_E_INVALID, (lo, hi)
    for lo, hi in ((1, 100), (1, 1), (100, 100), (37, 37)):
        assert rc(lo=lo, hi=hi) == N.DVC_OK, (lo, hi)
    assert rc(W=0) == N.DVC_E_INVALID and rc(H=70000) == N.DVC_E_INVALID and rc(fmt=7) == N.DVC_E_INVALID
    assert rc(mb=-1) == N.DVC_E_INVALID and rc(mb=513) == N.DVC_E_INVALID
    assert rc(target=1) == N.DVC_OK                 # too small a target is not refused: every group is a miss
    assert rc(target=2 ** 40, flags=N.DVC_FLAG_JPEG_OPT_HUFFMAN | N.DVC_FLAG_DEVICE_PTRS) == N.DVC_OK
    assert L.dvc_jpeg_create_rate(48, 32, R.FMT_BGR, 1000, 10, 95, 1, -1, None, 0, None) == N.DVC_E_INVALID
    # a fixed-quality handle has no counters
    h, st = ctypes.c_void_p(), (ctypes.c_uint64 * 9)()
    N.check(L.dvc_jpeg_create(48, 32, R.FMT_BGR, 75, 1, -1, None, 0, ctypes.byref(h)))
    try:
        assert L.dvc_jpeg_rate_stats(h, st) == N.DVC_E_STATE
        assert L.dvc_jpeg_rate_stats(h, None) == N.DVC_E_INVALID and L.dvc_jpeg_rate_stats(None, st) == N.DVC_E_INVALID
    finally:
        L.dvc_jpeg_destroy(h)


def test_abi_declares_the_rate_calls():
    """include/dvc_jpeg_rate.h, a header of its own over dvc.h, against
    _native.JPEG_RATE_SIGNATURES: dvc.h's prototypes and _native.EXPORTS are pinned,
    so they are as they were, and the ABI is still 10."""
    from dvc_amd import _native as N
    from tests import test_host as TH
    src = open(os.path.join(ROOT, "include", "dvc_jpeg_rate.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert '#include "dvc.h"' in code
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(dvc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code):
        protos[name] = [TH._c_class(ret, False)] + [TH._c_class(p, True) for p in params.split(",")]
    assert list(protos) == list(N.JPEG_RATE_SIGNATURES) == ["dvc_jpeg_create_rate", "dvc_jpeg_rate_stats"]
    assert TH._signature_mismatches(protos, N.JPEG_RATE_SIGNATURES) == []
    assert protos["dvc_jpeg_create_rate"] == ["i32", "i32", "i32", "i32", "u64", "i32", "i32", "i32", "i32", "ptr", "u32",
                                              "ptr"]
    assert protos["dvc_jpeg_rate_stats"] == ["i32", "ptr", "ptr"]
    assert not set(N.JPEG_RATE_SIGNATURES) & set(N.EXPORTS)
    assert N.ABI_VERSION == 10 and "#define DVC_ABI_VERSION 10" in open(os.path.join(ROOT, "include", "dvc.h")).read()
    body = re.search(r"struct\s+dvc_jpeg_rate_stats\s*\{(.*?)\}\s*;", code, re.S).group(1)
    fields = [d.split() for d in body.split(";") if d.strip()]
    assert [f[-1] for f in fields] == list(N.JPEG_RATE_STATS) == list(RR.STATS)
    assert all(f[:-1] == ["uint64_t"] for f in fields)
    for name in N.JPEG_RATE_SIGNATURES:
        assert hasattr(N.lib(), name)


def test_encoder_without_the_rate_calls_says_unsupported(monkeypatch):
    """An older library (an A/B run) lacks the entry points: the class raises, nothing falls back."""
    from dvc_amd import _native as N

    class Old:
        def __getattr__(self, name):
            if name in N.JPEG_RATE_SIGNATURES:
                raise AttributeError(name)
            return getattr(N._lib, name)

    N.lib()
    monkeypatch.setattr(N, "lib", lambda: Old())
    with pytest.raises(N.DvcError) as e:
        N.JpegEncoder(48, 32, device=-1, target_bytes=1000)
    assert e.value.code == N.DVC_E_UNSUPPORTED


def test_host_only_encoder_takes_a_target():
    from dvc_amd import _native as N
    enc = N.JpegEncoder(48, 32, device=-1, target_bytes=1000, quality_range=(20, 90), optimize=True)
    try:
        assert enc.quality is None and enc.target_bytes == 1000 and enc.quality_range == (20, 90)
        assert enc.header == _rate_header(48, 32, R.FMT_BGR, N.DVC_FLAG_JPEG_OPT_HUFFMAN)
        n = ctypes.c_size_t()
        N.check(N.lib().dvc_jpeg_bound(48, 32, R.FMT_BGR, ctypes.byref(n)))
        assert enc.bound == n.value + N.JPEG_RATE_PREFIX_MAX
    finally:
        enc.close()
    enc = N.JpegEncoder(48, 32, quality=60, device=-1)
    assert enc.quality == 60 and enc.target_bytes is None
    enc.close()
    with pytest.raises(N.DvcError):
        N.JpegEncoder(48, 32, device=-1, target_bytes=1000, quality_range=(60, 50))


# ---- the drivers' side -----------------------------------------------------------------------------
def test_bitrate_to_bytes():
    from dvc_amd import video_io as V
    assert V.bitrate_target_bytes(2000, 25) == 10000            # 2 Mbit/s at 25 fps
    assert V.bitrate_target_bytes(1, 30) == 4                   # 125 / 30 rounds down
    assert V.bitrate_target_bytes(0.001, 60) == 1               # never 0: that would be refused
    assert V.bitrate_target_bytes(8000, 29.97) == int(8000 * 125 / 29.97)


class _Stub:
    header = b""
    seen = []

    def __init__(self, width, height, is_color=True, quality=75, max_batch=8, device=0, optimize=False, **kw):
        _Stub.seen.append((width, height, is_color, quality, max_batch, optimize, kw))

    def encode(self, frames):
        return [b""] * len(frames)


@pytest.fixture
def stub(tmp_path, monkeypatch):
    from dvc_amd import _native, video_io
    _Stub.seen = []
    monkeypatch.setattr(_native, "JpegEncoder", _Stub)
    monkeypatch.setattr(video_io, "cv2", None)
    monkeypatch.setenv("DVC_VIDEO_SINK", "mjpeg")
    for name in ("DVC_VIDEO_BITRATE", "DVC_VIDEO_QUALITY_RANGE", "DVC_VIDEO_HUFFMAN", "DVC_VIDEO_QUALITY"):
        monkeypatch.delenv(name, raising=False)
    return video_io


def test_open_sink_without_a_bitrate_is_as_before(stub, tmp_path):
    w = stub.open_sink(str(tmp_path / "a.mp4"), 25.0, (32, 16))
    assert _Stub.seen == [(32, 16, True, 75, 8, False, {})]      # no new keyword reaches the encoder
    assert w.target_bytes is None
    w.release()


def test_open_sink_hands_the_bitrate_to_the_encoder(stub, tmp_path, monkeypatch):
    monkeypatch.setenv("DVC_VIDEO_BITRATE", "800")
    w = stub.open_sink(str(tmp_path / "a.mp4"), 25.0, (32, 16))
    assert _Stub.seen[-1] == (32, 16, True, 75, 8, False, {"target_bytes": 4000, "quality_range": (10, 95)})
    w.release()
    monkeypatch.setenv("DVC_VIDEO_QUALITY_RANGE", "30:80")
    monkeypatch.setenv("DVC_VIDEO_HUFFMAN", "optimized")
    monkeypatch.setenv("DVC_VIDEO_BITRATE", "1.5")
    w = stub.open_sink(str(tmp_path / "b.mp4"), 30.0, (32, 16), is_color=False)
    assert _Stub.seen[-1] == (32, 16, False, 75, 8, True, {"target_bytes": 6, "quality_range": (30, 80)})
    w.release()
    w = stub.Mp4MjpegWriter(str(tmp_path / "c.mp4"), 50.0, (32, 16), batch=3, bitrate_kbps=400, quality_range=(5, 50))
    assert _Stub.seen[-1] == (32, 16, True, 75, 3, False, {"target_bytes": 1000, "quality_range": (5, 50)})
    w.release()


@pytest.mark.parametrize("value", ["", "fast", "0", "-3", "nan", "inf", "1e999"])
def test_open_sink_refuses_a_bitrate_that_is_no_positive_number(stub, tmp_path, monkeypatch, value):
    monkeypatch.setenv("DVC_VIDEO_BITRATE", value)
    with pytest.raises(ValueError, match="DVC_VIDEO_BITRATE"):
        stub.open_sink(str(tmp_path / "a.mp4"), 25.0, (32, 16))


@pytest.mark.parametrize("value", ["", "50", "50:", ":50", "0:50", "60:50", "10:101", "a:b", "10:95:3", "-1:5"])
def test_open_sink_refuses_a_bad_quality_range(stub, tmp_path, monkeypatch, value):
    monkeypatch.setenv("DVC_VIDEO_BITRATE", "800")
    monkeypatch.setenv("DVC_VIDEO_QUALITY_RANGE", value)
    with pytest.raises(ValueError, match="DVC_VIDEO_QUALITY_RANGE"):
        stub.open_sink(str(tmp_path / "a.mp4"), 25.0, (32, 16))


# ---- the fixtures of the GPU tests, from the reference alone ------------------------------------------
@pytest.mark.parametrize("name,lo,hi,table", [
    ("clean48x32", 1, 100, {1: 1437, 25: 2131, 50: 2882, 75: 3747, 95: 5799, 100: 8030}),
    ("noisy40x24", 1, 100, {1: 1445, 25: 2074, 50: 2626, 75: 3314, 95: 4934, 100: 6720}),
    ("gray33x17", 20, 90, {25: 1758, 50: 1988, 75: 2203}),
])
def test_estimate_is_monotone_on_the_fixtures(name, lo, hi, table):
    """E over the whole range used: never decreasing, so on these fixtures the
    procedure finds the largest quality that fits; and the recorded values."""
    frames = RR.fixture(name)
    E = [RR.estimate(frames, q) for q in range(lo, hi + 1)]
    assert all(a <= b for a, b in zip(E, E[1:]))
    assert {q: E[q - lo] for q in table} == table
    for budget in (E[0] - 1, E[0], E[len(E) // 2], E[-1] - 1, E[-1] + 5):
        q, miss, e, _ = RR.search(lambda x: E[x - lo], budget, lo, hi)
        fits = [x for x in range(lo, hi + 1) if E[x - lo] <= budget]
        assert (q, miss, e) == ((max(fits), 0, E[max(fits) - lo]) if fits else (lo, 1, E[0]))
    if name == "noisy40x24":            # what the header says about stuffing: 40 bytes in 3314 at quality 75
        assert sum(RR.ref(f, 75)["stuffed"] for f in frames) == 40


def test_targets_of_the_search_test_hit_their_cases():
    """48x32 clean, three frames a group, range 1..100: 400 is a miss, 5000 gives q_max, the others are interior."""
    frames = RR.fixture("clean48x32")
    got = {t: RR.encode(frames, t, 1, 100, 3)["groups"][0] for t in (400, 700, 1000, 1250, 5000)}
    assert got[400][:2] == (1, 1) and got[5000][:2] == (100, 0)
    qs = [got[t][0] for t in (700, 1000, 1250)]
    assert all(1 < q < 100 for q in qs) and qs == sorted(set(qs)) and not any(got[t][1] for t in (700, 1000, 1250))
    for t, (q, miss, e, m) in got.items():
        assert m == 3 and (e > 3 * t if miss else e <= 3 * t)


def test_groups_of_the_group_test_get_different_qualities():
    """40x24, flat frames then noise, groups of 2, 2, 1 at 900 bytes a frame."""
    g = RR.encode(RR.fixture("flat_then_noise40x24"), 900, 1, 100, 2)
    qs = [q for q, _, _, _ in g["groups"]]
    assert [m for _, _, _, m in g["groups"]] == [2, 2, 1] and len(set(qs)) > 1 and qs[0] == 100
    assert g["stats"]["q_lowest"] == min(qs) and g["stats"]["q_highest"] == 100 and g["stats"]["q_last"] == qs[-1]


def test_other_fixtures_are_interior():
    for name, target, lo, hi in (("gray33x17", 700, 20, 90), ("wide688x16", 9000, 1, 100), ("tall16x48", 800, 1, 100)):
        frames = RR.fixture(name)[:1] if name != "gray33x17" else RR.fixture(name)
        q, miss, e, tried = RR.search(lambda x: RR.estimate(frames, x), len(frames) * target, lo, hi)
        assert lo < q < hi and not miss, (name, q, e)
    assert R.parse_header(R.header_bytes(688, 16, R.FMT_BGR, 50))["dri"] * 6 == 258
