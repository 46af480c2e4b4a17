"""The accumulated-mask recurrence (fd:107) over its accepted parameter range, on
the CPU: the oracle's addWeighted against an independent float64 model
(tests/acc_ref.py) for every row of tests/acc_cases.py; k_acc's short-form
predicate and its exactness argument executed on the host
(tools/acc_fast_host_check.cc compiles csrc/fd_kernels.h); and the conditions the
GPU tests' clip (test_acc_gpu.py) has to meet, checked with the oracle alone."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import acc_cases as C
from tests import acc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------ oracle vs model ----
@pytest.mark.parametrize("row", C.ROWS, ids=lambda r: r.name)
def test_oracle_add_weighted_equals_model(oracle_lib, row):
    """All 256 x {0, 255} inputs, bit-exact; NaN sums give 0 in both."""
    acc = np.tile(np.arange(256, dtype=np.uint8), 2)
    dil = np.repeat(np.array([0, 255], np.uint8), 256)
    al, be, ga = C.weights(row)
    got = oracle_lib.add_weighted(acc, al, dil, be, ga)
    want = acc_ref.add_weighted(acc, dil, row.alpha, row.beta, row.gamma)
    assert np.array_equal(got, want), (row.name, np.flatnonzero(got != want)[:8])
    if row.name in ("r_nan", "r_inf"):
        assert not want.any()


def test_model_known_answers():
    """The model itself, on values worked out by hand."""
    aw = acc_ref.add_weighted
    assert aw(1, 0, 0.5, 0.5, 0).item() == 0          # 0.5 -> 0 (half to even)
    assert aw(3, 0, 0.5, 0.5, 0).item() == 2          # 1.5 -> 2
    assert aw(1, 0, 0.51, 0.49, 0).item() == 1        # 0.51 -> 1: never decays
    assert aw(255, 255, 1.0, 1.0, 0).item() == 255    # 510 saturates
    assert aw(200, 255, 1.25, -0.25, 0).item() == 186  # 250 - 63.75 = 186.25
    assert aw(255, 0, 1.25, -0.25, 0).item() == 255   # 318.75 saturates
    assert aw(7, 255, -0.5, 1.5, 0).item() == 255 and aw(7, 0, -0.5, 1.5, 0).item() == 0
    assert aw(0, 0, 0.5, 0.5, 0.6).item() == 1 and aw(0, 0, 0.5, 0.5, 0.4).item() == 0
    assert aw(9, 255, float("nan"), 0.5, 0).item() == 0
    assert aw(0, 0, float("inf"), float("-inf"), 0).item() == 0   # 0 * inf
    assert aw(9, 255, float("inf"), float("-inf"), 0).item() == 0  # inf - inf
    seq = acc_ref.run(np.array([255], np.uint8), [np.array([0], np.uint8)] * 9, 0.3, 0.7, 0)
    # 255 * float32(0.3) = 76.500003: the float32 result is 76.5 (half an ulp is 3.8e-6), then half to even
    assert [int(a[0]) for a in seq] == [76, 23, 7, 2, 1, 0, 0, 0, 0]


def test_release_0p3_reaches_few_values():
    """Why two parameter points were not enough: from 0, release_factor 0.3 reaches
    only 49 of the 256 byte values whatever the dilated masks are."""
    row = C.BY_NAME["r0p3"]
    seen, frontier = {0}, {0}
    while frontier:
        a = np.array(sorted(frontier), np.uint8)
        nxt = set()
        for d in (0, 255):
            nxt |= set(acc_ref.add_weighted(a, np.full_like(a, d), row.alpha, row.beta, row.gamma).tolist())
        frontier = nxt - seen
        seen |= nxt
    assert len(seen) == 49


# ------------------------------------------- the predicate, executed ----
def _rocm_include():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def _build_host_check(tmp_path, name, *flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I", _rocm_include(), *flags, "-o", str(exe),
                    os.path.join(ROOT, "tools", "acc_fast_host_check.cc")], check=True)
    return exe


def _run_host_check(exe, tmp_path):
    rows = tmp_path / "rows.txt"
    rows.write_text("".join(f"{r.name} {_bits(r.alpha):08x} {_bits(r.beta):08x} {_bits(r.gamma):08x}\n"
                            for r in C.ROWS))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(rows)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


def _check_report(rep):
    assert rep["failures"] == 0
    assert rep["rows"] == {r.name: {"fast": int(r.fast), "acc0_fixed": int(r.acc0_fixed)} for r in C.ROWS}
    assert rep["swept"] >= len(C.ROWS) + 65537 + 96 + 23 ** 3
    # every (r, 1 - r, 0) with r in [0, 1] takes the short form: the 65537 grid points alone
    assert rep["fast"] > 65537


def test_short_form_predicate_on_the_host(tmp_path):
    """acc_fast_ok and acc_zero_fixed as the library compiles them, over the table,
    a 2^16 grid of release factors, the neighbours of 0, 0.5 and 1, special values
    in every position and raw grids: wherever the predicate holds the unclamped
    short form equals the clamped form on all 512 inputs, and the table's
    expectation columns are what the predicates give."""
    _check_report(_run_host_check(_build_host_check(tmp_path, "acc_fast_host_check"), tmp_path))


def test_short_form_predicate_under_sanitizers(tmp_path):
    """The same stand-alone program under ASan and UBSan (a float that is no byte
    value converted to an integer would be reported)."""
    exe = _build_host_check(tmp_path, "acc_fast_host_check_san", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all")
    _check_report(_run_host_check(exe, tmp_path))


# --------------------------------------- the GPU tests' clip, on the CPU ----
@pytest.fixture(scope="module")
def seeded(oracle_lib):
    """Per geometry: the oracle's dilated plane of every frame from the seeded step
    on (they do not depend on the weights)."""
    row = C.BY_NAME["r0p5"]
    return {g: [f[3] for f in C.oracle_run(oracle_lib, *g, row, C.N_FRAMES - 1)] for g in C.GEOMS}


@pytest.mark.parametrize("geom", C.GEOMS, ids=lambda g: "%dx%d-b%d" % g)
def test_clip_reaches_every_pair_and_the_partial_blocks(seeded, geom):
    W, H, B = geom
    dil, dil2 = seeded[geom][:2]
    assert set(np.unique(dil).tolist()) == {0, 255}
    seed = C.seed_plane(W, H)
    pairs = set(zip(seed.ravel().tolist(), (dil.ravel() != 0).tolist()))
    assert len(pairs) == 512
    assert dil2.any() and not dil2.all()       # frame 2: the rectangles leave, motion once more
    if W % B:                                   # the right column of partial blocks
        col = dil[:, W - W % B:]
        assert col.any() and not col.all()
        # ... with a partial block that is dilated all over and one that is not at all
        per_block = [col[y:y + B] for y in range(0, H, B)]
        assert any(b.all() for b in per_block) and any(not b.any() for b in per_block)
    if H % B:                                   # the bottom row of partial blocks
        rowp = dil[H - H % B:]
        assert rowp.any() and not rowp.all()
    # no odd block side: the run never stops at cv2.dct (fd:122)
    assert (W % B) % 2 == 0 and (H % B) % 2 == 0


@pytest.mark.parametrize("geom", C.GEOMS, ids=lambda g: "%dx%d-b%d" % g)
def test_clip_moves_only_at_its_events(seeded, geom):
    """Frame 2's dilated mask is not frame 1's; after it only the frames of
    acc_cases.EVENTS have dilated pixels, each in block rows of its own, one of
    them in every 8-frame chunk position class the kernels' load pipeline has: the
    second chunk of a launch (frames 12, 13 of a 33- or 17-frame launch; 27, 28 of
    the 16-frame launch behind it), the fourth (27, 28 of 33) and the first of the
    third trip, which is also the launch's last frame (33)."""
    W, H, B = geom
    dils = seeded[geom]
    assert not np.array_equal(dils[0], dils[1])
    rows = {}
    for t in range(3, C.N_FRAMES):
        d = dils[t - 1]
        assert d.any() == (t in C.EVENTS), t
        if t in C.EVENTS:
            rows[t] = set((np.flatnonzero(d.any(axis=1)) // B).tolist())
            assert len(rows[t]) < -(-H // B)
    assert not (rows[12] & rows[27]) and not (rows[27] & rows[33]) and not (rows[12] & rows[33])
    assert rows[12] == rows[13] and rows[27] == rows[28]


@pytest.mark.parametrize("geom", C.GEOMS, ids=lambda g: "%dx%d-b%d" % g)
@pytest.mark.parametrize("name", [r.name for r in C.ROWS if r.alpha < 0.5])
def test_clip_decay_has_static_and_moving_blocks(oracle_lib, geom, name):
    """Rows whose accumulated mask decays to 0 (alpha < 0.5): after the seeded
    step, a frame has static blocks beside blocks that are not (the static test
    and the speculative outputs both matter), a block that was not static becomes
    static, and the oracle's accumulated masks equal the model's recurrence."""
    W, H, B = geom
    row = C.BY_NAME[name]
    run = C.oracle_run(oracle_lib, W, H, B, row, C.N_FRAMES - 1)
    st = [C.static_blocks(f[2], B) for f in run]
    assert any(s.any() and not s.all() for s in st[1:])
    assert any((~st[t - 1] & st[t]).any() for t in range(2, len(st)))
    model = acc_ref.run(C.seed_plane(W, H), [f[3] for f in run], row.alpha, row.beta, row.gamma)
    for t, (f, m) in enumerate(zip(run, model)):
        assert np.array_equal(f[2], m), (name, t + 1)
    # the stats count the same static blocks
    assert run[-1][4]["static_blocks"] == sum(int(s.sum()) for s in st)
