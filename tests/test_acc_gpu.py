"""GPU parity of the accumulated-mask recurrence (fd:107) over the weights the
handle accepts (tests/acc_cases.py), through the C-ABI: k_acc<4>, k_acc<8> (short
and general form) and k_acc_rows against the CPU oracle and the float64 model
of tests/acc_ref.py, bit for bit.

Both workers are primed on frame 0 of acc_cases.clip and resumed with
``set_state(gray, seed)``, seed[y, x] = (x + y) & 255, so that the first step
meets all 512 (acc, dilated) pairs; frame 2 has motion once more and frames
3..33 none, so the mask only decays, but for three short events in later chunks
of a launch (acc_cases.EVENTS). The same frames go one a call, as one
33-frame launch (a third trip through the kernels' 16-frame load pipeline with a
clamped tail) and in device mode in launches of 17 and 16. test_acc.py checks on
the CPU that the clip meets these conditions.
"""
import json
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

from tests import acc_cases as C
from tests import acc_gpu_run, acc_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_GID = "%dx%d-b%d"
_refs = OrderedDict()


def _ref(oracle, geom, row, n):
    """The oracle's run, kept for the cases that follow on the same geometry and row."""
    key = (geom, row.name)
    if key not in _refs or len(_refs[key]) < n:
        _refs[key] = C.oracle_run(oracle, *geom, row, n)
        while len(_refs) > 2:
            _refs.popitem(last=False)
    return _refs[key][:n]


def _seeded(gpu_lib, geom, row, frames, **kw):
    W, H, B = geom
    N = gpu_lib._native
    w = gpu_lib.FDWorker(W, H, keep_planes=True, **kw, **C.worker_kwargs(row, B))
    try:
        # the kernel under test is the one the table says: k_acc's short or general form, or k_acc_rows
        assert w.acc_form() == ("rows" if B not in (4, 8) else "short" if row.fast else "general"), row.name
        w.prime(frames[0])
        w.set_state(w.plane(N.PLANE_GRAY), C.seed_plane(W, H))
    except BaseException:
        w.close()
        raise
    return w


def _check_model(geom, row, ref, accs):
    """The accumulated masks against the independent recurrence fed the oracle's dilated planes."""
    model = acc_ref.run(C.seed_plane(*geom[:2]), [f[3] for f in ref], row.alpha, row.beta, row.gamma)
    for t, (a, m) in enumerate(zip(accs, model)):
        assert np.array_equal(a, m), f"{row.name}: acc != float64 model at frame {t + 1}"


def _steps(gpu_lib, oracle_lib, geom, row, n):
    """One ``step`` a frame: planes, outputs and stats after every frame."""
    N = gpu_lib._native
    ref = _ref(oracle_lib, geom, row, n)
    frames = C.clip(*geom[:2])
    w = _seeded(gpu_lib, geom, row, frames)
    accs = []
    try:
        for t in range(1, n + 1):
            ov, cp = w.step(frames[t])
            rov, rcp, racc, rdil, rst = ref[t - 1]
            accs.append(w.plane(N.PLANE_ACC))
            assert np.array_equal(w.plane(N.PLANE_DILATED), rdil), f"{row.name}: dilated differs at frame {t}"
            assert np.array_equal(accs[-1], racc), f"{row.name}: acc differs at frame {t}"
            assert np.array_equal(ov, rov), f"{row.name}: overlay differs at frame {t}"
            assert np.array_equal(cp, rcp), f"{row.name}: compressed differs at frame {t}"
            assert w.stats() == rst, f"{row.name}: stats differ at frame {t}"
    finally:
        w.close()
    _check_model(geom, row, ref, accs)


@pytest.mark.parametrize("geom", C.GEOMS, ids=lambda g: _GID % g)
@pytest.mark.parametrize("row", C.ROWS, ids=lambda r: r.name)
def test_seeded_step_and_frame2(gpu_lib, oracle_lib, geom, row):
    """Every row on every geometry: the exhaustive seeded step, then frame 2."""
    _steps(gpu_lib, oracle_lib, geom, row, 2)


_DECAY = [(g, n, m) for g in C.GEOMS for n in C.DECAY
          for m in (("step", "batch33", "dev17") if g in C.MODE_GEOMS else ("step",))]


@pytest.mark.parametrize("geom,name,mode", _DECAY, ids=[f"{_GID % g}-{n}-{m}" for g, n, m in _DECAY])
def test_decay(gpu_lib, oracle_lib, geom, name, mode):
    """The seeded step, frame 2 and 31 frames of decay (with acc_cases.EVENTS).
    ``step``: a frame a call. ``batch33``: one launch of 33 frames. ``dev17``:
    device buffers, launches of 17 and 16 frames, the one-pass output stage and
    the kept mask through device memory."""
    W, H, B = geom
    row = C.BY_NAME[name]
    n = C.N_FRAMES - 1
    if mode == "step":
        _steps(gpu_lib, oracle_lib, geom, row, n)
        return
    N = gpu_lib._native
    ref = _ref(oracle_lib, geom, row, n)
    frames = C.clip(W, H)
    if mode == "batch33":
        w = _seeded(gpu_lib, geom, row, frames, max_batch=n)
        try:
            ov, cp = w.step_batch(frames[1:])
            acc, dil, st = w.plane(N.PLANE_ACC), w.plane(N.PLANE_DILATED), w.stats()
        finally:
            w.close()
    else:
        import torch
        seq = torch.from_numpy(frames).cuda()
        w = _seeded(gpu_lib, geom, row, seq, device_ptrs=True, max_batch=17, fused=False, kept_plane=True)
        try:
            dov = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
            dcp = torch.empty_like(dov)
            w.step_batch(seq[1:], dov, dcp)
            w.sync()
            acc, dil, st = w.plane(N.PLANE_ACC), w.plane(N.PLANE_DILATED), w.stats()
        finally:
            w.close()
        ov, cp = dov.cpu().numpy(), dcp.cpu().numpy()
    for t in range(n):
        assert np.array_equal(ov[t], ref[t][0]), f"{name}: overlay differs at frame {t + 1}"
        assert np.array_equal(cp[t], ref[t][1]), f"{name}: compressed differs at frame {t + 1}"
    assert np.array_equal(acc, ref[-1][2]), f"{name}: acc differs after the last frame"
    assert np.array_equal(dil, ref[-1][3]), f"{name}: dilated differs at the last frame"
    assert st == ref[-1][4]
    model = acc_ref.run(C.seed_plane(W, H), [f[3] for f in ref], row.alpha, row.beta, row.gamma)
    assert np.array_equal(acc, model[-1]), f"{name}: acc != float64 model after the last frame"


def test_short_form_equals_general_form(gpu_lib):
    """The rows that take k_acc's short form, in-process, against a fresh child
    process started with DVC_ACC_GENERAL=1 (read when a handle is created): every
    frame's overlay, compressed and accumulated mask hash equal, and every handle
    here reports the short form, every handle of the child the general form."""
    assert "DVC_ACC_GENERAL" not in os.environ
    assert all(C.BY_NAME[n].fast for n in C.SHORT_VS_GENERAL)
    short = acc_gpu_run.hashes()
    r = subprocess.run([sys.executable, "-m", "tests.acc_gpu_run"], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, DVC_ACC_GENERAL="1"), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    general = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(general) == sorted(short) and len(short) == 2 * len(C.SHORT_VS_GENERAL)
    for key in short:
        assert short[key]["forms"] == ["short", "short"], key
        assert general[key]["forms"] == ["general", "general"], key
        for what in ("acc", "overlay", "compressed"):
            assert len(short[key][what]) == C.N_FRAMES - 1
            assert short[key][what] == general[key][what], (key, what)
