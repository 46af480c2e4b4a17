"""bench.py --dump-outputs (CPU, no GPU): the sample written for an output
sequence is fixed by the seed and the shapes alone, covers every frame, stays
within the size budget, and small arrays are written whole."""
import os

import numpy as np


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    import torch

    import bench
    P, H, W = 7, 12, 20
    monkeypatch.setattr(bench, "DUMP_ELEMS", 2 * P * 16)       # 16 elements a frame for each of two outputs
    rng = np.random.default_rng(1)
    ov = rng.integers(0, 256, (P, H, W, 3), dtype=np.uint8)
    cp = rng.integers(0, 256, (P, H, W, 3), dtype=np.uint8)
    stats = np.array([P, 10, 3, 99], np.float64)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, {"overlay": torch.from_numpy(ov), "compressed": cp, "stats": stats})
    bench.dump_outputs(b, {"overlay": ov, "compressed": torch.from_numpy(cp), "stats": stats})
    assert sorted(os.listdir(a)) == ["compressed.npy", "overlay.npy", "stats.npy"]
    total = 0
    for f in os.listdir(a):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert np.array_equal(x, y) and x.dtype in (np.float32, np.float64)
        total += x.size
    assert total <= bench.DUMP_ELEMS + stats.size
    x = np.load(os.path.join(a, "overlay.npy"))
    assert x.shape == (P, 16)
    for j in range(P):                                          # row j holds values of frame j
        assert np.isin(x[j], ov[j]).all()
    assert np.array_equal(np.load(os.path.join(a, "stats.npy")), stats)
    # an output within its share is written whole
    monkeypatch.setattr(bench, "DUMP_ELEMS", 4 * ov.size)
    bench.dump_outputs(a, {"overlay": ov, "compressed": cp})
    assert np.array_equal(np.load(os.path.join(a, "overlay.npy")), ov.astype(np.float32))


def test_dump_budget_is_within_64_mb():
    import bench
    assert bench.DUMP_ELEMS * 4 + 4 * 8 <= 64 * 1000 * 1000
