"""GPU: the lifecycle the six handle classes share (_native.Handle): each is
created inside ``with``, called once, closed twice and created again after the
close. The calls need no oracle; the other GPU tests compare every output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, BATCH = 64, 48, 2


@pytest.fixture(scope="module")
def frames():
    return np.random.default_rng(7).integers(0, 256, (BATCH, H, W, 3), dtype=np.uint8)


def _lifecycle(make, call):
    """``call`` on a handle inside ``with``, which closes it; a second close; the same on a new handle."""
    for _ in range(2):
        with make() as h:
            assert h._h
            call(h)
        assert h._h is None
        h.close()
        assert h._h is None


@pytest.mark.parametrize("device_ptrs", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("path", ["FDWorker", "OFWorker"])
def test_worker_lifecycle(gpu_lib, frames, path, device_ptrs):
    import torch

    def call(w):
        f0, f1 = (torch.from_numpy(f).cuda() for f in frames) if device_ptrs else frames
        w.prime(f0)
        if device_ptrs:
            a = torch.empty(w._ashape, dtype=torch.uint8, device="cuda")
            b = torch.empty(w._bshape, dtype=torch.uint8, device="cuda")
            assert w.step(f1, a, b) is None
        else:
            a, b = w.step(f1)
            assert a.shape == w._ashape and b.shape == w._bshape
        assert w.stats()["frames"] == 1

    _lifecycle(lambda: getattr(gpu_lib, path)(W, H, max_batch=BATCH, device_ptrs=device_ptrs), call)


def test_codec_lifecycle(gpu_lib, frames):
    N = gpu_lib._native
    payloads = []

    def encode(enc):
        payloads[:] = [enc.header + p for p in enc.encode(frames[:1])]
        assert len(payloads) == 1

    def decode(dec):
        out = dec.decode(payloads)
        assert len(out) == 1 and out[0].shape == (H, W, 3)

    _lifecycle(lambda: N.JpegEncoder(W, H, max_batch=BATCH), encode)
    _lifecycle(lambda: N.JpegDecoder(W, H, max_batch=BATCH), decode)


def test_quality_meter_lifecycle(gpu_lib, frames):
    def call(q):
        rec = q.compare(frames, frames)
        assert not rec["sse"].any() and (rec["pixels"] == W * H).all()

    _lifecycle(lambda: gpu_lib._native.QualityMeter(W, H, max_batch=BATCH), call)


def test_of_compressor_lifecycle(gpu_lib, frames):
    """An all-255 mask compresses no block, but the frames do not come back
    unchanged: every pixel still takes the 8-bit BGR -> YCrCb -> BGR round trip
    (of:170-171, dvc_of_compress in include/dvc.h), so only the shape is checked."""
    def call(c):
        out = c.run(frames, np.full((BATCH, H, W), 255, np.uint8))
        assert out.shape == frames.shape and out.dtype == np.uint8

    _lifecycle(lambda: gpu_lib._native.OFCompressor(W, H, max_batch=BATCH), call)
