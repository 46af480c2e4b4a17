"""GPU: the Motion-JPEG rate target (include/dvc_jpeg_rate.h; DESIGN.md "Motion-JPEG
stream", "Rate target") byte for byte against tests/mjpeg_rate_ref.py, whose
fixtures tests/test_mjpeg_rate.py checks on the CPU (monotone estimates; a miss,
interior qualities, q_max): the quality found, the DQT pair and SOS in front of
every frame, the entropy data of a fixed-quality handle at that quality, the
counters; several groups with different qualities; gray frames at an odd pitch;
segments longer than one trip of the kernels' loops; optimised tables; the
stream output; two asynchronous calls without a wait between them; a file
written at a bitrate and read back; and the drivers with the frames kept on the
device."""
import io
import os

import numpy as np
import pytest

from tests import mjpeg_opt_ref as O
from tests import mjpeg_rate_ref as RR

pytestmark = pytest.mark.gpu


def _encode(N, frames, target, lo, hi, max_batch, optimize=False):
    frames = np.stack(frames)
    with N.JpegEncoder(frames.shape[2], frames.shape[1], frames.ndim == 4, max_batch=max_batch, optimize=optimize,
                       target_bytes=target, quality_range=(lo, hi)) as enc:
        assert enc.rate_stats() == dict.fromkeys(RR.STATS, 0)
        out = enc.encode(frames)
        return enc.header, out, enc.rate_stats(), enc.bound


@pytest.mark.parametrize("target", [400, 700, 1000, 1250, 5000])
def test_search_outcomes(gpu_lib, target):
    """48x32 clean BGR, one group of three, range 1..100: a miss (400), interior qualities, q_max (5000)."""
    N = gpu_lib._native
    frames = RR.fixture("clean48x32")
    want = RR.encode(frames, target, 1, 100, 3)
    header, got, stats, bound = _encode(N, frames, target, 1, 100, 3)
    q = want["groups"][0][0]
    print(f"target {target}: reference q* {q}, E {want['groups'][0][2]}; device {stats}")
    assert stats == want["stats"]
    assert header == want["header"] and got == want["frames"]
    with N.JpegEncoder(48, 32, True, q, 3) as fixed:                     # the entropy data of a fixed-quality handle
        for g, f in zip(got, fixed.encode(np.stack(frames))):
            assert g[152:] == f and g[:138] == RR.dqt_pair(q)
    assert all(len(g) <= bound for g in got)


def test_groups_get_qualities_of_their_own(gpu_lib):
    """40x24, five frames in groups of 2, 2, 1: flat frames, then noise, 900 bytes a frame."""
    N = gpu_lib._native
    frames = RR.fixture("flat_then_noise40x24")
    want = RR.encode(frames, 900, 1, 100, 2)
    header, got, stats, _ = _encode(N, frames, 900, 1, 100, 2)
    assert stats == want["stats"] and stats["groups"] == 3 and stats["q_lowest"] < stats["q_highest"]
    assert header == want["header"] and got == want["frames"]


def test_gray_frames_at_an_odd_pitch(gpu_lib):
    """33x17 noisy gray (rows of 33 bytes), range 20..90."""
    N = gpu_lib._native
    frames = RR.fixture("gray33x17")
    want = RR.encode(frames, 700, 20, 90, 3)
    header, got, stats, _ = _encode(N, frames, 700, 20, 90, 3)
    assert stats == want["stats"] and 20 < stats["q_last"] < 90
    assert header == want["header"] and got == want["frames"]
    assert all(g[138:148] == b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" for g in got)
    # one frame at a time, from rows 40 bytes apart (dvc_jpeg_encode's pitch)
    padded = np.full((17, 40), 0x5A, np.uint8)
    padded[:, :33] = frames[1]
    one = RR.encode(frames[1:2], 700, 20, 90, 1)
    with N.JpegEncoder(33, 17, False, max_batch=1, target_bytes=700, quality_range=(20, 90)) as enc:
        out, sizes = np.zeros(enc.bound, np.uint8), np.zeros(1, np.uint32)
        N.check(N.lib().dvc_jpeg_encode(enc._h, padded.ctypes.data, 40, 40 * 17, 1, out.ctypes.data, out.size,
                                        sizes.ctypes.data))
        assert out[:int(sizes[0])].tobytes() == one["frames"][0] and enc.rate_stats() == one["stats"]


@pytest.mark.parametrize("name,target", [("wide688x16", 9000), ("tall16x48", 800)])
def test_loop_trips(gpu_lib, name, target):
    """688x16: one segment of 258 blocks, past one trip of 256; 16x48: three segments."""
    N = gpu_lib._native
    frames = RR.fixture(name)
    want = RR.encode(frames, target, 1, 100, 1)
    header, got, stats, _ = _encode(N, frames, target, 1, 100, 1)
    assert stats == want["stats"] and 1 < stats["q_last"] < 100
    assert header == want["header"] and got == want["frames"]


def test_optimised_tables_with_a_target(gpu_lib):
    """48x32, three frames: the optimised reference at the reference's q*, DQT, DQT, DHT, SOS in front."""
    N = gpu_lib._native
    frames = RR.fixture("clean48x32")
    want = RR.encode(frames, 1000, 1, 100, 3, optimize=True)
    header, got, stats, bound = _encode(N, frames, 1000, 1, 100, 3, optimize=True)
    assert stats == want["stats"] == RR.encode(frames, 1000, 1, 100, 3)["stats"]        # the estimate uses the fixed tables
    assert header == want["header"] and got == want["frames"]
    q = want["groups"][0][0]
    opt = O.encode_group([RR.ref(f, q) for f in frames])
    for g, o in zip(got, opt["frames"]):
        segs, _ = RR.segments(g)
        assert [m for m, _ in segs] == [0xDB, 0xDB, 0xC4, 0xDA] and g[138:] == o and len(g) <= bound
    # the table builder on counts of the caller's still answers, and leaves the group's prefix alone
    with N.JpegEncoder(48, 32, True, max_batch=3, optimize=True, target_bytes=1000, quality_range=(1, 100)) as enc:
        first = enc.encode(np.stack(frames))
        assert enc.tables(np.array(opt["counts"], np.uint64)) == O.dht_segment(opt["counts"])
        assert enc.encode(np.stack(frames)) == first == want["frames"]


@pytest.mark.parametrize("mode", ["host", "device"])
def test_stream_output_over_two_groups(gpu_lib, mode):
    """encode_stream: header + encode's bytes back to back, three frames in groups of 2 and 1."""
    import torch
    N = gpu_lib._native
    frames = np.stack(RR.fixture("noisy40x24"))
    want = RR.encode(frames, 1000, 1, 100, 2)
    samples = [want["header"] + f for f in want["frames"]]
    cap = sum(len(s) for s in samples) + 64
    if mode == "host":
        with N.JpegEncoder(40, 24, True, max_batch=2, target_bytes=1000, quality_range=(1, 100)) as enc:
            out, offs = np.full(cap, 0xA5, np.uint8), np.zeros(4, np.uint64)
            enc.encode_stream(frames, out, offs)
            stats = enc.rate_stats()
    else:
        st = torch.cuda.Stream()
        with N.JpegEncoder(40, 24, True, max_batch=2, target_bytes=1000, quality_range=(1, 100), device_ptrs=True,
                           stream=st.cuda_stream) as enc, torch.cuda.stream(st):
            d_in = torch.from_numpy(frames).cuda()
            d_out = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
            d_offs = torch.zeros(4, dtype=torch.int64, device="cuda")
            enc.encode_stream(d_in, d_out, d_offs)
            enc.sync()
            out, offs, stats = d_out.cpu().numpy(), d_offs.cpu().numpy(), enc.rate_stats()
    offs = [int(v) for v in offs]
    assert offs == [0] + list(np.cumsum([len(s) for s in samples]))
    assert [out[a:b].tobytes() for a, b in zip(offs, offs[1:])] == samples and (out[offs[-1]:] == 0xA5).all()
    assert stats == want["stats"] and stats["groups"] == 2


def test_two_asynchronous_calls_without_a_wait_between(gpu_lib):
    """A device-pointer handle on a joined stream: two calls with different content, one
    dvc_jpeg_sync behind both; each call's search ran on its own coefficients."""
    import torch
    N = gpu_lib._native
    a, b = np.stack(RR.fixture("noisy40x24")), np.stack(RR.fixture("flat_then_noise40x24")[:3])
    with N.JpegEncoder(40, 24, True, max_batch=3, target_bytes=900, quality_range=(1, 100)) as host:
        want = [[host.header + f for f in host.encode(x)] for x in (a, b)]
        want_stats = host.rate_stats()
    ref = [RR.encode(x, 900, 1, 100, 3) for x in (a, b)]
    assert [[r["header"] + f for f in r["frames"]] for r in ref] == want
    assert ref[0]["groups"][0][0] != ref[1]["groups"][0][0]
    st = torch.cuda.Stream()
    with N.JpegEncoder(40, 24, True, max_batch=3, target_bytes=900, quality_range=(1, 100), device_ptrs=True,
                       stream=st.cuda_stream) as enc, torch.cuda.stream(st):
        cap = enc.bound * 3 + 3 * len(enc.header)
        d_in = [torch.from_numpy(x).cuda() for x in (a, b)]
        d_out = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
        d_offs = [torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(2)]
        for k in range(2):
            enc.encode_stream(d_in[k], d_out[k], d_offs[k])
        enc.sync()
        for k in range(2):
            out, offs = d_out[k].cpu().numpy(), [int(v) for v in d_offs[k].cpu().numpy()]
            assert [out[x:y].tobytes() for x, y in zip(offs, offs[1:])] == want[k], k
        assert enc.rate_stats() == want_stats == RR.add_stats(ref[0]["stats"], ref[1]["stats"])


def test_writer_at_a_bitrate_round_trip(gpu_lib, tmp_path, caplog, monkeypatch):
    """Mp4MjpegWriter(bitrate_kbps=...) on 64x48, 12 frames in batches of 4: every sample opens in
    Pillow, the reader's GPU decoder returns Pillow's bytes, and the mean size before stuffing is
    within the target (no group is a miss, says the reference)."""
    from PIL import Image
    from dvc_amd import video_io as V
    frames = RR.fixture("clip64x48")
    kbps, fps = 320, 25
    target = V.bitrate_target_bytes(kbps, fps)
    want = RR.encode(frames, target, 10, 95, 4)
    assert target == 1600 and not want["stats"]["missed_groups"] and want["stats"]["groups"] == 3
    path = str(tmp_path / "rate.mp4")
    w = V.Mp4MjpegWriter(path, fps, (64, 48), batch=4, bitrate_kbps=kbps)
    for f in frames:
        w.write(f)
    with caplog.at_level("INFO"):
        w.release()
    assert "rate target" in caplog.text and "0 of 3 groups missed" in caplog.text
    monkeypatch.setenv("DVC_MJPEG_DECODE", "gpu")
    r = V.Mp4MjpegReader(path)
    data = open(path, "rb").read()
    samples = [data[o:o + s] for o, s in r.samples]
    assert samples == [want["header"] + f for f in want["frames"]]
    unstuffed = [len(s) - s[s.index(b"\xff\xda"):].count(b"\xff\x00") for s in samples]
    assert sum(unstuffed) == want["stats"]["est_bytes"] and sum(unstuffed) / len(unstuffed) <= target
    assert r._gpu
    for s in samples:
        im = Image.open(io.BytesIO(s))
        im.load()
        ok, got = r.read()
        assert ok and np.array_equal(got, np.asarray(im.convert("RGB"))[..., ::-1])
    assert not r.read()[0]
    r.release()


def _outputs(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".mp4"):
                out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


def test_fd_driver_at_a_bitrate_with_the_chain_on_and_off(gpu_lib, tmp_path, monkeypatch, caplog):
    """process_single_video_fd on a small Y4M with the Motion-JPEG sink at a bitrate: the files
    of a run with the frames kept on the device are those of the host path, byte for byte, and
    their frames carry quantisers of their own."""
    from dvc_amd import frame_differencing as fdm
    from dvc_amd import video_io as V
    from dvc_amd.synthetic import clip
    monkeypatch.setattr(fdm, "READ_AHEAD", 8)
    monkeypatch.setenv("DVC_VIDEO_SINK", "mjpeg")
    monkeypatch.setenv("DVC_VIDEO_BITRATE", "400")
    monkeypatch.setenv("DVC_VIDEO_QUALITY_RANGE", "5:95")
    src = str(tmp_path / "clip.y4m")
    w = V.Y4mWriter(src, 25, (96, 64))
    for f in clip(96, 64, 18, seed=5):
        w.write(f)
    w.release()
    runs = {}
    for chain in ("off", "on"):
        monkeypatch.setenv("DVC_DEVICE_CHAIN", chain)
        caplog.clear()
        with caplog.at_level("INFO"):
            fdm.process_single_video_fd(src, str(tmp_path / chain))
        runs[chain] = _outputs(str(tmp_path / chain))
        log = caplog.text
        for d, _, files in os.walk(str(tmp_path / chain)):
            if "processing.log" in files:
                log += open(os.path.join(d, "processing.log")).read()
        assert "rate target" in log
        assert ("sink=device" in log) == (chain == "on")
    assert len(runs["off"]) == 2 and sorted(runs["on"]) == sorted(runs["off"])
    for k, blob in runs["off"].items():
        assert runs["on"][k] == blob, k
        p = tmp_path / "probe.mp4"
        p.write_bytes(blob)
        r = V.Mp4MjpegReader(str(p))
        samples = [blob[o:o + s] for o, s in r.samples]
        r.release()
        assert len(samples) == 17
        hl = samples[0].index(b"\xff\xdb")
        assert all(s[hl:hl + 5] == b"\xff\xdb\x00\x43\x00" and s[hl + 69:hl + 74] == b"\xff\xdb\x00\x43\x01" for s in samples)
