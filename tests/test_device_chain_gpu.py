"""GPU: the drop-in drivers with frames kept on the device between the Motion-JPEG
decoder, the worker and the Motion-JPEG encoder (_dropin.DeviceChain,
``DVC_DEVICE_CHAIN``): every output video of a run with the chain ``on`` is byte for
byte the file of the run with it ``off``, the log names the ends that were on the
device, and with both ends there the bytes copied stay under what the design
allows: the compressed samples, their sizes and offsets, and the status words.
96 x 64 sources of 7 frames, READ_AHEAD 4: one frame primes, one full and one
short chunk follow."""
import os
import re

import numpy as np
import pytest

from tests import mjpeg_cam_cases as C

pytestmark = pytest.mark.gpu

W, H, FRAMES = 96, 64, 7


def _clip(n=FRAMES):
    from dvc_amd.synthetic import clip
    return clip(W, H, n, seed=5)


def _cam_samples():
    return [C.strip_dht(C.stream(W, H, "422", "row", v, content="gradient" if v % 2 else "noise")) for v in range(FRAMES)]


def _source(kind, folder):
    """Write the source; (path, [its samples' sizes] or None for raw frames)."""
    from dvc_amd import video_io
    os.makedirs(folder, exist_ok=True)
    if kind == "avi":          # a 4:2:2 camera AVI without DHT segments
        samples = _cam_samples()
        path = os.path.join(folder, "cam.avi")
        open(path, "wb").write(C.avi(samples, W, H, 25, 1))
    elif kind == "avi_cut":    # ... its fifth sample cut short: the stream ends there
        samples = _cam_samples()
        samples[4] = samples[4][:len(samples[4]) // 2]
        path = os.path.join(folder, "cut.avi")
        open(path, "wb").write(C.avi(samples, W, H, 25, 1))
    elif kind == "mjpeg":      # a raw stream whose samples switch quantisation tables after frame 3
        samples = [C.stream(W, H, "420", "row", v, quality=75 if v < 4 else 40) for v in range(FRAMES)]
        path = os.path.join(folder, "raw.mjpeg")
        open(path, "wb").write(b"".join(samples))
    elif kind in ("mp4", "mp4_18"):   # what Mp4MjpegWriter writes; 18 frames: 17 written, three table groups
        path = os.path.join(folder, "clip.mp4")
        w = video_io.Mp4MjpegWriter(path, 25, (W, H))
        for f in _clip(18 if kind == "mp4_18" else FRAMES):
            w.write(f)
        w.release()
        r = video_io.Mp4MjpegReader(path)
        samples = [b"x" * s for _, s in r.samples]
        r.release()
    else:                      # raw 4:2:0 frames
        path = os.path.join(folder, "clip.y4m")
        w = video_io.Y4mWriter(path, 25, (W, H))
        for f in _clip():
            w.write(f)
        w.release()
        return path, None
    return path, [len(s) for s in samples]


def _outputs(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            if os.path.splitext(f)[1] in (".npy", ".json", ".mp4", ".y4m"):
                p = os.path.join(d, f)
                out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _run(driver, path, out, chain, monkeypatch, caplog, **kw):
    from dvc_amd.frame_differencing import process_single_video_fd
    from dvc_amd.motion_compression_opt import process_single_video_of
    monkeypatch.setenv("DVC_DEVICE_CHAIN", chain)
    caplog.clear()
    with caplog.at_level("INFO"):
        {"fd": process_single_video_fd, "of": process_single_video_of}[driver](path, out, **kw)
    log = caplog.text
    for d, _, files in os.walk(out):
        if "processing.log" in files:
            log += open(os.path.join(d, "processing.log")).read()
    return _outputs(out), re.findall(r"device chain: source=(\w+) sink=(\w+) h2d=(\d+) d2h=(\d+)", log)


def _both(driver, kind, tmp_path, monkeypatch, caplog, ahead=4, sink="mjpeg", huffman="fixed", **kw):
    """Run off and on; the files must agree. Returns (files, the on run's chain line, sample sizes)."""
    from dvc_amd import frame_differencing as fdm
    from dvc_amd import motion_compression_opt as ofm
    monkeypatch.setattr(fdm, "READ_AHEAD", ahead)
    monkeypatch.setattr(ofm, "READ_AHEAD", ahead)
    monkeypatch.setenv("DVC_VIDEO_SINK", sink)
    monkeypatch.setenv("DVC_VIDEO_HUFFMAN", huffman)
    path, sizes = _source(kind, str(tmp_path / "src"))
    want, none = _run(driver, path, str(tmp_path / "off"), "off", monkeypatch, caplog, **kw)
    got, lines = _run(driver, path, str(tmp_path / "on"), "on", monkeypatch, caplog, **kw)
    assert none == [] and len(set(lines)) == 1, (none, lines)
    assert want and sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k
    return got, lines[0], sizes


def _up16(v):
    return (v + 15) & ~15


def _chunks(n, ahead):
    """Frame 0 primes; chunks of ``ahead`` follow."""
    return [(0, 1)] + [(a, min(a + ahead, n)) for a in range(1, n, ahead)]


def _sample_sizes(blob, tmp_path):
    from dvc_amd import video_io
    p = tmp_path / "probe.mp4"
    p.write_bytes(blob)
    r = video_io.Mp4MjpegReader(str(p))
    sizes = [s for _, s in r.samples]
    r.release()
    return sizes


@pytest.mark.parametrize("kind", ["avi", "mp4", "mjpeg", "y4m"])
@pytest.mark.parametrize("driver", ["fd", "of"])
def test_chain_on_equals_off(gpu_lib, tmp_path, monkeypatch, caplog, driver, kind):
    got, (src, snk, h2d, d2h), sizes = _both(driver, kind, tmp_path, monkeypatch, caplog)
    assert (src, snk) == ("host" if kind == "y4m" else "device", "device")
    outs = [k for k in got if k.endswith(("dilated_motion_mask_video.mp4", "compressed_final_video.mp4", "overlay.mp4",
                                          "mask.mp4"))]
    assert len(outs) == 2
    if sizes is None:
        return
    # both ends on the device: what crosses is compressed samples, sizes, offsets and status words
    up = sum((b - a) * _up16(max(sizes[a:b])) + 8 * (b - a) for a, b in _chunks(FRAMES, 4))
    assert int(h2d) <= up, (h2d, up)
    down = 0
    for k in outs:
        written = _sample_sizes(got[k], tmp_path)
        assert len(written) == FRAMES - 1
        for a, b in _chunks(FRAMES, 4)[1:]:
            n = b - a
            down += sum(written[a - 1:b - 1]) + 8 * (n + 1) + 4 * n
    assert int(d2h) <= down, (d2h, down)
    assert int(h2d) < FRAMES * W * H * 3 and int(d2h) < (FRAMES - 1) * W * H * 3      # under a raw frame a frame


@pytest.mark.parametrize("ahead,sink_end", [(4, "host"), (3, "host"), (8, "device")])
@pytest.mark.parametrize("driver", ["fd", "of"])
def test_optimised_tables_keep_their_groups(gpu_lib, tmp_path, monkeypatch, caplog, driver, ahead, sink_end):
    """The file's bytes depend on the table groups: 8 frames from frame 0. Chunks that hold whole
    groups go through the device sink; others keep the host sink, and the files agree either way.
    17 written frames: two whole groups and a partial one, in chunks of 8, 8 and 1 with READ_AHEAD 8."""
    got, (src, snk, _, _), _ = _both(driver, "mp4_18", tmp_path, monkeypatch, caplog, ahead=ahead, huffman="optimized")
    assert (src, snk) == ("device", sink_end)
    first = next(v for k, v in sorted(got.items()) if k.endswith(".mp4"))
    assert len(_sample_sizes(first, tmp_path)) == 17


@pytest.mark.parametrize("huffman,ahead", [("fixed", 4), ("optimized", 8)])
def test_samples_past_the_device_buffer_go_the_host_way(gpu_lib, tmp_path, monkeypatch, caplog, huffman, ahead):
    """A device sample buffer of 800 bytes a frame: chunks whose samples pass it are cut back to a
    table-group boundary and the rest is fetched raw and encoded by the writer's host encoder — the
    one place where raw frames cross with the chain on. The files still equal the host path's."""
    from dvc_amd import _dropin
    monkeypatch.setattr(_dropin.DeviceChain, "FRAME_CAP", 800)
    got, (src, snk, _, d2h), _ = _both("fd", "mp4_18", tmp_path, monkeypatch, caplog, ahead=ahead, huffman=huffman)
    assert (src, snk) == ("device", "device")
    sizes = _sample_sizes(got[os.path.join("clip", "compressed_final_video.mp4")], tmp_path)
    assert len(sizes) == 17 and sum(sizes[:ahead]) > 800 * ahead      # the first chunk does not fit
    assert int(d2h) > W * H * 3                                        # raw frames came down


def test_fd_scale_factor(gpu_lib, tmp_path, monkeypatch, caplog):
    got, (src, snk, _, _), _ = _both("fd", "avi", tmp_path, monkeypatch, caplog, scale_factor=0.5)
    assert (src, snk) == ("device", "device")
    assert any(k.endswith("compressed_final_video.mp4") for k in got)


def test_fd_odd_dct_stop(gpu_lib, tmp_path, monkeypatch, caplog):
    """block_size 3, and no contour large enough to count as motion, so every 3 x 3 block is static:
    the frames before the stop, then the failing frame's overlay alone, the same error logged."""
    got, (src, snk, _, _), _ = _both("fd", "mp4", tmp_path, monkeypatch, caplog, block_size=3, min_area=10 ** 6)
    assert (src, snk) == ("device", "device") and "Odd-size DCT" in caplog.text
    n = {os.path.basename(k): len(_sample_sizes(v, tmp_path)) for k, v in got.items() if k.endswith(".mp4")}
    assert n["dilated_motion_mask_video.mp4"] == n["compressed_final_video.mp4"] + 1


@pytest.mark.parametrize("driver", ["fd", "of"])
def test_a_cut_sample_ends_the_stream(gpu_lib, tmp_path, monkeypatch, caplog, driver):
    got, (src, snk, _, _), _ = _both(driver, "avi_cut", tmp_path, monkeypatch, caplog)
    assert (src, snk) == ("device", "device")
    first = next(v for k, v in sorted(got.items()) if k.endswith(".mp4"))
    assert len(_sample_sizes(first, tmp_path)) == 3          # frames 1..3; sample 4 is damaged


@pytest.mark.parametrize("sink", ["y4m", "npy"])
def test_device_source_with_a_host_sink(gpu_lib, tmp_path, monkeypatch, caplog, sink):
    _, (src, snk, _, _), _ = _both("fd", "mp4", tmp_path, monkeypatch, caplog, sink=sink)
    assert (src, snk) == ("device", "host")


def test_on_raises_when_the_source_decodes_with_pillow(gpu_lib, tmp_path, monkeypatch):
    from dvc_amd.frame_differencing import process_single_video_fd
    path, _ = _source("avi", str(tmp_path / "src"))
    monkeypatch.setenv("DVC_VIDEO_SINK", "mjpeg")
    monkeypatch.setenv("DVC_MJPEG_DECODE", "pillow")
    monkeypatch.setenv("DVC_DEVICE_CHAIN", "on")
    with pytest.raises(RuntimeError, match="DVC_DEVICE_CHAIN=on"):
        process_single_video_fd(path, str(tmp_path / "out"))
    monkeypatch.setenv("DVC_DEVICE_CHAIN", "auto")           # auto keeps the host source
    process_single_video_fd(path, str(tmp_path / "out"))
    assert any(k.endswith("compressed_final_video.mp4") for k in _outputs(str(tmp_path / "out")))
