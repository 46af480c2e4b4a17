"""GPU: the camera stream set (DVC_FLAG_JPEGD_CAMERA) of dvc_jpegd_decode byte
for byte against Pillow on the streams of tests/mjpeg_cam_cases.py: 4:2:2 and
4:4:4 at sizes whose MCU counts are odd (segments start mid-row, MCUs straddle
the IDCT kernel's waves), narrow planes, a second workgroup along x, hundreds of
one-MCU segments, padded pitches on a caller's stream, frames without DHT
segments, header changes between all four layouts, damaged data (the same bytes
tools/jpegd_host_check.cc has run under the host sanitizers in
tests/test_mjpeg_camera.py), and a camera AVI through both drivers."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import mjpeg_cam_cases as C

pytestmark = pytest.mark.gpu


def _handle(N, W, H, max_batch=3, stream=None, flags=0):
    h = ctypes.c_void_p()
    N.check(N.lib().dvc_jpegd_create(W, H, max_batch, 0, stream, flags | N.DVC_FLAG_JPEGD_CAMERA, ctypes.byref(h)))
    return h


def _set_header(N, h, jpg):
    n, w, hh, fmt = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    N.check(N.lib().dvc_jpegd_set_header(h, jpg, len(jpg), ctypes.byref(n), ctypes.byref(w), ctypes.byref(hh),
                                         ctypes.byref(fmt)))
    return n.value, w.value, hh.value, 3 if fmt.value == N.FMT_BGR else 1


def _pack(datas, stride=None):
    stride = stride or max(len(d) for d in datas) + 3
    buf = np.full((len(datas), stride), 0xEE, np.uint8)
    for i, d in enumerate(datas):
        buf[i, :len(d)] = np.frombuffer(d, np.uint8)
    return buf, np.array([len(d) for d in datas], np.uint32)


def _decode_host(N, h, jpgs, guard=0xA5):
    """Whole samples of one header through host pointers -> (frames, status, rc)."""
    hl, W, H, ch = _set_header(N, h, jpgs[0])
    assert all(j[:hl] == jpgs[0][:hl] for j in jpgs)
    buf, sizes = _pack([j[hl:] for j in jpgs])
    out = np.full((len(jpgs), H, W * ch), guard, np.uint8)
    status = np.full(len(jpgs), 77, np.int32)
    rc = N.lib().dvc_jpegd_decode(h, buf.ctypes.data, buf.shape[1], sizes.ctypes.data, len(jpgs), out.ctypes.data,
                                  W * ch, H * W * ch, status.ctypes.data)
    return out.reshape((len(jpgs), H, W, 3) if ch == 3 else (len(jpgs), H, W)), status, rc


def _check(N, jpgs, max_batch=3):
    W, H = C.pillow(jpgs[0]).shape[1::-1]
    h = _handle(N, W, H, max_batch)
    try:
        got, status, rc = _decode_host(N, h, jpgs)
    finally:
        N.lib().dvc_jpegd_destroy(h)
    assert rc == 0 and not status.any()
    for t, j in enumerate(jpgs):
        ref = C.pillow(j)
        assert np.array_equal(got[t], ref), f"frame {t}: {np.count_nonzero(got[t] != ref)} bytes differ from Pillow, " \
            f"first at {tuple(int(a[0]) for a in np.nonzero(got[t] != ref))}"


@pytest.mark.parametrize("restart", ["none", "dri1", "dri7", "row"])
@pytest.mark.parametrize("sub", ["422", "444"])
@pytest.mark.parametrize("w,h", [(70, 37), (33, 17)])
def test_decode_matches_pillow(gpu_lib, w, h, sub, restart):
    """5 x 5 and 3 x 3 (4:2:2), 9 x 5 and 5 x 3 (4:4:4) MCUs: odd counts. A batch of 3 different frames."""
    _check(gpu_lib._native, [C.stream(w, h, sub, restart, v) for v in (0, 1, 2)])


@pytest.mark.parametrize("w,h", [(3, 5), (4, 4), (5, 9)])
def test_narrow_planes_422(gpu_lib, w, h):
    """Chroma planes 2, 2 and 3 samples wide: the replication rule and the first width past it."""
    _check(gpu_lib._native, [C.stream(w, h, "422", "none", v) for v in (0, 1)])


@pytest.mark.parametrize("sub", ["422", "444"])
def test_second_workgroup_along_x(gpu_lib, sub):
    """264 x 40: 66 lanes a row in k_jpegd_out, and 33 (4:4:4) blocks a plane row."""
    _check(gpu_lib._native, [C.stream(264, 40, sub, "row", v) for v in (0, 1)])


@pytest.mark.parametrize("sub,n", [("444", 19), ("422", 36)])
def test_two_lanes_a_wave_of_the_huffman_kernel(gpu_lib, sub, n):
    """136 x 104, one MCU a segment: 221 (4:4:4) or 117 (4:2:2) segments a frame, n frames in one
    launch -> 4199 / 4212 segments: two lanes a wave, an odd count, so the last workgroup has one."""
    jpgs = [C.stream(136, 104, sub, "dri1", v) for v in range(n)]
    segs = n * (221 if sub == "444" else 117)
    assert 2 * 2048 <= segs < 3 * 2048
    _check(gpu_lib._native, jpgs, max_batch=n)


def test_max_batch_2_given_5_frames(gpu_lib):
    _check(gpu_lib._native, [C.stream(70, 37, "422", "dri7", v) for v in range(5)], max_batch=2)


@pytest.mark.parametrize("sub", ["420", "422", "444"])
def test_frames_without_dht_segments(gpu_lib, sub):
    jpgs = [C.strip_dht(C.stream(70, 37, sub, "dri7", v)) for v in (0, 1, 2)]
    assert not C.dht_segments(jpgs[0])
    _check(gpu_lib._native, jpgs)


@pytest.mark.parametrize("pad", [5, 6])       # 3 * 70 + 5: unaligned rows, byte stores; + 6 = 216: dword stores
@pytest.mark.parametrize("sub", ["422", "444"])
def test_device_pointers_padded_pitch_caller_stream(gpu_lib, sub, pad):
    import torch
    N = gpu_lib._native
    jpgs = [C.stream(70, 37, sub, "dri7", v) for v in (0, 1, 2)]
    s = torch.cuda.Stream()
    h = _handle(N, 70, 37, 2, ctypes.c_void_p(s.cuda_stream), N.DVC_FLAG_DEVICE_PTRS)
    try:
        hl, W, H, ch = _set_header(N, h, jpgs[0])
        stride = max(len(j) - hl for j in jpgs) + 3
        stride += (stride % 4 == 0)                              # frames 1 and 2 start at odd addresses
        buf, sizes = _pack([j[hl:] for j in jpgs], stride)
        pitch = ch * W + pad
        slot = H * pitch + 8                                     # guard bytes between the frames' slots
        with torch.cuda.stream(s):
            d_in = torch.from_numpy(buf).pin_memory().to("cuda", non_blocking=True)
            d_sizes = torch.from_numpy(sizes.view(np.int32)).pin_memory().to("cuda", non_blocking=True)
            d_out = torch.full((3, slot), 0xA5, dtype=torch.uint8, device="cuda")
            d_status = torch.full((3,), 77, dtype=torch.int32, device="cuda")
            N.check(N.lib().dvc_jpegd_decode(h, d_in.data_ptr(), stride, d_sizes.data_ptr(), 3, d_out.data_ptr(), pitch,
                                             slot, d_status.data_ptr()))
            out = d_out.to("cpu", non_blocking=True)
            status = d_status.to("cpu", non_blocking=True)
        s.synchronize()
        assert N.lib().dvc_jpegd_sync(h) == N.DVC_OK
    finally:
        N.lib().dvc_jpegd_destroy(h)
    out, status = out.numpy(), status.numpy()
    assert not status.any()
    for t in range(3):
        rows = out[t, :H * pitch].reshape(H, pitch)
        assert np.array_equal(rows[:, :3 * W], C.pillow(jpgs[t]).reshape(H, 3 * W)), (sub, t)
        assert (rows[:, 3 * W:] == 0xA5).all() and (out[t, H * pitch:] == 0xA5).all()   # outside each row and slot


def test_jpeg_decoder_class_across_the_four_layouts(gpu_lib):
    N = gpu_lib._native
    samples = [C.stream(70, 37, "420", "row", 0), C.stream(70, 37, "422", "dri7", 0), C.stream(70, 37, "422", "dri7", 1),
               C.stream(70, 37, "444", "dri1", 0), C.gray_stream(70, 37), C.stream(33, 17, "444", "none", 1),
               C.stream(70, 37, "420", "row", 1)]
    dec = N.JpegDecoder(70, 37, max_batch=2, camera=True)
    try:
        frames = dec.decode(samples)
        assert len(frames) == len(samples)
        for f, s in zip(frames, samples):
            assert np.array_equal(f, C.pillow(s))
        with pytest.raises(N.DvcError) as e:
            dec.decode([C.rgb_stream()])
        assert e.value.code == N.DVC_E_UNSUPPORTED
        assert np.array_equal(dec.decode(samples[1:2])[0], C.pillow(samples[1]))      # the handle goes on working
    finally:
        dec.close()


@pytest.mark.parametrize("damage", C.DAMAGE)
@pytest.mark.parametrize("sub", ["422", "444"])
def test_damaged_frame_is_reported_and_its_neighbours_decode(gpu_lib, sub, damage):
    """(tests/test_mjpeg_camera.py::test_host_program_under_sanitizers_camera_mode has run the same
    bytes through the kernels' routines on the host.)"""
    N = gpu_lib._native
    hdr, data = C.damaged(sub, damage)
    refs = [C.pillow(C.stream(70, 37, sub, "row", v)) for v in (0, 1, 2)]
    H, W = refs[0].shape[:2]
    buf, sizes = _pack(data)
    h = _handle(N, W, H, 3)
    try:
        _set_header(N, h, hdr)
        out = np.full((3, H * 3 * W + 16), 0xA5, np.uint8)
        status = np.full(3, 77, np.int32)
        rc = N.lib().dvc_jpegd_decode(h, buf.ctypes.data, buf.shape[1], sizes.ctypes.data, 3, out.ctypes.data, 3 * W,
                                      out.shape[1], status.ctypes.data)
        assert status[1] == N.DVC_E_INVALID and rc == N.DVC_E_INVALID and status[0] == 0 and status[2] == 0
        for t in (0, 2):
            assert np.array_equal(out[t, :H * 3 * W].reshape(H, W, 3), refs[t])
        assert (out[:, H * 3 * W:] == 0xA5).all() and (out[1] == 0xA5).all()       # the slot keeps its sentinel
        assert N.lib().dvc_jpegd_sync(h) == N.DVC_OK
    finally:
        N.lib().dvc_jpegd_destroy(h)


def _outputs(root):
    """{relative path: bytes} of the video files and their metadata under root (not logs or timings)."""
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            if os.path.splitext(f)[1] in (".npy", ".json", ".mp4", ".y4m"):
                p = os.path.join(d, f)
                out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("driver", ["fd", "of"])
def test_camera_avi_through_the_drivers(gpu_lib, tmp_path, monkeypatch, driver):
    """A 96 x 64, 6-frame camera AVI (4:2:2, no DHT segments) decoded on the GPU gives the output
    files of a run on the .npy of Pillow's decode of the same samples."""
    from dvc_amd import video_io
    from dvc_amd.frame_differencing import process_single_video_fd
    from dvc_amd.motion_compression_opt import process_single_video_of
    run = {"fd": process_single_video_fd, "of": process_single_video_of}[driver]
    samples = [C.strip_dht(C.stream(96, 64, "422", "row", v, content="gradient" if v % 2 else "flat")) for v in range(6)]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    (tmp_path / "a" / "cam.avi").write_bytes(C.avi(samples, 96, 64, 25, 1))
    np.save(tmp_path / "b" / "cam.npy", np.stack([C.pillow(s) for s in samples]))
    (tmp_path / "b" / "cam.json").write_text(json.dumps({"fps": 25.0}))
    monkeypatch.setenv("DVC_MJPEG_DECODE", "gpu")
    r = video_io.open_source(str(tmp_path / "a" / "cam.avi"))
    assert isinstance(r, video_io.AviMjpegReader) and r.isOpened() and r._gpu
    assert [r.get(p) for p in (video_io.CAP_PROP_FPS, video_io.CAP_PROP_FRAME_COUNT)] == [25.0, 6.0]
    r.release()
    run(str(tmp_path / "a" / "cam.avi"), str(tmp_path / "out_a"))
    run(str(tmp_path / "b" / "cam.npy"), str(tmp_path / "out_b"))
    got, want = _outputs(tmp_path / "out_a"), _outputs(tmp_path / "out_b")
    assert want and sorted(got) == sorted(want)
    assert any(k.endswith(".npy") and len(v) > 256 + 96 * 64 for k, v in want.items())      # frames were written
    for k in want:
        assert got[k] == want[k], k
