"""GPU: dvc_jpegd_decode byte for byte against tests/mjpeg_dec_ref.py (which
tests/test_mjpeg_decode.py holds equal to Pillow) on the streams of
tests/mjpeg_dec_cases.py; header changes on one handle, device pointers on a
caller's stream, damaged data (the same bytes tools/jpegd_host_check.cc has run
under the host sanitizers in the CPU suite), and Mp4MjpegReader and the OF
driver with DVC_MJPEG_DECODE=gpu against pillow."""
import ctypes

import numpy as np
import pytest

from tests import mjpeg_dec_cases as D

pytestmark = pytest.mark.gpu


def _handle(N, W, H, max_batch=2, stream=None, flags=0):
    h = ctypes.c_void_p()
    N.check(N.lib().dvc_jpegd_create(W, H, max_batch, 0, stream, flags, ctypes.byref(h)))
    return h


def _set_header(N, h, jpg):
    n, w, hh, fmt = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    N.check(N.lib().dvc_jpegd_set_header(h, jpg, len(jpg), ctypes.byref(n), ctypes.byref(w), ctypes.byref(hh),
                                         ctypes.byref(fmt)))
    return n.value, w.value, hh.value, 3 if fmt.value == N.FMT_BGR else 1


def _pack(datas, stride=None):
    """Entropy data of n frames -> (host array (n, stride), sizes)."""
    stride = stride or max(len(d) for d in datas) + 3
    buf = np.full((len(datas), stride), 0xEE, np.uint8)
    for i, d in enumerate(datas):
        buf[i, :len(d)] = np.frombuffer(d, np.uint8)
    return buf, np.array([len(d) for d in datas], np.uint32)


def _decode_host(N, h, jpgs, guard=0xA5):
    """Whole samples of one header through host pointers -> (frames (n, H, W[, 3]), status, rc)."""
    hl, W, H, ch = _set_header(N, h, jpgs[0])
    buf, sizes = _pack([j[hl:] for j in jpgs])
    out = np.full((len(jpgs), H, W * ch), guard, np.uint8)
    status = np.full(len(jpgs), 77, np.int32)
    rc = N.lib().dvc_jpegd_decode(h, buf.ctypes.data, buf.shape[1], sizes.ctypes.data, len(jpgs), out.ctypes.data,
                                  W * ch, H * W * ch, status.ctypes.data)
    return out.reshape((len(jpgs), H, W, 3) if ch == 3 else (len(jpgs), H, W)), status, rc


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind,name,gray", D.ids())
def test_decode_matches_reference_and_pillow(gpu_lib, kind, name, gray, n):
    N = gpu_lib._native
    variants = [0, 1, 2][:n]                                     # three different frames; max_batch 2: a call of 3 splits
    jpgs = [D.stream(kind, name, gray, v) for v in variants]
    headers = [j[:D.header_len(j)] for j in jpgs]
    # one call for the batch; optimised Huffman tables differ from frame to frame: a call per header then
    runs = [jpgs] if len(set(headers)) == 1 else [[j] for j in jpgs]
    assert len(runs) == 1 or "opt" in name
    want = D.expected(kind, name, gray)
    h = _handle(N, want.shape[1], want.shape[0])
    try:
        got = []
        for run in runs:
            frames, status, rc = _decode_host(N, h, run)
            assert rc == 0 and not status.any()
            got += list(frames)
    finally:
        N.lib().dvc_jpegd_destroy(h)
    for t, v in enumerate(variants):
        ref = D.expected(kind, name, gray, v)
        assert np.array_equal(got[t], ref), f"{name} frame {t}: {np.count_nonzero(got[t] != ref)} bytes differ from " \
            f"the reference, first at {tuple(int(a[0]) for a in np.nonzero(got[t] != ref))}"
        assert np.array_equal(got[t], D.pillow(jpgs[t])), f"{name} frame {t} differs from Pillow"


def test_one_handle_across_header_changes(gpu_lib):
    N = gpu_lib._native
    h = _handle(N, 70, 37, 3)
    try:
        for kind, name, gray, variants in [("pil", "pil70x37_q90", None, (0, 1)), ("pil", "pil33x17_opt", None, (0,)),
                                           ("pil", "pil33x17_opt", None, (1,)),      # its own Huffman tables again
                                           ("ref", "noise70x37_q90", True, (0, 1)), ("pil", "pil70x37_q90", None, (1, 0))]:
            jpgs = [D.stream(kind, name, gray, v) for v in variants]
            got, status, rc = _decode_host(N, h, jpgs)
            assert rc == 0 and not status.any()
            for t, v in enumerate(variants):
                assert np.array_equal(got[t], D.expected(kind, name, gray, v)), name
    finally:
        N.lib().dvc_jpegd_destroy(h)


def test_jpeg_decoder_class_splits_at_header_changes(gpu_lib):
    N = gpu_lib._native
    cases = [("pil", "pil70x37_q90", None, 0), ("pil", "pil70x37_q90", None, 1), ("pil", "pil33x17_opt", None, 0),
             ("ref", "noise70x37_q90", True, 0), ("ref", "noise70x37_q90", True, 1)]
    dec = N.JpegDecoder(70, 37, max_batch=2)
    try:
        frames = dec.decode([D.stream(*c) for c in cases] + [b"\xff\xd8\xff"])
        assert len(frames) == 6 and frames[5] is None
        for f, c in zip(frames, cases):
            assert np.array_equal(f, D.expected(*c)), c
        with pytest.raises(N.DvcError) as e:                     # 4:4:4: outside the decoder's set
            import io
            from PIL import Image
            buf = io.BytesIO()
            Image.fromarray(np.zeros((37, 70, 3), np.uint8)).save(buf, "JPEG", subsampling=0)
            dec.decode([buf.getvalue()])
        assert e.value.code == N.DVC_E_UNSUPPORTED
    finally:
        dec.close()


@pytest.mark.parametrize("pad", [5, 6])       # 3 * 70 + 5: unaligned rows, byte stores; + 6 = 216: dword stores
@pytest.mark.parametrize("kind,name,gray", [("pil", "pil70x37_blocks7", None), ("ref", "noise70x37_q90", True)])
def test_device_pointers_padded_pitch_caller_stream(gpu_lib, kind, name, gray, pad):
    import torch
    N = gpu_lib._native
    jpgs = [D.stream(kind, name, gray, v) for v in (0, 1, 2)]
    s = torch.cuda.Stream()
    h = _handle(N, 70, 37, 2, ctypes.c_void_p(s.cuda_stream), N.DVC_FLAG_DEVICE_PTRS)
    try:
        hl, W, H, ch = _set_header(N, h, jpgs[0])
        stride = max(len(j) - hl for j in jpgs) + 3
        stride += (stride % 4 == 0)                              # frames 1 and 2 start at odd addresses
        assert stride % 4
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
            out = d_out.to("cpu", non_blocking=True)             # copied out on the caller's stream, no other sync
            status = d_status.to("cpu", non_blocking=True)
        s.synchronize()
        assert N.lib().dvc_jpegd_sync(h) == N.DVC_OK
    finally:
        N.lib().dvc_jpegd_destroy(h)
    out, status = out.numpy(), status.numpy()
    assert not status.any()
    for t in range(3):
        rows = out[t, :H * pitch].reshape(H, pitch)
        ref = D.expected(kind, name, gray, t).reshape(H, ch * W)
        assert np.array_equal(rows[:, :ch * W], ref), (name, t)
        assert (rows[:, ch * W:] == 0xA5).all() and (out[t, H * pitch:] == 0xA5).all()   # outside each row and slot


@pytest.mark.parametrize("damage", list(D.DAMAGE))
def test_damaged_frame_is_reported_and_its_neighbours_decode(gpu_lib, damage):
    """(tests/test_mjpeg_decode.py::test_host_program_under_sanitizers has run the
    same bytes through the kernels' routines on the host.)"""
    import torch
    N = gpu_lib._native
    hdr, data = D.damaged(damage)
    refs = [D.expected("ref", D.DAMAGE_CASE, False, v) for v in (0, 1, 0)]
    H, W = refs[0].shape[:2]
    buf, sizes = _pack(data)
    # host pointers: the call returns the middle frame's status
    h = _handle(N, W, H, 3)
    try:
        _set_header(N, h, hdr)
        out = np.full((3, H * 3 * W + 16), 0xA5, np.uint8)
        status = np.full(3, 77, np.int32)
        rc = N.lib().dvc_jpegd_decode(h, buf.ctypes.data, buf.shape[1], sizes.ctypes.data, 3, out.ctypes.data, 3 * W,
                                      out.shape[1], status.ctypes.data)
        assert status[1] < 0 and rc == status[1] and status[0] == 0 and status[2] == 0
        for t in (0, 2):
            assert np.array_equal(out[t, :H * 3 * W].reshape(H, W, 3), refs[t])
        assert (out[:, H * 3 * W:] == 0xA5).all() and (out[1] == 0xA5).all()
        assert N.lib().dvc_jpegd_sync(h) == N.DVC_OK
        # the handle goes on working
        good = [D.stream("ref", D.DAMAGE_CASE, False, 1)]
        got, st, rc = _decode_host(N, h, good)
        assert rc == 0 and np.array_equal(got[0], refs[1])
    finally:
        N.lib().dvc_jpegd_destroy(h)
    # device pointers: asynchronous, the next dvc_jpegd_sync reports it, once
    h = _handle(N, W, H, 3, None, N.DVC_FLAG_DEVICE_PTRS)
    try:
        _set_header(N, h, hdr)
        d_in, d_sizes = torch.from_numpy(buf).cuda(), torch.from_numpy(sizes.view(np.int32)).cuda()
        d_out = torch.full((3, H * 3 * W + 16), 0xA5, dtype=torch.uint8, device="cuda")
        d_status = torch.full((3,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        N.check(N.lib().dvc_jpegd_decode(h, d_in.data_ptr(), buf.shape[1], d_sizes.data_ptr(), 3, d_out.data_ptr(), 3 * W,
                                         d_out.shape[1], d_status.data_ptr()))
        rc = N.lib().dvc_jpegd_sync(h)
        status, o = d_status.cpu().numpy(), d_out.cpu().numpy()
        assert status[1] < 0 and rc == status[1] and status[0] == 0 and status[2] == 0
        assert N.lib().dvc_jpegd_sync(h) == N.DVC_OK
        for t in (0, 2):
            assert np.array_equal(o[t, :H * 3 * W].reshape(H, W, 3), refs[t])
        assert (o[:, H * 3 * W:] == 0xA5).all() and (o[1] == 0xA5).all()
    finally:
        N.lib().dvc_jpegd_destroy(h)


def _read_all(path, monkeypatch, mode):
    from dvc_amd import video_io
    monkeypatch.setenv("DVC_MJPEG_DECODE", mode)
    r = video_io.Mp4MjpegReader(path)
    assert r.isOpened() and r._gpu == (mode == "gpu")
    props = [r.get(p) for p in (video_io.CAP_PROP_FPS, video_io.CAP_PROP_FRAME_WIDTH, video_io.CAP_PROP_FRAME_HEIGHT,
                                video_io.CAP_PROP_FRAME_COUNT)]
    frames = []
    while True:
        ok, f = r.read()
        if not ok:
            assert f is None
            break
        frames.append(f)
    assert r.read() == (False, None)
    r.release()
    return frames, props


@pytest.mark.parametrize("is_color", [True, False])
def test_reader_gpu_equals_pillow(gpu_lib, tmp_path, monkeypatch, is_color):
    from dvc_amd import video_io
    from dvc_amd.synthetic import SyntheticClip
    clip = SyntheticClip(130, 50, seed=9)
    path = str(tmp_path / "clip.mp4")
    w = video_io.Mp4MjpegWriter(path, 25, (130, 50), is_color)
    for t in range(11):                                          # batches of 8: the last one is partial
        f = clip.frame(t)
        w.write(f if is_color else np.ascontiguousarray(f[..., 1]))
    w.release()
    gpu, gp = _read_all(path, monkeypatch, "gpu")
    pil, pp = _read_all(path, monkeypatch, "pillow")
    assert gp == pp == [25.0, 130.0, 50.0, 11.0]
    assert len(gpu) == len(pil) == 11
    for a, b in zip(gpu, pil):
        assert a.shape == b.shape == ((50, 130, 3) if is_color else (50, 130)) and np.array_equal(a, b)


def test_reader_ends_at_a_damaged_sample(gpu_lib, tmp_path, monkeypatch):
    from dvc_amd import video_io
    hdr, data = D.damaged("no_rst")
    path = str(tmp_path / "damaged.mp4")
    mux = video_io.Mp4Muxer(path, 25, (70, 37))
    for d in data:
        mux.add_sample(hdr + d)
    mux.close()
    frames, props = _read_all(path, monkeypatch, "gpu")
    assert props[3] == 3.0 and len(frames) == 1
    assert np.array_equal(frames[0], D.expected("ref", D.DAMAGE_CASE, False, 0))


def test_of_driver_same_output_with_either_decoder(gpu_lib, tmp_path, monkeypatch):
    from dvc_amd import video_io
    from dvc_amd.motion_compression_opt import process_single_video_of

    def _samples(path):
        r = video_io.Mp4MjpegReader(path)
        assert r.isOpened(), path
        out = []
        while True:
            ok, data = r.read_sample()
            if not ok:
                r.release()
                return out
            out.append(data)

    monkeypatch.setenv("DVC_VIDEO_SINK", "mjpeg")
    src = "synthetic://160x96?frames=12"
    got = {}
    for mode in ("gpu", "pillow"):
        monkeypatch.setenv("DVC_MJPEG_DECODE", mode)
        out = tmp_path / mode
        process_single_video_of(src, str(out))
        got[mode] = _samples(str(out / "160x96" / "compressed.mp4"))
    assert len(got["gpu"]) == 11 and got["gpu"] == got["pillow"]
