"""Motion-JPEG decoder throughput (GPU box): dvc_jpegd_decode on device-resident
entropy data of 1080p synthetic-clip frames (encoded by dvc_jpeg_encode at
quality 75), batches of 32, device pointers on a joined stream, timed with
device events around `steps` calls (5 runs after a warm-up). Prints one JSON
line: decode Mpx/s and frames/s (the median run, with every run's value) and —
with --kernels, from a second run of this script under rocprofv3 --kernel-trace
--stats — the time of each kernel per batch.
  python tools/bench_decode.py [--kernels] [--out FILE] [--width W --height H --batch B --quality Q]
With --subsampling 420|422|444 the frames are encoded by Pillow instead (quality
75 unless --quality says otherwise, one MCU row a restart segment) in that
sampling and decoded on a camera handle (DVC_FLAG_JPEGD_CAMERA); the line then
also carries the rate of a device-to-device copy of the 6 bytes a pixel that
k_jpegd_out moves, timed in the same run.
"""
import ctypes

from codec_bench import child_args, emit, kernel_times, parser, time_calls


def main():
    ap = parser()
    ap.add_argument("--subsampling", choices=["420", "422", "444"], default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    from dvc_amd import _native as N
    from dvc_amd.synthetic import SyntheticClip

    W, H, B = a.width, a.height, a.batch
    L = N.lib()
    clip = SyntheticClip(W, H, seed=0)
    frames = np.stack([clip.frame(t) for t in range(B)])
    flags, nseg = N.DVC_FLAG_DEVICE_PTRS, (H + 15) // 16
    if a.subsampling:
        import io
        from PIL import Image
        jpgs = []
        for f in frames:
            buf = io.BytesIO()
            Image.fromarray(f[..., ::-1].copy()).save(buf, "JPEG", quality=a.quality, restart_marker_rows=1,
                                                      subsampling={"444": 0, "422": 1, "420": 2}[a.subsampling])
            jpgs.append(buf.getvalue())
        hl = 2                                                       # marker segments, SOI through SOS
        while jpgs[0][hl + 1] != 0xDA:
            hl += 2 + int.from_bytes(jpgs[0][hl + 2:hl + 4], "big")
        hl += 2 + int.from_bytes(jpgs[0][hl + 2:hl + 4], "big")
        header = jpgs[0][:hl]
        assert all(j[:hl] == header for j in jpgs)
        payloads = [j[hl:] for j in jpgs]
        flags |= N.DVC_FLAG_JPEGD_CAMERA
        nseg = (H + (15 if a.subsampling == "420" else 7)) // (16 if a.subsampling == "420" else 8)
    else:
        enc = N.JpegEncoder(W, H, True, a.quality, B)
        payloads = enc.encode(frames)
        header = enc.header
        enc.close()
    stride = (max(len(p) for p in payloads) + 255) & ~255
    host = np.zeros((B, stride), np.uint8)
    for i, p in enumerate(payloads):
        host[i, :len(p)] = np.frombuffer(p, np.uint8)
    data = torch.from_numpy(host).cuda()
    sizes = torch.tensor([len(p) for p in payloads], dtype=torch.int32, device="cuda")
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    h = ctypes.c_void_p()
    N.check(L.dvc_jpegd_create(W, H, B, 0, ctypes.c_void_p(s.cuda_stream), flags, ctypes.byref(h)))
    N.check(L.dvc_jpegd_set_header(h, header, len(header), None, None, None, None))

    def call():
        N.check(L.dvc_jpegd_decode(h, data.data_ptr(), stride, sizes.data_ptr(), B, out.data_ptr(), 3 * W, 3 * W * H,
                                   status.data_ptr()))

    ms = time_calls(s, call, a.warmup, a.runs, a.steps)
    N.check(L.dvc_jpegd_sync(h))
    L.dvc_jpegd_destroy(h)
    assert not status.cpu().numpy().any()
    in_bytes = sum(len(p) for p in payloads)
    mid = float(np.median(ms))
    px = B * W * H
    res = {
        "metric": "Motion-JPEG decode, device-resident entropy data -> BGR (dvc_jpegd_decode)",
        "value": round(px / mid / 1e3, 1), "unit": "Mpixels/s",
        "frames_per_s": round(B / mid * 1e3, 1), "ms_per_batch": round(mid, 4),
        "timing": {"ms_per_batch_per_run": [round(m, 4) for m in ms], "steps": a.steps, "warmup": a.warmup,
                   "value_per_run": [round(px / m / 1e3, 1) for m in ms], "statistic": "median of the runs",
                   "timed_with": "device events, joined stream"},
        "config": {"width": W, "height": H, "batch": B, "quality": a.quality, "data": "synthetic clip seed 0",
                   "io": "device", "restart_segments_per_frame": nseg},
        "compressed_bytes_per_frame": round(in_bytes / B), "bits_per_pixel": round(8 * in_bytes / px, 3),
    }
    more = []
    if a.subsampling:
        res["config"].update(subsampling=a.subsampling, encoder="Pillow, restart_marker_rows=1", handle="camera")
        more = ["--subsampling", a.subsampling]
        # what k_jpegd_out moves for 4:4:4: 3 B/px of planes in, 3 B/px of BGR out = a copy of 3 B/px
        src = torch.empty_like(out)
        cms = time_calls(s, lambda: out.copy_(src, non_blocking=True), a.warmup, a.runs, a.steps)
        res["copy_6B_per_px"] = {"ms_per_batch": round(float(np.median(cms)), 4),
                                 "GB_per_s": round(6 * px / float(np.median(cms)) / 1e6, 1)}
    if a.kernels:
        res["kernels"] = kernel_times(__file__, "k_jpegd_", child_args(a, *more))
    emit(res, a.out)


if __name__ == "__main__":
    main()
