"""Motion-JPEG decoder throughput (GPU box): dvc_jpegd_decode on device-resident
entropy data of 1080p synthetic-clip frames (encoded by dvc_jpeg_encode at
quality 75), batches of 32, device pointers on a joined stream, timed with
device events around `steps` calls (5 runs after a warm-up). Prints one JSON
line: decode Mpx/s and frames/s (the median run, with every run's value) and —
with --kernels, from a second run of this script under rocprofv3 --kernel-trace
--stats — the time of each kernel per batch.
  python tools/bench_decode.py [--kernels] [--out FILE] [--width W --height H --batch B --quality Q]
"""
import ctypes

from codec_bench import child_args, emit, kernel_times, parser, time_calls


def main():
    ap = parser()
    a = ap.parse_args()

    import numpy as np
    import torch
    from dvc_amd import _native as N
    from dvc_amd.synthetic import SyntheticClip

    W, H, B = a.width, a.height, a.batch
    L = N.lib()
    clip = SyntheticClip(W, H, seed=0)
    frames = np.stack([clip.frame(t) for t in range(B)])
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
    N.check(L.dvc_jpegd_create(W, H, B, 0, ctypes.c_void_p(s.cuda_stream), N.DVC_FLAG_DEVICE_PTRS, ctypes.byref(h)))
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
                   "io": "device", "restart_segments_per_frame": (H + 15) // 16},
        "compressed_bytes_per_frame": round(in_bytes / B), "bits_per_pixel": round(8 * in_bytes / px, 3),
    }
    if a.kernels:
        res["kernels"] = kernel_times(__file__, "k_jpegd_", child_args(a))
    emit(res, a.out)


if __name__ == "__main__":
    main()
