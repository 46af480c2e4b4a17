"""Motion-JPEG encoder throughput (GPU box): dvc_jpeg_encode on device-resident
1080p BGR frames of the synthetic clip, batches of 32, device pointers on a
joined stream, timed with device events around `steps` calls (5 runs after a
warm-up). Prints one JSON line: encode Mpx/s and frames/s, the bytes moved per
second against dvc_copy_rate on the same box, and — with --kernels, from a
second run of this script under rocprofv3 --kernel-trace --stats — the time of
each kernel per batch. --huffman optimized: a handle with
DVC_FLAG_JPEG_OPT_HUFFMAN (tables built on the GPU for every batch); --frames fd:
the FD worker's compressed frames of the same clip instead of the clip's own.
The line carries the total bytes per frame, header included, for both modes.
  python tools/bench_encode.py [--kernels] [--out FILE] [--width W --height H --batch B --quality Q]
                               [--huffman fixed|optimized] [--frames clip|fd]
"""
import ctypes

from codec_bench import child_args, emit, kernel_times, parser, time_calls


def main():
    ap = parser()
    ap.add_argument("--no-copy-rate", action="store_true")
    ap.add_argument("--huffman", choices=("fixed", "optimized"), default="fixed")
    ap.add_argument("--frames", choices=("clip", "fd"), default="clip")
    a = ap.parse_args()

    import numpy as np
    import torch
    from dvc_amd import _native as N
    from dvc_amd.synthetic import SyntheticClip

    W, H, B = a.width, a.height, a.batch
    L = N.lib()
    clip = SyntheticClip(W, H, seed=0)
    if a.frames == "fd":   # what the FD driver hands to its compressed video: static blocks flattened
        import dvc_amd
        fd = dvc_amd.FDWorker(W, H, device=0)
        fd.prime(clip.frame(0))
        host = np.stack([fd.step(clip.frame(t + 1))[1].copy() for t in range(B)])
        fd.close()
    else:
        host = np.stack([clip.frame(t) for t in range(B)])
    frames = torch.from_numpy(host).cuda()
    opt = a.huffman == "optimized"
    bound = ctypes.c_size_t()
    N.check(L.dvc_jpeg_bound(W, H, N.FMT_BGR, ctypes.byref(bound)))
    stride = (bound.value + (N.JPEG_OPT_PREFIX_MAX if opt else 0) + 255) & ~255
    out = torch.empty((B, stride), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    h = ctypes.c_void_p()
    N.check(L.dvc_jpeg_create(W, H, N.FMT_BGR, a.quality, B, 0, ctypes.c_void_p(s.cuda_stream),
                              N.DVC_FLAG_DEVICE_PTRS | (N.DVC_FLAG_JPEG_OPT_HUFFMAN if opt else 0), ctypes.byref(h)))
    hn = ctypes.c_size_t()
    N.check(L.dvc_jpeg_header(h, None, 0, ctypes.byref(hn)))

    def call():
        N.check(L.dvc_jpeg_encode(h, frames.data_ptr(), 3 * W, 3 * W * H, B, out.data_ptr(), stride, sizes.data_ptr()))

    ms = time_calls(s, call, a.warmup, a.runs, a.steps)
    N.check(L.dvc_jpeg_sync(h))
    L.dvc_jpeg_destroy(h)
    out_bytes = int(sizes.cpu().numpy().astype(np.int64).sum())
    best = float(np.median(ms))
    px = B * W * H
    # bytes the four kernels move per batch: BGR in; levels (int16, 1.5 samples per pixel) written once and
    # read twice; block offsets written twice, read twice; the stream written to scratch, read, written out
    nblk = px * 1.5 / 64
    pipeline = 3 * px + 3 * 3 * px + 4 * 4 * nblk + 3 * out_bytes
    res = {
        "metric": "Motion-JPEG encode, device-resident BGR -> entropy data (dvc_jpeg_encode)",
        "value": round(px / best / 1e3, 1), "unit": "Mpixels/s",
        "frames_per_s": round(B / best * 1e3, 1), "ms_per_batch": round(best, 4),
        "timing": {"ms_per_batch_per_run": [round(m, 4) for m in ms], "steps": a.steps, "warmup": a.warmup,
                   "value_per_run": [round(px / m / 1e3, 1) for m in ms], "timed_with": "device events, joined stream"},
        "config": {"width": W, "height": H, "batch": B, "quality": a.quality, "io": "device", "huffman": a.huffman,
                   "data": "synthetic clip seed 0" + (", the FD worker's compressed frames" if a.frames == "fd" else "")},
        "compressed_bytes_per_frame": round(out_bytes / B), "bits_per_pixel": round(8 * out_bytes / px, 3),
        # what a file holds of a frame: the handle's header in front of the encoder's bytes
        "header_bytes": int(hn.value), "total_bytes_per_frame": round(out_bytes / B + hn.value),
        "algorithmic_GBps": round((3 * px + out_bytes) / best / 1e6, 1),
        "pipeline_GBps": round(pipeline / best / 1e6, 1),
    }
    if not a.no_copy_rate:
        res["copy_rate_GBps"] = round(N.copy_rate(0), 1)
        res["pipeline_frac_of_copy_rate"] = round(res["pipeline_GBps"] / res["copy_rate_GBps"], 4)
    if a.kernels:
        res["kernels"] = kernel_times(__file__, "k_jpeg_", child_args(a, "--no-copy-rate", "--huffman", a.huffman, "--frames", a.frames))
    emit(res, a.out)


if __name__ == "__main__":
    main()
