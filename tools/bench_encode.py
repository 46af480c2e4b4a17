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
--target-bytes N: a rate handle (dvc_jpeg_create_rate) with N bytes a frame and
--quality-range lo:hi (default 10:95) instead of --quality; N = 0 takes the
size of the same frames at --quality with the fixed tables, header included, so
that the search ends inside the range. The line then carries the handle's
counters and the bytes written against the target, stuffing included.
  python tools/bench_encode.py [--kernels] [--out FILE] [--width W --height H --batch B --quality Q]
                               [--huffman fixed|optimized] [--frames clip|fd]
                               [--target-bytes N [--quality-range lo:hi]]
"""
import ctypes

from codec_bench import child_args, emit, kernel_times, parser, time_calls


def main():
    ap = parser()
    ap.add_argument("--no-copy-rate", action="store_true")
    ap.add_argument("--huffman", choices=("fixed", "optimized"), default="fixed")
    ap.add_argument("--frames", choices=("clip", "fd"), default="clip")
    ap.add_argument("--target-bytes", type=int, default=None)
    ap.add_argument("--quality-range", default="10:95")
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
    rate = a.target_bytes is not None
    stride = (bound.value + (N.JPEG_RATE_PREFIX_MAX if rate else N.JPEG_OPT_PREFIX_MAX if opt else 0) + 255) & ~255
    out = torch.empty((B, stride), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    h = ctypes.c_void_p()
    hn = ctypes.c_size_t()
    flags = N.DVC_FLAG_DEVICE_PTRS | (N.DVC_FLAG_JPEG_OPT_HUFFMAN if opt else 0)

    def call():
        N.check(L.dvc_jpeg_encode(h, frames.data_ptr(), 3 * W, 3 * W * H, B, out.data_ptr(), stride, sizes.data_ptr()))

    target, q_lo, q_hi = a.target_bytes, *(int(v) for v in a.quality_range.split(":"))
    if rate and not target:   # the same frames at --quality, fixed tables: header + data
        N.check(L.dvc_jpeg_create(W, H, N.FMT_BGR, a.quality, B, 0, ctypes.c_void_p(s.cuda_stream), N.DVC_FLAG_DEVICE_PTRS,
                                  ctypes.byref(h)))
        N.check(L.dvc_jpeg_header(h, None, 0, ctypes.byref(hn)))
        call()
        N.check(L.dvc_jpeg_sync(h))
        L.dvc_jpeg_destroy(h)
        target = int(sizes.cpu().numpy().astype(np.int64).sum()) // B + hn.value
    if rate:
        N.check(L.dvc_jpeg_create_rate(W, H, N.FMT_BGR, target, q_lo, q_hi, B, 0, ctypes.c_void_p(s.cuda_stream), flags,
                                       ctypes.byref(h)))
    else:
        N.check(L.dvc_jpeg_create(W, H, N.FMT_BGR, a.quality, B, 0, ctypes.c_void_p(s.cuda_stream), flags, ctypes.byref(h)))
    N.check(L.dvc_jpeg_header(h, None, 0, ctypes.byref(hn)))

    ms = time_calls(s, call, a.warmup, a.runs, a.steps)
    N.check(L.dvc_jpeg_sync(h))
    stats = None
    if rate:
        buf = (ctypes.c_uint64 * len(N.JPEG_RATE_STATS))()
        N.check(L.dvc_jpeg_rate_stats(h, buf))
        stats = dict(zip(N.JPEG_RATE_STATS, (int(v) for v in buf)))
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
    if rate:
        res["metric"] = "Motion-JPEG encode at a rate target, device-resident BGR -> entropy data (dvc_jpeg_encode)"
        res["config"].update(quality=None, target_bytes=target, quality_range=[q_lo, q_hi])
        res["rate"] = dict(stats, rounds=1 + (q_hi - q_lo).bit_length(),
                           mean_quality=round(stats["quality_frames"] / max(stats["frames"], 1), 2),
                           est_bytes_per_frame=round(stats["est_bytes"] / max(stats["frames"], 1)),
                           written_bytes_per_frame=res["total_bytes_per_frame"],
                           written_over_target=round(res["total_bytes_per_frame"] / target, 4))
    if not a.no_copy_rate:
        res["copy_rate_GBps"] = round(N.copy_rate(0), 1)
        res["pipeline_frac_of_copy_rate"] = round(res["pipeline_GBps"] / res["copy_rate_GBps"], 4)
    if a.kernels:
        res["kernels"] = kernel_times(__file__, "k_jpeg_", child_args(a, "--no-copy-rate", "--huffman", a.huffman, "--frames", a.frames,
                                                                    *(["--target-bytes", str(target), "--quality-range",
                                                                       a.quality_range] if rate else [])))
    emit(res, a.out)


if __name__ == "__main__":
    main()
