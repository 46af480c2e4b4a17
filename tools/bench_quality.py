"""Quality-meter throughput (GPU box): dvc_quality_compare on device-resident
1080p BGR frames, the synthetic clip against its quality-75 JPEG round trip
(the project's GPU encoder and decoder), batches of 32, device pointers on a
joined stream, timed with device events around `steps` calls (5 runs after a
warm-up). Prints one JSON line: Mpx/s, the bytes read per second (6 B a pixel:
both frames once) against dvc_copy_rate on the same box in the same run, the
one-core time of the numpy reference (tests/quality_ref.py) on the same frames,
and — with --kernels, from a second run of this script under rocprofv3
--kernel-trace --stats — the time of each kernel per batch. The records of the
timed batch are checked against the reference on two frames.
  python tools/bench_quality.py [--kernels] [--out FILE] [--width W --height H --batch B --quality Q]
--regions measures dvc_quality_compare_regions instead: the same frames under a
mask of 8x8 blocks of which about 10 % are non-zero (seed 0; block 8, partial
blocks kept, the OF driver's rule), with the whole-frame meter timed in the same
run, run by run in turn, as the yardstick: Mpx/s of both, their ratio, and the
bytes read per pixel (6 + 1 + the class bits) against the same run's copy rate.
  python tools/bench_quality.py --regions [--kernels] [--out profiles/quality_regions_1080p.json]
"""
import ctypes
import time

from codec_bench import child_args, emit, kernel_times, parser, time_calls


def main():
    ap = parser(steps=2000)
    ap.add_argument("--no-copy-rate", action="store_true")
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--regions", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    from dvc_amd import _native as N
    from dvc_amd.synthetic import SyntheticClip

    W, H, B = a.width, a.height, a.batch
    L = N.lib()
    clip = SyntheticClip(W, H, seed=0)
    ref = np.stack([clip.frame(t) for t in range(B)])
    enc, dec = N.JpegEncoder(W, H, True, a.quality, max_batch=8), N.JpegDecoder(W, H, max_batch=8)
    test, jpeg_bytes = [], 0
    for f0 in range(0, B, 8):
        samples = [enc.header + p for p in enc.encode(ref[f0:f0 + 8])]
        jpeg_bytes += sum(len(s) for s in samples)
        test += dec.decode(samples)
    enc.close()
    dec.close()
    test = np.stack(test)
    d_ref, d_test = torch.from_numpy(ref).cuda(), torch.from_numpy(test).cuda()
    rec_size = np.dtype(N.QUALITY_FRAME).itemsize
    d_res = torch.zeros(B * rec_size, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    h = ctypes.c_void_p()
    N.check(L.dvc_quality_create(W, H, B, 0, ctypes.c_void_p(s.cuda_stream), N.DVC_FLAG_DEVICE_PTRS, ctypes.byref(h)))

    def call():
        N.check(L.dvc_quality_compare(h, d_ref.data_ptr(), 3 * W, 3 * W * H, d_test.data_ptr(), 3 * W, 3 * W * H, B,
                                      d_res.data_ptr()))

    if a.regions:
        return regions(a, N, L, h, s, call, ref, test, d_ref, d_test)
    ms = time_calls(s, call, a.warmup, a.runs, a.steps)
    N.check(L.dvc_quality_sync(h))
    L.dvc_quality_destroy(h)
    rec = d_res.cpu().numpy().view(N.QUALITY_FRAME)
    from dvc_amd import quality
    summary = quality.summarize(rec)
    best = float(np.median(ms))
    px = B * W * H
    res = {
        "metric": "quality meter, device-resident BGR pairs -> frame records (dvc_quality_compare)",
        "value": round(px / best / 1e3, 1), "unit": "Mpixels/s",
        "frame_pairs_per_s": round(B / best * 1e3, 1), "ms_per_batch": round(best, 4),
        "timing": {"ms_per_batch_per_run": [round(m, 4) for m in ms], "steps": a.steps, "warmup": a.warmup,
                   "value_per_run": [round(px / m / 1e3, 1) for m in ms], "timed_with": "device events, joined stream"},
        "config": {"width": W, "height": H, "batch": B, "quality": a.quality,
                   "data": "synthetic clip seed 0 against its Motion-JPEG round trip", "io": "device"},
        "read_GBps": round(6 * px / best / 1e6, 1),
        "clip": {"psnr_y_dB": round(summary["psnr_y"], 3), "psnr_bgr_dB": round(summary["psnr_bgr"], 3),
                 "ssim_y": round(summary["ssim_y"], 5), "bits_per_pixel": round(8 * jpeg_bytes / px, 3)},
    }
    if not a.no_copy_rate:
        # dvc_copy_rate counts bytes read + written; the meter only reads
        res["copy_rate_GBps"] = round(N.copy_rate(0), 1)
        res["read_frac_of_copy_rate"] = round(res["read_GBps"] / res["copy_rate_GBps"], 4)
    if not a.no_reference:
        from tests import quality_ref as R
        t0 = time.perf_counter()
        want = R.records(ref[:2], test[:2])
        res["numpy_reference_s_per_frame_pair"] = round((time.perf_counter() - t0) / 2, 4)
        res["equals_reference"] = bool(np.array_equal(rec[:2], want))
        if not res["equals_reference"]:
            raise SystemExit("the timed batch's records differ from the reference")
    if a.kernels:
        res["kernels"] = kernel_times(__file__, "k_quality_", child_args(a, "--no-copy-rate", "--no-reference"))
    emit(res, a.out)


def regions(a, N, L, h, s, whole, ref, test, d_ref, d_test):
    """--regions: dvc_quality_compare_regions and the whole-frame call `whole`, run by run in turn."""
    import numpy as np
    import torch
    W, H, B, block = a.width, a.height, a.batch, 8
    live = np.random.default_rng(0).random((B, -(-H // block), -(-W // block))) < 0.1
    masks = (np.repeat(np.repeat(live, block, axis=1), block, axis=2)[:, :H, :W] * 255).astype(np.uint8)
    d_mask = torch.from_numpy(masks).cuda()
    d_res = torch.zeros(B * np.dtype(N.QUALITY_REGIONS).itemsize, dtype=torch.uint8, device="cuda")

    def call():
        N.check(L.dvc_quality_compare_regions(h, d_ref.data_ptr(), 3 * W, 3 * W * H, d_test.data_ptr(), 3 * W, 3 * W * H,
                                              d_mask.data_ptr(), W, W * H, block, 0, B, d_res.data_ptr()))

    ms, ms_whole = [], []
    for r in range(a.runs):
        ms_whole += time_calls(s, whole, a.warmup if r == 0 else 0, 1, a.steps)
        ms += time_calls(s, call, a.warmup if r == 0 else 0, 1, a.steps)
    N.check(L.dvc_quality_sync(h))
    L.dvc_quality_destroy(h)
    rec = d_res.cpu().numpy().view(N.QUALITY_REGIONS)
    from dvc_amd import quality
    summary = quality.summarize_regions(rec)
    best, best_whole = float(np.median(ms)), float(np.median(ms_whole))
    px = B * W * H
    class_bytes = 4 * B * (-(-H // block)) * (-(-W // 32))
    read = 7 * px + class_bytes
    res = {
        "metric": "quality meter split by a mask, device-resident BGR pairs and masks -> region records "
                  "(dvc_quality_compare_regions)",
        "value": round(px / best / 1e3, 1), "unit": "Mpixels/s", "ms_per_batch": round(best, 4),
        "whole_frame_value": round(px / best_whole / 1e3, 1), "whole_frame_ms_per_batch": round(best_whole, 4),
        "ratio_to_whole_frame": round(best_whole / best, 4), "bytes_ratio_whole_to_regions": round(6 * px / read, 4),
        "timing": {"ms_per_batch_per_run": [round(m, 4) for m in ms],
                   "whole_frame_ms_per_batch_per_run": [round(m, 4) for m in ms_whole], "steps": a.steps,
                   "warmup": a.warmup, "timed_with": "device events, joined stream, the two calls run by run in turn"},
        "config": {"width": W, "height": H, "batch": B, "quality": a.quality, "block": block, "partial_static": 0,
                   "mask": "8x8 blocks, 10 % non-zero, seed 0", "io": "device",
                   "data": "synthetic clip seed 0 against its Motion-JPEG round trip"},
        "read_bytes_per_pixel": round(read / px, 4), "read_GBps": round(read / best / 1e6, 1),
        "whole_frame_read_GBps": round(6 * px / best_whole / 1e6, 1),
        "clip": {"static_pixel_share": round(summary["static_pixel_share"], 4),
                 "psnr_y_kept_dB": round(summary["psnr_y_kept"], 3), "psnr_y_static_dB": round(summary["psnr_y_static"], 3),
                 "ssim_y_kept": round(summary["ssim_y_kept"], 5), "ssim_y_static": round(summary["ssim_y_static"], 5)},
    }
    if not a.no_copy_rate:
        res["copy_rate_GBps"] = round(N.copy_rate(0), 1)
        res["read_frac_of_copy_rate"] = round(res["read_GBps"] / res["copy_rate_GBps"], 4)
        res["whole_frame_read_frac_of_copy_rate"] = round(res["whole_frame_read_GBps"] / res["copy_rate_GBps"], 4)
    if not a.no_reference:
        from tests import quality_regions_ref as RR
        want = RR.records(ref[:2], test[:2], masks[:2], block, 0)
        res["equals_reference"] = bool(np.array_equal(rec[:2], want))
        if not res["equals_reference"]:
            raise SystemExit("the timed batch's records differ from the reference")
    if a.kernels:
        res["kernels"] = kernel_times(__file__, "k_quality_", child_args(a, "--regions", "--no-copy-rate", "--no-reference"))
    emit(res, a.out)


if __name__ == "__main__":
    main()
