"""Motion-JPEG decoder throughput (GPU box): dvc_jpegd_decode on device-resident
entropy data of 1080p synthetic-clip frames (encoded by dvc_jpeg_encode at
quality 75), batches of 32, device pointers on a joined stream, timed with
device events around `steps` calls (5 runs after a warm-up). Prints one JSON
line: decode Mpx/s and frames/s (the median run, with every run's value) and —
with --kernels, from a second run of this script under rocprofv3 --kernel-trace
--stats — the time of each kernel per batch.
  python tools/bench_decode.py [--kernels] [--out FILE] [--width W --height H --batch B --quality Q]
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


def kernel_times(a):
    """{kernel: microseconds per launch} from a profiled child run (3 steps)."""
    d = tempfile.mkdtemp(prefix="dvc_jpegd_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--steps", "3", "--runs", "1",
               "--width", str(a.width), "--height", str(a.height), "--batch", str(a.batch), "--quality", str(a.quality)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=300)
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "k_jpegd_" in row["Name"]:
                    name = "k_jpegd_" + row["Name"].split("k_jpegd_")[1].split("(")[0].split("<")[0]
                    out[name] = {"us_per_launch": round(float(row["AverageNs"]) / 1e3, 1), "launches": int(row["Calls"])}
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default="")
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

    with torch.cuda.stream(s):
        for _ in range(a.warmup):
            call()
        s.synchronize()
        ms = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.steps):
                call()
            e1.record(s)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.steps)
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
        res["kernels"] = kernel_times(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
