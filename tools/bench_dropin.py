"""Drop-in driver throughput (GPU box): process_single_video_fd (or _of) end to
end as a user calls it — a 1080p Y4M (4:2:0) camera file in, the two output videos out
(.npy streams of BGR frames, Y4M with DVC_VIDEO_SINK=y4m, or Motion-JPEG .mp4 with
DVC_VIDEO_SINK=mjpeg), file I/O and host copies included. Prints one JSON line per run
(DVC_MJPEG_DECODE=gpu|pillow, recorded in the line, chooses how the OF driver's second
pass reads the first pass's .mp4 files back).
--source mjpeg reads the same synthetic clip as a Motion-JPEG .mp4 written by Mp4MjpegWriter;
--chain auto|on|off sets DVC_DEVICE_CHAIN for the run (none: leaves it unset). Both are recorded in the
line, with --label as "build" and the bytes the chain copied a frame ("chain_copies", from processing.log).
The run that finds no clip in --dir builds it first, in this process: its timed call starts with the
library loaded and the runtime initialised, which the other runs pay for inside their time.
  python tools/bench_dropin.py [--frames N] [--source y4m|mjpeg] [--sink npy|y4m|mjpeg] [--chain auto|on|off|none]
                               [--label NAME] [--module NAME] [--dir /tmp/x]
"""
import argparse
import importlib
import json
import os
import re
import shutil
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


def make_clip(path, W, H, n):
    from dvc_amd._native import bgr_to_i420
    from dvc_amd.synthetic import SyntheticClip
    c = SyntheticClip(W, H, seed=0)
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (W, H))
        for t in range(n):
            f.write(b"FRAME\n" + bgr_to_i420(c.frame(t), 0).tobytes())


def make_mjpeg_clip(path, W, H, n):
    from dvc_amd.synthetic import SyntheticClip
    from dvc_amd.video_io import Mp4MjpegWriter
    c = SyntheticClip(W, H, seed=0)
    w = Mp4MjpegWriter(path, 30, (W, H))
    for t in range(n):
        w.write(c.frame(t))
    w.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sink", choices=("npy", "y4m", "mjpeg"), default="npy")
    ap.add_argument("--path", choices=("fd", "of"), default="fd")
    ap.add_argument("--module", default="")
    ap.add_argument("--dir", default="/tmp/dvc_dropin")
    ap.add_argument("--source", choices=("y4m", "mjpeg"), default="y4m",
                    help="mjpeg: the synthetic clip as a Motion-JPEG .mp4 written by Mp4MjpegWriter")
    ap.add_argument("--chain", choices=("auto", "on", "off", "none"), default="auto",
                    help="DVC_DEVICE_CHAIN for the run; none: leave it unset (a build without the switch)")
    ap.add_argument("--label", default="", help="recorded in the line as \"build\" (an A/B of two trees)")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    src = os.path.join(a.dir, "cam.y4m" if a.source == "y4m" else "cam.mp4")
    if not os.path.exists(src):
        (make_clip if a.source == "y4m" else make_mjpeg_clip)(src, a.width, a.height, a.frames)
    os.environ["DVC_VIDEO_SINK"] = a.sink
    if a.chain != "none":
        os.environ["DVC_DEVICE_CHAIN"] = a.chain
    module = a.module or ("frame_differencing" if a.path == "fd" else "motion_compression_opt")
    mod = importlib.import_module(f"dvc_amd.{module}")
    out = os.path.join(a.dir, "out")
    shutil.rmtree(out, ignore_errors=True)
    t0 = time.time()
    if a.path == "fd":
        mod.process_single_video_fd(src, out)
    else:
        mod.process_single_video_of(src, out)
    dt = time.time() - t0
    n = a.frames - 1
    # the drivers' "device chain: source=.. sink=.. h2d=.. d2h=.." lines (one a loop): the bytes the chain copied
    chain_lines = []
    for d, _, files in os.walk(out):
        if "processing.log" in files:
            chain_lines += re.findall(r"device chain: source=(\w+) sink=(\w+) h2d=(\d+) d2h=(\d+)",
                                      open(os.path.join(d, "processing.log")).read())
    copied = [{"source": s, "sink": k, "h2d_bytes_per_frame": round(int(u) / n), "d2h_bytes_per_frame": round(int(v) / n)}
              for s, k, u, v in chain_lines]
    print(json.dumps({**({"build": a.label} if a.label else {}), "mode": f"drop-in process_single_video_{a.path}", "module": module,
                      "source": "y4m I420 file" if a.source == "y4m" else "mjpeg .mp4 file", "chain": a.chain,
                      "sink": a.sink, "mjpeg_decode": os.environ.get("DVC_MJPEG_DECODE", "auto"), "frames": n, "seconds": round(dt, 3), "fps": round(n / dt, 1),
                      "Mpx_per_s": round(n * a.width * a.height / dt / 1e6, 1), "chain_copies": copied}))
    shutil.rmtree(out, ignore_errors=True)


if __name__ == "__main__":
    main()
