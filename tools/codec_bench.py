"""What bench_encode.py, bench_decode.py and bench_quality.py share: the common
command line, the profiled child run behind --kernels, the warm-up / runs /
device-event timing loop, and the print-and-write tail. A module, not a script."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


def parser(steps=20):
    """The arguments every codec benchmark takes (a tool adds its own to the result)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--steps", type=int, default=steps)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default="")
    return ap


def kernel_times(script, prefix, args):
    """{kernel: microseconds per launch} of the ``prefix`` kernels from a child run
    of ``script`` with ``args`` under rocprofv3 --kernel-trace --stats."""
    d = tempfile.mkdtemp(prefix="dvc_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(script), *args]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=300)
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if prefix in row["Name"]:
                    name = prefix + row["Name"].split(prefix)[1].split("(")[0].split("<")[0]
                    out[name] = {"us_per_launch": round(float(row["AverageNs"]) / 1e3, 1),
                                 "launches": int(row["Calls"])}
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def child_args(a, *more):
    """The command line of the profiled child run: 3 steps, one run, the parent's geometry."""
    return ["--steps", "3", "--runs", "1", *more, "--width", str(a.width), "--height", str(a.height),
            "--batch", str(a.batch), "--quality", str(a.quality)]


def time_calls(stream, call, warmup, runs, steps):
    """Milliseconds per call of each of ``runs`` runs of ``steps`` calls, timed with
    device events on ``stream`` (a torch stream the handle has joined) after ``warmup`` calls."""
    import torch
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            call()
        stream.synchronize()
        ms = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(steps):
                call()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / steps)
    return ms


def emit(res, out):
    """Print the result as one JSON line; ``out``: also write it to that file."""
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
