"""Per-run quality report over an output folder, next to ``performance_analysis``.

``python -m dvc_amd.quality_analysis <output_folder> <source> [<source> ...]``

Each source is a video or a folder of videos. For every
``<output_folder>/<name>/`` that holds a compressed output (the pairing of
``performance_analysis.get_original_and_compressed_paths``: ``compressed.mp4``
of the OF driver, else ``compressed_final_video.mp4`` of the FD driver) the
source whose ``video_io.video_name`` is ``<name>`` is compared with it on the
GPU (:func:`quality.compare_videos` at ``quality.DRIVER_REF_SKIP``), and
``<output_folder>/performance/quality_data.csv`` receives one row per video.
``performance_data.csv`` is not touched. The reference has no such report
(its ``performance_analysis.py`` reports sizes and times only).
"""
from __future__ import annotations

import csv
import os
import sys

from . import performance_analysis as pa
from . import quality, video_io

FIELDNAMES = [
    "video",
    "frames",
    "psnr_y (dB)",
    "psnr_y_min (dB)",
    "psnr_bgr (dB)",
    "ssim_y",
    "ssim_y_min",
    "compressed_size_bytes",
    "bits_per_pixel",
]


def sources_by_name(sources) -> dict:
    """``video_io.video_name`` -> path for every source (a folder gives its files)."""
    found = {}
    for s in sources:
        paths = [os.path.join(s, f) for f in sorted(os.listdir(s))] if os.path.isdir(s) else [s]
        for p in paths:
            if not os.path.isdir(p) and not p.endswith(".json"):   # (.json: the sidecar of an .npy stream)
                found.setdefault(video_io.video_name(p), p)
    return found


def collect(output_folder, sources, meter=None):
    """One row dict per ``<output_folder>/<name>/`` with a compressed output and a source."""
    by_name = sources_by_name(sources)
    rows = []
    for item in sorted(os.listdir(output_folder)):
        sub = os.path.join(output_folder, item)
        if not os.path.isdir(sub):
            continue
        comp = pa.get_original_and_compressed_paths(sub)[1]
        if comp is None:
            continue
        if item not in by_name:
            print(f"Warning: no source named {item} for {sub}")
            continue
        _, s = quality.compare_videos(by_name[item], pa._resolve(comp), quality.DRIVER_REF_SKIP, meter)
        if s["frames"] == 0:
            print(f"Warning: no frame pairs in {sub}")
            continue
        size = pa.get_file_size(comp)
        rows.append({"video": item, "frames": s["frames"], "psnr_y (dB)": s["psnr_y"],
                     "psnr_y_min (dB)": s["psnr_y_min"], "psnr_bgr (dB)": s["psnr_bgr"], "ssim_y": s["ssim_y"],
                     "ssim_y_min": s["ssim_y_min"], "compressed_size_bytes": size,
                     "bits_per_pixel": size * 8 / (s["frames"] * s["width"] * s["height"])})
    return rows


def write_csv(rows, csv_file):
    with open(csv_file, mode="w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=FIELDNAMES)
        w.writeheader()
        w.writerows(rows)


def main(argv=None, meter=None):
    argv = sys.argv if argv is None else argv
    if len(argv) < 3:
        print("Usage: python quality_analysis.py <output_folder> <source> [<source> ...]")
        sys.exit(1)
    output_folder = argv[1]
    if not os.path.isdir(output_folder):
        print(f"Invalid output folder: {output_folder}")
        sys.exit(1)
    rows = collect(output_folder, argv[2:], meter)
    if not rows:
        print("No quality data found.")
        sys.exit(1)
    perf = os.path.join(output_folder, "performance")
    os.makedirs(perf, exist_ok=True)
    csv_file = os.path.join(perf, "quality_data.csv")
    write_csv(rows, csv_file)
    print(f"CSV saved in: {csv_file}")


if __name__ == "__main__":
    main()
