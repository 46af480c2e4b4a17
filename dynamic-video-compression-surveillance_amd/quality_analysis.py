"""Per-run quality report over an output folder, next to ``performance_analysis``.

``python -m dvc_amd.quality_analysis [--fd [name=value,...]] <output_folder> <source> [<source> ...]``

Each source is a video or a folder of videos. For every
``<output_folder>/<name>/`` that holds a compressed output (the pairing of
``performance_analysis.get_original_and_compressed_paths``: ``compressed.mp4``
of the OF driver, else ``compressed_final_video.mp4`` of the FD driver) the
source whose ``video_io.video_name`` is ``<name>`` is compared with it on the
GPU (:func:`quality.compare_videos` at ``quality.DRIVER_REF_SKIP``), and
``<output_folder>/performance/quality_data.csv`` receives one row per video.
``performance_data.csv`` is not touched. The reference has no such report
(its ``performance_analysis.py`` reports sizes and times only).

``<output_folder>/performance/quality_regions.csv`` splits those figures into the
blocks the workers kept and the blocks they flattened (DESIGN.md "Quality
metrics", :func:`quality.compare_videos_regions`). A folder with
``compressed.mp4`` and ``mask.mp4`` (the OF driver) gets a row from that mask
video, blocks of 8, partial blocks kept. A folder with
``compressed_final_video.mp4`` (the FD driver, which writes no mask) gets a row
only with ``--fd``: the masks are replayed from the source
(:func:`quality.fd_static_masks`) with the driver's defaults, or with
``--fd block_size=8,kernel_size=10,release_factor=0.3`` those values — they must
be the ones the run used, which is why nothing is guessed without the option.
"""
from __future__ import annotations

import csv
import math
import os
import re
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

REGION_FIELDNAMES = [
    "video",
    "frames",
    "static_pixel_share",
    "psnr_y_kept (dB)",
    "psnr_y_static (dB)",
    "psnr_bgr_kept (dB)",
    "psnr_bgr_static (dB)",
    "ssim_y_kept",
    "ssim_y_static",
    "ssim_y_mixed",
    "kept_windows",
    "static_windows",
    "mixed_windows",
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


def collect_regions(output_folder, sources, fd=None, meter=None, fd_masks=quality.fd_static_masks):
    """One ``quality_regions.csv`` row dict per ``<output_folder>/<name>/`` whose mask is
    known: the OF driver's ``mask.mp4``, or with ``fd`` (a dict of the FD driver's
    parameters, empty for its defaults) the masks ``fd_masks(source, **fd)`` replays."""
    by_name = sources_by_name(sources)
    rows = []
    for item in sorted(os.listdir(output_folder)):
        sub = os.path.join(output_folder, item)
        if not os.path.isdir(sub) or item not in by_name:
            continue
        of_comp, of_mask = (pa._resolve(os.path.join(sub, f)) for f in ("compressed.mp4", "mask.mp4"))
        fd_comp = pa._resolve(os.path.join(sub, "compressed_final_video.mp4"))
        if of_comp and of_mask:
            comp, masks, block, partial_static = of_comp, of_mask, 8, 0
        elif fd_comp and fd is not None:
            comp, masks, block, partial_static = fd_comp, fd_masks(by_name[item], **fd), int(fd.get("block_size", 4)), 1
        else:
            continue
        _, s = quality.compare_videos_regions(by_name[item], comp, masks, block, partial_static,
                                              quality.DRIVER_REF_SKIP, meter)
        if s["frames"] == 0:
            continue
        rows.append({"video": item, "frames": s["frames"], "static_pixel_share": s["static_pixel_share"],
                     "psnr_y_kept (dB)": s["psnr_y_kept"], "psnr_y_static (dB)": s["psnr_y_static"],
                     "psnr_bgr_kept (dB)": s["psnr_bgr_kept"], "psnr_bgr_static (dB)": s["psnr_bgr_static"],
                     "ssim_y_kept": s["ssim_y_kept"], "ssim_y_static": s["ssim_y_static"],
                     "ssim_y_mixed": s["ssim_y_mixed"], "kept_windows": s["kept_windows"],
                     "static_windows": s["static_windows"], "mixed_windows": s["mixed_windows"]})
    return rows


def write_csv(rows, csv_file, fieldnames=FIELDNAMES):
    """A class without a pixel or a window has no figure (nan): its cell stays empty."""
    with open(csv_file, mode="w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=fieldnames)
        w.writeheader()
        w.writerows({k: "" if isinstance(v, float) and math.isnan(v) else v for k, v in r.items()} for r in rows)


_FD_TYPES = {"block_size": int, "search_area": int, "motion_threshold": float, "min_area": float, "kernel_size": int,
             "release_factor": float, "quantization_level": float, "scale_factor": float}


def parse_fd(argv):
    """``argv`` without ``--fd [name=value,...]``, and the FD parameters it gave
    (None without the option, {} for the driver's defaults)."""
    if "--fd" not in argv:
        return list(argv), None
    i = argv.index("--fd")
    rest, fd = list(argv[:i]) + list(argv[i + 1:]), {}
    if i < len(rest) and re.fullmatch(r"\w+=[^,=]+(,\w+=[^,=]+)*", rest[i]) and not os.path.exists(rest[i]):
        for pair in rest.pop(i).split(","):
            name, value = pair.split("=")
            if name not in _FD_TYPES:
                print(f"--fd: unknown parameter {name} (known: {', '.join(_FD_TYPES)})")
                sys.exit(1)
            fd[name] = _FD_TYPES[name](value)
    return rest, fd


def main(argv=None, meter=None, fd_masks=quality.fd_static_masks):
    argv, fd = parse_fd(sys.argv if argv is None else argv)
    if len(argv) < 3:
        print("Usage: python quality_analysis.py [--fd [name=value,...]] <output_folder> <source> [<source> ...]")
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
    regions = collect_regions(output_folder, argv[2:], fd, meter, fd_masks)
    if regions:
        csv_file = os.path.join(perf, "quality_regions.csv")
        write_csv(regions, csv_file, REGION_FIELDNAMES)
        print(f"CSV saved in: {csv_file}")


if __name__ == "__main__":
    main()
