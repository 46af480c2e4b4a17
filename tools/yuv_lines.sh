#!/bin/bash
# GPU box: the YUV bench lines kept under profiles/ (in-place surfaces).
set -e
cd "$(dirname "$0")/.."
O=${DVC_OUT:-bench_out}/yuv_lines   # where the lines go
mkdir -p $O
timeout -k 10 300 python3 -u bench.py --full --in-format NV12 > $O/nv12.json
timeout -k 10 300 python3 -u bench.py --full --in-format I420 > $O/i420.json
timeout -k 10 300 python3 -u bench.py --full --in-format NV12 --out-format I420 > $O/nv12_i420.json
timeout -k 10 300 python3 -u bench.py --full --io host-pinned --in-format NV12 --out-format I420 --steps 20 --warmup 2 \
    > $O/pinned_nv12_i420.json
timeout -k 10 300 python3 -u bench.py --full --io host-pinned --steps 20 --warmup 2 > $O/pinned_bgr.json
