#!/bin/bash
# GPU box: the noisy (CCL-stress) FD line and the default lines with the
# measured copy rate beside the roofline.
set -e
cd "$(dirname "$0")/.."
O=${DVC_OUT:-bench_out}/nc   # where the lines go
mkdir -p $O
timeout -k 10 300 python3 -u bench.py --full > $O/fd.json
timeout -k 10 300 python3 -u bench.py --full --noisy > $O/fd_noisy.json
timeout -k 10 300 python3 -u bench.py --full --width 3840 --height 2160 > $O/fd_4k.json
timeout -k 10 300 python3 -u bench.py --full --path of > $O/of.json
