#!/bin/bash
# Build libdvc_hip.so with extra compiler flags into another path (A/B and
# debug builds, e.g. -DDVC_SCAN_STAMPS):  tools/build_variant.sh <out.so> [flags...]
# The sources are every csrc/*.hip, as _native.build() takes them.
set -e
cd "$(dirname "$0")/.."
OUT=$1; shift
C=dynamic-video-compression-surveillance_amd/csrc
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off "$@" -o "$OUT" $C/*.hip
