"""CPU: the colour arithmetic of csrc/color_core.h — the text every kernel
compiles — built for the host under ASan and UBSan as a stand-alone program
(tools/color_host_check.cc) with the oracle's C files, and swept over all 2^24
inputs of each conversion: BGR2GRAY (scalar and v_dot4 forms), BGR2YCrCb,
YCrCb2BGR and their round trip, and BT.601 BGR2YUV_I420 / YUV2BGR_I420 / _NV12."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("color")
    objs = []
    for name in ("dvc_oracle.c", "contours_literal.c", "yuv_oracle.c"):
        obj = tmp / (name[:-2] + ".o")
        subprocess.run(["gcc", "-std=c11", *SAN, "-c", os.path.join(ROOT, "oracle", name), "-o", str(obj)], check=True)
        objs.append(str(obj))
    out = tmp / "color_host_check"
    subprocess.run(["g++", "-std=c++17", *SAN, "-o", str(out), os.path.join(ROOT, "tools", "color_host_check.cc"),
                    *objs, "-lm"], check=True)
    return str(out)


# the whole program takes about 15 s on one core: one test per part, every sweep in full
@pytest.mark.parametrize("part,sweeps", [("gray", 1), ("ycrcb", 2), ("bt601", 3)])
def test_host_program_under_sanitizers(exe, part, sweeps):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, part], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"%d sweeps of 2\^24 triples, 0 mismatches" % sweeps, r.stdout), r.stdout
    print(r.stdout.strip())
