"""Per-kernel instruction-stream comparison of two csrc trees (CPU).

    python tools/kernel_isa_diff.py <parent csrc dir> <new csrc dir> [--json out.json]

Compiles every *_kernels.hip of both trees for gfx950, device code only, with
the library's flags, disassembles the code objects and compares the kernels by
symbol: which are gone, which are added, and which survivors differ. A stream
is normalised by dropping the disassembler's `//` comments and blanking the
literal of the s_add_u32 that follows an s_getpc_b64 (the pc-relative offset
of a read-only table, which moves when other kernels come or go). The parent
tree is a `git worktree add` or `git archive` of the parent commit in a
temporary directory outside the repository.
"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "--offload-device-only", "--no-gpu-bundle-output", "-c"]


def kernels(src, obj):
    """{kernel symbol: normalised instruction list} and the code object's size."""
    if not os.path.exists(src):
        return {}, 0
    subprocess.run([os.path.join(ROCM, "bin", "hipcc"), *FLAGS, src, "-o", obj], check=True)
    objdump = os.path.join(ROCM, "llvm", "bin", "llvm-objdump")
    syms = subprocess.run([objdump, "-t", obj], check=True, capture_output=True, text=True).stdout
    # a kernel is a function with a kernel descriptor <name>.kd beside it
    kds = {m.group(1) for m in re.finditer(r"\s(\S+)\.kd$", syms, re.M)}
    dis = subprocess.run([objdump, "-d", "--no-show-raw-insn", "--no-leading-addr", obj], check=True,
                         capture_output=True, text=True).stdout
    out, cur, getpc = {}, None, False
    for line in dis.split("\n"):
        m = re.match(r"<(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in kds else None
            continue
        ins = line.split("//")[0].strip()
        if cur is None or not ins:
            continue
        if getpc and ins.startswith("s_add_u32"):
            ins = ins.rsplit(",", 1)[0] + ", <pcrel>"
        getpc = ins.startswith("s_getpc_b64")
        cur.append(ins)
    return out, os.path.getsize(obj)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--json", help="also write the result to this file")
    a = ap.parse_args()
    names = sorted({os.path.basename(p) for d in (a.parent, a.new) for p in glob.glob(os.path.join(d, "*_kernels.hip"))})
    res = {"gone": [], "added": [], "differ": [], "files": {}}
    with tempfile.TemporaryDirectory() as tmp:
        with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as pool:   # the compiles are child processes
            jobs = [[pool.submit(kernels, os.path.join(d, n), os.path.join(tmp, f"{i}_{n}.o"))
                     for i, d in enumerate((a.parent, a.new))] for n in names]
        for n, job in zip(names, jobs):
            (pk, pb), (nk, nb) = (j.result() for j in job)
            res["gone"] += sorted(set(pk) - set(nk))
            res["added"] += sorted(set(nk) - set(pk))
            res["differ"] += sorted(k for k in set(pk) & set(nk) if pk[k] != nk[k])
            res["files"][n] = {t: {"kernels": len(k), "instructions": sum(map(len, k.values())), "code_object_bytes": b}
                               for t, k, b in (("parent", pk, pb), ("new", nk, nb))}
    filt = subprocess.run(["c++filt"], input="\n".join(res["gone"] + res["added"] + res["differ"]), capture_output=True,
                          text=True).stdout.split("\n")
    dem = iter(re.sub(r"^void |\(.*", "", d) for d in filt)
    for key in ("gone", "added", "differ"):
        print(f"{key}: {len(res[key])}")
        res[key] = [{"symbol": s, "name": next(dem)} for s in res[key]]
        for k in res[key]:
            print(f"  {k['name']}")
    for n, f in res["files"].items():
        for t in ("parent", "new"):
            print(f"{n:22s} {t:6s} kernels {f[t]['kernels']:3d}  instructions {f[t]['instructions']:7d}  "
                  f"code object {f[t]['code_object_bytes']} B")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
