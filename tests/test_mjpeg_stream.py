"""CPU tests of the Motion-JPEG encoder's stream output (DESIGN.md "Motion-JPEG
stream", "Stream output"): the prototype of include/dvc_jpeg_stream.h against
_native's table, tools/jpeg_stream_host_check.cc — csrc/jpeg_stream_core.h, the
offset arithmetic the two stream kernels compile, built for the host under ASan
and UBSan — against a restatement in Python, and the muxer's block write. The
call itself is a GPU kernel chain: tests/test_mjpeg_stream_gpu.py."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_the_stream_call():
    """The prototype is declared in include/dvc_jpeg_stream.h, a header of its own over
    dvc.h, and bound from _native.JPEG_STREAM_SIGNATURES: dvc.h's prototypes and
    _native.EXPORTS are pinned, so they are as they were, and the ABI is still 10."""
    from dvc_amd import _native as N
    from tests import test_host as TH
    src = open(os.path.join(ROOT, "include", "dvc_jpeg_stream.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert '#include "dvc.h"' in code
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(dvc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code):
        protos[name] = [TH._c_class(ret, False)] + [TH._c_class(p, True) for p in params.split(",")]
    assert list(protos) == list(N.JPEG_STREAM_SIGNATURES) == ["dvc_jpeg_encode_stream"]
    assert TH._signature_mismatches(protos, N.JPEG_STREAM_SIGNATURES) == []
    assert protos["dvc_jpeg_encode_stream"] == ["i32", "ptr", "ptr", "u64", "u64", "i32", "ptr", "u64", "ptr"]
    assert not set(N.JPEG_STREAM_SIGNATURES) & set(N.EXPORTS)
    assert N.ABI_VERSION == 10 and "#define DVC_ABI_VERSION 10" in open(os.path.join(ROOT, "include", "dvc.h")).read()


def test_abi_declares_the_stream_handle_calls():
    """include/dvc_stream.h (the stream the drivers' handles join, created and destroyed per run)
    against _native.STREAM_SIGNATURES."""
    from dvc_amd import _native as N
    from tests import test_host as TH
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvc_stream.h")).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(dvc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code):
        protos[name] = [TH._c_class(ret, False)] + [TH._c_class(p, True) for p in params.split(",")]
    assert list(protos) == list(N.STREAM_SIGNATURES) == ["dvc_stream_create", "dvc_stream_destroy"]
    assert TH._signature_mismatches(protos, N.STREAM_SIGNATURES) == []
    assert not set(N.STREAM_SIGNATURES) & set(N.EXPORTS)


def _expected(hl, mb, cap, n, nseg, prefix, seglen):
    """The layout of the header's text, restated: (overflow, offsets, fits, segment starts)."""
    need = [hl + prefix[t // mb] + sum(v + 2 for v in seglen[t * nseg:(t + 1) * nseg]) for t in range(n)]
    offsets = [sum(need[:t]) for t in range(n + 1)]
    fits = [int(offsets[t + 1] <= cap) for t in range(n)]
    starts = [hl + prefix[t // mb] + sum(v + 2 for v in seglen[t * nseg:t * nseg + s])
              for t in range(n) for s in range(nseg)]
    return int(not all(fits)), offsets, fits, starts


def _cases():
    rng = np.random.default_rng(7)
    out = {}

    def add(name, hl, mb, cap, n, nseg, prefix=None, seglen=None):
        groups = -(-n // mb)
        prefix = [0] * groups if prefix is None else prefix
        seglen = [int(v) for v in rng.integers(0, 300, n * nseg)] if seglen is None else seglen
        out[name] = (hl, mb, cap, n, nseg, prefix, seglen)

    add("no_frames", 623, 8, 100, 0, 3)                                   # zero-length lists
    add("no_segments", 623, 2, 10 ** 6, 3, 0, prefix=[40, 41])            # a frame without segments
    add("empty_segments", 20, 4, 10 ** 6, 2, 5, seglen=[0] * 10)          # segments of no bytes
    add("one_frame", 623, 8, 10 ** 6, 1, 1)
    add("one_frame_long", 337, 1, 10 ** 6, 1, 300)                        # more segments than lanes and threads
    add("group_boundary", 623, 2, 10 ** 6, 5, 3, prefix=[100, 77, 431])   # the carry, a prefix per group
    add("group_exact", 331, 4, 10 ** 6, 8, 2, prefix=[60, 61])            # n a multiple of max_batch
    big = [2 ** 31 - 700] * 12
    add("past_2_32", 623, 2, 2 ** 40, 6, 2, seglen=big)                   # 64-bit offsets
    add("past_2_32_cap", 623, 2, 2 ** 33 + 5, 6, 2, seglen=big)           #... against a cap between two samples
    # cap on either side of a sample's end: the last one, one in the middle, one at a group boundary
    hl, mb, n, nseg = 100, 2, 5, 3
    seglen = [int(v) for v in rng.integers(0, 200, n * nseg)]
    prefix = [10, 0, 33]
    _, offs, _, _ = _expected(hl, mb, 0, n, nseg, prefix, seglen)
    for t in (5, 3, 2, 1):
        for d in (-1, 0, 1):
            add(f"cap_end{t}{'m=p'[d + 1]}", hl, mb, offs[t] + d, n, nseg, prefix=prefix, seglen=seglen)
    add("cap_zero", hl, mb, 0, n, nseg, prefix=prefix, seglen=seglen)
    return out


def test_host_program_under_sanitizers(tmp_path):
    """jpeg_stream_core.h compiled for the host with ASan and UBSan into a stand-alone
    program and run on launch groups as the library runs them: offsets, the fits
    test and every segment's place equal the restatement above; the bytes of the
    samples that fit are written into a block of exactly ``cap`` bytes."""
    exe = tmp_path / "jpeg_stream_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), os.path.join(ROOT, "tools", "jpeg_stream_host_check.cc")], check=True)
    cases = _cases()
    text = "".join(f"{name} {hl} {mb} {cap} {n} {nseg}\n{' '.join(map(str, prefix))}\n{' '.join(map(str, seglen))}\n"
                   for name, (hl, mb, cap, n, nseg, prefix, seglen) in cases.items())
    (tmp_path / "cases.txt").write_text(text)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {ln.split()[0]: ln.split(None, 1)[1] for ln in r.stdout.splitlines()}
    assert sorted(lines) == sorted(cases)
    for name, case in cases.items():
        head, offs, fits, starts = (s.split() for s in lines[name].split("|"))
        got = (int(head[0]), [int(v) for v in offs], [int(v) for v in fits], [int(v) for v in starts])
        assert got == _expected(*case), name
    assert _expected(*cases["past_2_32"])[1][-1] > 2 ** 32
    assert _expected(*cases["past_2_32_cap"])[2] == [1, 1, 0, 0, 0, 0]
    assert _expected(*cases["cap_end5m"])[2] == [1, 1, 1, 1, 0] and _expected(*cases["cap_end5="])[0] == 0


def test_muxer_writes_a_block_of_samples_as_add_sample_would(tmp_path):
    """Mp4Muxer.add_samples(buffer, offsets) leaves the file add_sample leaves for the
    same samples, one after the other."""
    from dvc_amd import video_io as V
    rng = np.random.default_rng(3)
    samples = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (5, 1, 300, 17, 64)]
    a, b = V.Mp4Muxer(str(tmp_path / "a.mp4"), 25, (16, 16)), V.Mp4Muxer(str(tmp_path / "b.mp4"), 25, (16, 16))
    for s in samples:
        a.add_sample(s)
    block = np.frombuffer(b"".join(samples) + b"tail", np.uint8)
    offs = np.cumsum([0] + [len(s) for s in samples]).astype(np.uint64)
    b.add_samples(block, offs[:3])        # two calls: the file position carries over
    b.add_samples(block, offs[2:])
    a.close()
    b.close()
    assert (tmp_path / "a.mp4").read_bytes() == (tmp_path / "b.mp4").read_bytes()
