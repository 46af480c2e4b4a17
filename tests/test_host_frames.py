"""CPU: the frame contract of csrc/host_frames.h (what a frame spans, which
pitches it may have, how a host frame is packed, how a bit plane reads back)
as a stand-alone program under ASan and UBSan — tools/host_frames_check.cc,
whose buffers are heap blocks of exactly the span and exactly the packed size —
against a numpy restatement of include/dvc.h's frame layout written here."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(nbytes):
    return ((7 * np.arange(nbytes) + 3) % 256).astype(np.uint8)      # the program's source bytes


def _want_bgr():
    """10x6 BGR, rows 37 apart -> rows 36 apart; the six bytes between rows are never written."""
    span = 37 * 5 + 30
    src, out = _src(span), np.full(36 * 5 + 30, 0xEE, np.uint8)
    for y in range(6):
        out[36 * y:36 * y + 30] = src[37 * y:37 * y + 30]
    return span, out


def _want_i420():
    """6x4 I420, luma pitch 10, chroma planes after 6 luma rows: U rows of pitch 5 at
    60, V after the U plane's 3 rows, at 75 -> Y 6x4, U 3x2, V 3x2, packed."""
    span = 10 * 6 * 3 // 2
    src = _src(span)
    y = src[:60].reshape(6, 10)[:4, :6]
    u = src[60:75].reshape(3, 5)[:2, :3]
    v = src[75:90].reshape(3, 5)[:2, :3]
    return span, np.concatenate([y.ravel(), u.ravel(), v.ravel()])


def _want_nv12():
    """6x4 NV12, pitch 9, the UV plane after 4 luma rows -> Y 6x4, UV 6x2, packed."""
    span = 9 * 4 * 3 // 2
    src = _src(span)
    return span, np.concatenate([src[:36].reshape(4, 9)[:, :6].ravel(), src[36:54].reshape(2, 9)[:, :6].ravel()])


def _want_bits():
    out = np.zeros((3, 70), np.uint8)
    out[:, [0, 63, 64, 69]] = 255
    return out.ravel()


def test_frame_contract_under_sanitizers(tmp_path):
    exe = tmp_path / "host_frames_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), os.path.join(ROOT, "tools", "host_frames_check.cc")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    span, pack, pitch_ok = {}, {}, {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "span":
            span[int(w[1])] = int(w[2])
        elif w[0] == "pack":
            pack[int(w[1])] = np.frombuffer(bytes.fromhex(w[2]), np.uint8)
        else:
            assert w[0] == "pitch_ok"
            pitch_ok[tuple(int(v) for v in w[1:4])] = int(w[4])
    for case, (want_span, want) in {1: _want_bgr(), 2: _want_i420(), 3: _want_nv12()}.items():
        assert span[case] == want_span, case
        assert np.array_equal(pack[case], want), case
    assert np.array_equal(pack[4], _want_bits())
    BGR, I420, NV12 = 0, 1, 2
    assert pitch_ok == {(BGR, 10, 29): 0, (BGR, 10, 30): 1, (I420, 6, 7): 0, (I420, 6, 8): 1, (NV12, 6, 7): 1}
