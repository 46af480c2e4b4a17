"""Hashes of what the HIP accumulate stage produces on the clip of acc_cases.py,
for test_acc_gpu.py's comparison of k_acc's short form with its general form.

The library reads DVC_ACC_GENERAL when a handle is created. The test calls
:func:`hashes` in-process (short form) and runs this module as a fresh child
with DVC_ACC_GENERAL=1, which prints the same dictionary as JSON; each entry
carries the form its handles report (dvc_fd_acc_form), which the test asserts.
"""
import hashlib
import json
import sys

import numpy as np

from tests import acc_cases as C

GEOMS = [(262, 258, 4), (262, 258, 8)]   # full and partial blocks of both k_acc<B>


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def hashes():
    """{"<row>-<W>x<H>-b<B>": {"overlay": [...], "compressed": [...], "acc": [...]}}:
    every frame's overlay and compressed of one 33-frame launch from the seeded
    state, and every frame's accumulated mask of the same frames stepped one a call."""
    import dvc_amd
    N = dvc_amd._native
    out = {}
    for W, H, B in GEOMS:
        frames, seed = C.clip(W, H), C.seed_plane(W, H)
        n = C.N_FRAMES - 1
        for name in C.SHORT_VS_GENERAL:
            kw = C.worker_kwargs(C.BY_NAME[name], B)
            w = dvc_amd.FDWorker(W, H, max_batch=n, **kw)
            try:
                forms = [w.acc_form()]
                w.prime(frames[0])
                gray = w.plane(N.PLANE_GRAY)
                w.set_state(gray, seed)
                ov, cp = w.step_batch(frames[1:])
                last = w.plane(N.PLANE_ACC)
            finally:
                w.close()
            accs = []
            w = dvc_amd.FDWorker(W, H, **kw)
            try:
                forms.append(w.acc_form())
                w.set_state(gray, seed)
                acc = np.empty((H, W), np.uint8)
                for t in range(1, n + 1):
                    w.step(frames[t], acc=acc)
                    accs.append(_sha(acc))
            finally:
                w.close()
            assert accs[-1] == _sha(last), (name, W, H, B)
            out[f"{name}-{W}x{H}-b{B}"] = {"overlay": [_sha(f) for f in ov], "compressed": [_sha(f) for f in cp],
                                          "acc": accs, "forms": forms}
    return out


if __name__ == "__main__":
    json.dump(hashes(), sys.stdout)
