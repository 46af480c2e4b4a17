"""An independent model of the accumulated-mask recurrence (frame_differencing.py:107,
``accumulated_mask = cv2.addWeighted(acc, r, dilated, 1 - r, 0)``) — plain numpy,
float64, no import of the oracle or of the library.

cv2.addWeighted on 8U planes takes its weights as doubles, converts them to
float32 and computes ``saturate_cast<uchar>(cvRound(acc * alpha + (dil * beta + gamma)))``
in float32, each multiply-add rounded once. Restated here as
``tests/golden/make_golden.py``'s addWeighted shim restates it:

* the weights are float32;
* ``inner = f32(dil * beta + gamma)`` and ``t = f32(acc * alpha + inner)``: a
  byte (8 bits) times a float32 (24 bits) is exact in float64 (53 bits), and so
  is the sum of that 32-bit product and a float32 unless the lowest bit of one
  lies more than 53 bits below the highest bit of the other, which no finite
  triple of ``acc_cases.py`` reaches: each
  float64 expression rounded to float32 is the float32 fused multiply-add;
* round half to even (cvRound), then saturate to [0, 255];
* NaN gives 0: cvRound(NaN) is INT_MIN (the "integer indefinite" of cvtss2si /
  lrint), and saturate_cast<uchar>(INT_MIN) is 0. A NaN arises from a NaN
  weight, from 0 * inf, or from inf - inf.
"""
import numpy as np


def add_weighted(acc, dil, alpha, beta, gamma):
    """One addWeighted of uint8 arrays (or scalars) ``acc`` and ``dil``; uint8 out."""
    al, be, ga = (np.float64(np.float32(v)) for v in (alpha, beta, gamma))
    a = np.asarray(acc, dtype=np.uint8).astype(np.float64)
    d = np.asarray(dil, dtype=np.uint8).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        inner = (d * be + ga).astype(np.float32)
        t = (a * al + inner.astype(np.float64)).astype(np.float32)
        r = np.rint(t.astype(np.float64))
    out = np.zeros(r.shape, np.uint8)            # NaN stays 0
    ok = ~np.isnan(r)
    out[ok] = np.clip(r[ok], 0.0, 255.0).astype(np.uint8)
    return out


def run(acc0, dilated_seq, alpha, beta, gamma):
    """The recurrence from ``acc0`` over the dilated planes (values 0 / 255), in
    order: the accumulated mask after each of them."""
    acc = np.asarray(acc0, dtype=np.uint8)
    out = []
    for d in dilated_seq:
        acc = add_weighted(acc, d, alpha, beta, gamma)
        out.append(acc)
    return out
