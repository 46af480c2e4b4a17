"""ctypes binding of ``libdvc_hip.so`` — the C-ABI declared in ``include/dvc.h``.

The reference has no FFI: it calls ``cv2.*`` inside the per-frame loop of
``frame_differencing.py:85-138``. This module is the thin layer that replaces
those calls with one ``dvc_fd_step`` per frame (or one ``dvc_fd_step_batch``
per run of frames). There is deliberately no CPU
fallback: if the HIP library is missing or fails to load, :func:`lib` raises.
"""
from __future__ import annotations

import ctypes
import glob
import os
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.path.join(PKG_DIR, "libdvc_hip.so")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"]

DVC_OK = 0
DVC_E_INVALID, DVC_E_HIP, DVC_E_STATE, DVC_E_NOMEM, DVC_E_UNSUPPORTED = -1, -2, -3, -4, -5
DVC_E_ODD_DCT = -6
DVC_FLAG_DEVICE_PTRS = 0x1
DVC_FLAG_KTIMING = 0x2
DVC_FLAG_KEEP_PLANES = 0x4
DVC_FLAG_JOIN_STREAM = 0x8
DVC_FLAG_OF_DIRECT_SUMS = 0x10
DVC_FLAG_OUT_I420 = 0x20
DVC_FLAG_FD_UNFUSED = 0x40
DVC_FLAG_FD_KEPT_PLANE = 0x80
DVC_FLAG_JPEGD_CAMERA = 0x100
DVC_FLAG_JPEG_OPT_HUFFMAN = 0x200
JPEG_OPT_PREFIX_MAX = 434                  # DVC_JPEG_OPT_PREFIX_MAX: the longest DHT + SOS in front of a frame
JPEG_RATE_PREFIX_MAX = 138 + JPEG_OPT_PREFIX_MAX   # DVC_JPEG_RATE_PREFIX_MAX: DQT, DQT in front of that
KTIME_OUT, KTIME_FRONT_FUSED = 0, 1         # dvc_fd_ktime_kernel: which kernel KTIMING timed
KTIME_FLOW, KTIME_FLOW_SCAN, KTIME_FLOW_SCAN2 = 2, 3, 4   # dvc_of_ktime_kernel: the level-0 flow kernel
ACC_FORM_GENERAL, ACC_FORM_SHORT, ACC_FORM_ROWS = 0, 1, 2   # dvc_fd_acc_form: the accumulate kernel of a handle
FMT_BGR, FMT_I420, FMT_NV12 = 0, 1, 2      # DVC_FMT_* frame formats (video I/O)
FMT_GRAY = 3                               # DVC_FMT_GRAY: one channel (the JPEG encoder's mask videos)
FORMATS = {"BGR": FMT_BGR, "I420": FMT_I420, "NV12": FMT_NV12}

PLANE_GRAY, PLANE_MOTION, PLANE_FILTERED, PLANE_ACC, PLANE_DILATED = range(5)
OF_PLANE_RAW, OF_PLANE_SMOOTH, OF_PLANE_MORPH, OF_PLANE_RECT, OF_PLANE_GRAY = range(5)

ABI_VERSION = 10
MAX_BATCH = 512


class DvcError(RuntimeError):
    """A negative status from the C-ABI (message from dvc_last_error)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"dvc error {code}: {msg}")
        self.code = code


class FdParams(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("block", ctypes.c_int32),
        ("ithresh", ctypes.c_int32),
        ("min_area2", ctypes.c_int64),
        ("ksize", ctypes.c_int32),
        ("anchor", ctypes.c_int32),
        ("alpha", ctypes.c_float),
        ("beta", ctypes.c_float),
        ("gamma", ctypes.c_float),
        ("quant", ctypes.c_float),
        ("prime_ksize", ctypes.c_int32),
        ("prime_sigma", ctypes.c_double),
        ("flags", ctypes.c_uint32),
        ("max_batch", ctypes.c_uint32),
        ("src_width", ctypes.c_int32),
        ("src_height", ctypes.c_int32),
        ("in_format", ctypes.c_int32),
        ("chroma_rows", ctypes.c_int32),
    ]


class FdStats(ctypes.Structure):
    _fields_ = [
        ("frames", ctypes.c_uint64),
        ("motion_px", ctypes.c_uint64),
        ("components", ctypes.c_uint64),
        ("static_blocks", ctypes.c_uint64),
    ]


class OfParams(ctypes.Structure):
    """``dvc_of_params`` (include/dvc.h)."""
    _fields_ = [
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("flow_threshold", ctypes.c_float),
        ("quant", ctypes.c_float),
        ("alpha_fraction", ctypes.c_double),
        ("window", ctypes.c_int32),
        ("morph_kernel", ctypes.c_int32),
        ("pyr_scale", ctypes.c_double),
        ("levels", ctypes.c_int32),
        ("winsize", ctypes.c_int32),
        ("iterations", ctypes.c_int32),
        ("poly_n", ctypes.c_int32),
        ("poly_sigma", ctypes.c_double),
        ("flags", ctypes.c_uint32),
        ("max_batch", ctypes.c_uint32),
        ("in_format", ctypes.c_int32),
        ("chroma_rows", ctypes.c_int32),
    ]


OfStats = FdStats   # same four counters (dvc_of_stats)


def sources() -> list:
    """What the library is compiled from: every csrc/*.hip (tools/build_variant.sh takes the same files)."""
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = sources()
    deps = srcs + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(PKG_DIR, "..", "include", "*.h"))
    if not force and os.path.exists(LIB_PATH):
        newest = max(os.path.getmtime(d) for d in deps)
        if os.path.getmtime(LIB_PATH) >= newest:
            return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    tmp = LIB_PATH + ".tmp"
    cmd = [hipcc, *HIPCC_FLAGS, "-o", tmp, *srcs]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


# The C-ABI: name -> (restype, argtypes), one entry per function include/dvc.h
# declares, in the header's order. lib() binds exactly this table and
# tests/test_host.py checks every entry against the header's prototype.
_I, _Z, _P, _U32, _F, _D = (ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float,
                            ctypes.c_double)
_PI, _PZ, _PD, _PU64, _PP = (ctypes.POINTER(t) for t in (_I, _Z, _D, ctypes.c_uint64, _P))
SIGNATURES = {
    # standalone conversions
    "dvc_yuv420_to_bgr": (_I, (_P, _Z, _I, _I, _I, _I, _I, _Z, _P, _Z, _Z, _I, _P, _U32)),
    "dvc_bgr_to_i420": (_I, (_P, _Z, _Z, _I, _I, _I, _P, _Z, _I, _Z, _I, _P, _U32)),
    # library / device introspection, page-locked host memory
    "dvc_abi_version": (_I, ()),
    "dvc_last_error": (ctypes.c_char_p, ()),
    "dvc_device_count": (_I, (_PI,)),
    "dvc_host_alloc": (_I, (_Z, _PP)),
    "dvc_host_free": (None, (_P,)),
    # frame-differencing path
    "dvc_fd_create": (_I, (ctypes.POINTER(FdParams), _I, _P, _PP)),
    "dvc_fd_prime": (_I, (_P, _P, _Z)),
    "dvc_fd_set_state": (_I, (_P, _P, _P)),
    "dvc_fd_step": (_I, (_P, _P, _Z, _P, _P, _P)),
    "dvc_fd_step_batch": (_I, (_P, _P, _Z, _Z, _I, _P, _P, _Z)),
    "dvc_fd_sync": (_I, (_P,)),
    "dvc_fd_get_stats": (_I, (_P, ctypes.POINTER(FdStats))),
    "dvc_fd_read_plane": (_I, (_P, _I, _P)),
    "dvc_fd_ktime": (_I, (_P, _PD, _PU64, _I)),
    "dvc_fd_ktime_kernel": (_I, (_P,)),
    "dvc_fd_acc_form": (_I, (_P,)),
    "dvc_fd_graph_stats": (_I, (_P, _PU64, _PU64)),
    "dvc_fd_destroy": (None, (_P,)),
    "dvc_contour_filter": (_I, (_P, _I, _I, ctypes.c_int64, _I, _P, _PU64)),
    # optical-flow path
    "dvc_of_create": (_I, (ctypes.POINTER(OfParams), _I, _P, _PP)),
    "dvc_of_prime": (_I, (_P, _P, _Z)),
    "dvc_of_set_state": (_I, (_P, _P, _P, _I)),
    "dvc_of_step": (_I, (_P, _P, _Z, _P, _P)),
    "dvc_of_step_batch": (_I, (_P, _P, _Z, _Z, _I, _P, _Z, _P, _Z)),
    "dvc_of_sync": (_I, (_P,)),
    "dvc_of_get_stats": (_I, (_P, ctypes.POINTER(OfStats))),
    "dvc_of_read_plane": (_I, (_P, _I, _P)),
    "dvc_of_read_flow": (_I, (_P, _P)),
    "dvc_of_ktime": (_I, (_P, _PD, _PU64, _I)),
    "dvc_of_ktime_kernel": (_I, (_P,)),
    "dvc_of_destroy": (None, (_P,)),
    "dvc_of_debug_read": (_I, (_P, _I, _I, _P, _PI, _PI)),
    "dvc_of_compress": (_I, (_P, _Z, _P, _I, _I, _F, _I, _P)),
    "dvc_ofc_create": (_I, (_I, _I, _F, _I, _I, _P, _U32, _PP)),
    "dvc_ofc_run": (_I, (_P, _P, _Z, _Z, _P, _Z, _Z, _I, _I, _P, _Z)),
    "dvc_ofc_sync": (_I, (_P,)),
    "dvc_ofc_destroy": (None, (_P,)),
    # Motion-JPEG encoder and decoder
    "dvc_jpeg_create": (_I, (_I, _I, _I, _I, _I, _I, _P, _U32, _PP)),
    "dvc_jpeg_destroy": (None, (_P,)),
    "dvc_jpeg_header": (_I, (_P, _P, _Z, _PZ)),
    "dvc_jpeg_bound": (_I, (_I, _I, _I, _PZ)),
    "dvc_jpeg_encode": (_I, (_P, _P, _Z, _Z, _I, _P, _Z, _P)),
    "dvc_jpeg_sync": (_I, (_P,)),
    "dvc_jpegd_create": (_I, (_I, _I, _I, _I, _P, _U32, _PP)),
    "dvc_jpegd_destroy": (None, (_P,)),
    "dvc_jpegd_set_header": (_I, (_P, _P, _Z, _PZ, _PI, _PI, _PI)),
    "dvc_jpegd_decode": (_I, (_P, _P, _Z, _P, _I, _P, _Z, _Z, _P)),
    "dvc_jpegd_sync": (_I, (_P,)),
    # quality metrics
    "dvc_quality_create": (_I, (_I, _I, _I, _I, _P, _U32, _PP)),
    "dvc_quality_compare": (_I, (_P, _P, _Z, _Z, _P, _Z, _Z, _I, _P)),
    "dvc_quality_sync": (_I, (_P,)),
    "dvc_quality_destroy": (None, (_P,)),
    # parity helpers and diagnostics
    "dvc_gaussian_taps_q8": (_I, (_I, _D, ctypes.POINTER(ctypes.c_uint16))),
    "dvc_copy_rate": (_I, (_I, _Z, _I, _I, _PD)),
}
EXPORTS = list(SIGNATURES)
# What include/dvc_quality_regions.h declares, bound the same way.
REGION_SIGNATURES = {
    "dvc_quality_compare_regions": (_I, (_P, _P, _Z, _Z, _P, _Z, _Z, _P, _Z, _Z, _I, _I, _I, _P)),
}
# What include/dvc_jpeg_opt.h declares.
JPEG_OPT_SIGNATURES = {
    "dvc_jpeg_opt_tables": (_I, (_P, _PU64, _P, _Z, _PZ)),
}
# What include/dvc_jpeg_stream.h declares.
JPEG_STREAM_SIGNATURES = {
    "dvc_jpeg_encode_stream": (_I, (_P, _P, _Z, _Z, _I, _P, _Z, _P)),
}
# What include/dvc_jpeg_rate.h declares.
JPEG_RATE_SIGNATURES = {
    "dvc_jpeg_create_rate": (_I, (_I, _I, _I, _Z, _I, _I, _I, _I, _P, _U32, _PP)),
    "dvc_jpeg_rate_stats": (_I, (_P, _P)),
}
JPEG_RATE_STATS = ("groups", "frames", "missed_groups", "est_bytes", "budget_bytes", "quality_frames", "q_lowest",
                   "q_highest", "q_last")   # struct dvc_jpeg_rate_stats: uint64_t each
# What include/dvc_stream.h declares.
STREAM_SIGNATURES = {
    "dvc_stream_create": (_I, (_I, _PP)),
    "dvc_stream_destroy": (_I, (_I, _P)),
}
# An older build loaded for an A/B run (DVC_LIB_PATH with DVC_ALLOW_ABI_MISMATCH=1)
# may lack these; FDWorker.ktime_kernel and OFWorker.ktime_kernel fall back.
OPTIONAL = ("dvc_fd_ktime_kernel", "dvc_fd_acc_form", "dvc_fd_graph_stats", "dvc_of_ktime_kernel")

_lib = None


def lib() -> ctypes.CDLL:
    """Load libdvc_hip.so. Raises (never falls back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("DVC_LIB_PATH") or LIB_PATH   # override: A/B runs of two builds
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (the HIP path has no CPU fallback)")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (same
    # SONAME). Loading torch first makes libdvc_hip.so bind to that instance, so
    # torch tensors/streams and this library share devices and streams; loading
    # /opt/rocm's copy first would leave torch without a usable GPU.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(path)
    if L.dvc_abi_version() != ABI_VERSION:   # (int (void): callable as loaded)
        # a library with another dvc_fd_params / flag layout would corrupt
        # memory: refuse it unless the caller opts in explicitly (A/B of builds
        # from an older tree whose layout is known to match)
        if os.environ.get("DVC_ALLOW_ABI_MISMATCH") != "1":
            raise ImportError(f"{path}: ABI version {L.dvc_abi_version()} != {ABI_VERSION} "
                              "(set DVC_ALLOW_ABI_MISMATCH=1 to load it anyway)")
        import warnings
        warnings.warn(f"{path}: ABI version mismatch accepted (DVC_ALLOW_ABI_MISMATCH=1)")
    for name, (restype, argtypes) in {**SIGNATURES, **REGION_SIGNATURES, **JPEG_OPT_SIGNATURES,
                                      **JPEG_STREAM_SIGNATURES, **JPEG_RATE_SIGNATURES, **STREAM_SIGNATURES}.items():
        # (such a build also lacks the stream output: encode_stream raises, the drivers keep the host path;
        # and the rate target: JpegEncoder(target_bytes=...) raises)
        if (name in OPTIONAL or name in JPEG_STREAM_SIGNATURES or name in JPEG_RATE_SIGNATURES
                or name in STREAM_SIGNATURES) and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != DVC_OK:
        msg = lib().dvc_last_error()
        raise DvcError(rc, msg.decode() if msg else "")


class Handle:
    """Owner of one C-ABI handle: the lifecycle the six handle classes share.
    ``_h`` is None until :meth:`_create` succeeds and again after :meth:`close`,
    so an object whose constructor raised closes and collects silently."""
    _destroy = ""   # the class's dvc_*_destroy
    _h = None

    def _create(self, create, *args) -> None:
        """``create(*args, &handle)``; the handle is kept only when the status is DVC_OK."""
        h = ctypes.c_void_p()
        check(create(*args, ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        h, self._h = self._h, None
        if h:
            getattr(lib(), self._destroy)(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Pinned:
    """Owner of one dvc_host_alloc block (freed when the last view dies)."""

    def __init__(self, nbytes: int):
        p = ctypes.c_void_p()
        check(lib().dvc_host_alloc(int(nbytes), ctypes.byref(p)))
        self.ptr, self.nbytes = p.value, int(nbytes)

    def __del__(self):
        try:
            lib().dvc_host_free(ctypes.c_void_p(self.ptr))
        except Exception:
            pass


def pinned(shape, dtype="uint8"):
    """A numpy array in page-locked host memory (dvc_host_alloc): host-pointer
    steps DMA such buffers directly, with no staging copy on the CPU."""
    import numpy as np
    dt = np.dtype(dtype)
    count = int(np.prod(shape))
    owner = _Pinned(max(count * dt.itemsize, 1))
    buf = (ctypes.c_uint8 * max(count * dt.itemsize, 1)).from_address(owner.ptr)
    buf._owner = owner          # every view of the array keeps the block alive
    return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


def contour_filter(mask, min_area2: int, device: int = 0):
    """fd:100-104 on the GPU for one host mask; returns (filtered, components)."""
    import numpy as np
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    H, W = m.shape
    out = np.empty_like(m)
    nc = ctypes.c_uint64()
    check(lib().dvc_contour_filter(m.ctypes.data, W, H, int(min_area2), int(device), out.ctypes.data,
                                   ctypes.byref(nc)))
    return out, int(nc.value)


def of_compress(bgr, mask, quant: float = 100.0, device: int = 0):
    """compress_with_motion for one frame with an arbitrary mask (of:151-183) on the GPU."""
    import numpy as np
    f = np.ascontiguousarray(bgr, dtype=np.uint8)
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    H, W = m.shape
    if f.shape != (H, W, 3):
        raise ValueError("frame and mask shapes differ")
    out = np.empty_like(f)
    check(lib().dvc_of_compress(f.ctypes.data, 3 * W, m.ctypes.data, W, H, float(quant), int(device),
                                out.ctypes.data))
    return out


class OFCompressor(Handle):
    """compress_with_motion's loop (of:141-185) on the GPU for chunks of frames
    (dvc_ofc): host numpy frames (n, H, W, 3) and decoded masks (n, H, W) or
    (n, H, W, 3) -> compressed frames (n, H, W, 3), or with
    ``out_format="I420"`` (DVC_FLAG_OUT_I420; W and H even) the encoder's 4:2:0
    frames (n, H*3/2, W)."""

    _destroy = "dvc_ofc_destroy"

    def __init__(self, width: int, height: int, quant: float = 100.0, max_batch: int = 32, device: int = 0,
                 out_format: str = "BGR"):
        if out_format not in ("BGR", "I420"):
            raise ValueError(f"out_format {out_format!r}: BGR or I420")
        self.out_format = out_format
        self.W, self.H, self.max_batch = int(width), int(height), max(1, int(max_batch))
        self._oshape = (self.H, self.W, 3) if out_format == "BGR" else (self.H * 3 // 2, self.W)
        self._obytes = self._oshape[0] * self._oshape[1] * (3 if out_format == "BGR" else 1)
        self._create(lib().dvc_ofc_create, self.W, self.H, float(quant), self.max_batch, int(device), None,
                     DVC_FLAG_OUT_I420 if out_format == "I420" else 0)

    def run(self, frames, masks, out=None):
        import numpy as np
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        m = np.ascontiguousarray(masks, dtype=np.uint8)
        if f.ndim == 3:
            f, m = f[None], m[None]
        n = f.shape[0]
        ch = 3 if m.ndim == 4 else 1
        if f.shape[1:] != (self.H, self.W, 3) or m.shape[:3] != (n, self.H, self.W):
            raise ValueError(f"frames {f.shape} / masks {m.shape} do not match {self.W}x{self.H}")
        if out is None:
            out = np.empty((n,) + self._oshape, np.uint8)
        elif out.dtype != np.uint8 or out.size != n * self._obytes or not out.flags.c_contiguous:
            raise ValueError(f"out: expected a contiguous uint8 array of shape {(n,) + self._oshape}")
        if n:
            check(lib().dvc_ofc_run(self._h, f.ctypes.data, 3 * self.W, f[0].nbytes, m.ctypes.data, self.W * ch,
                                    m[0].nbytes, ch, n, out.ctypes.data, self._obytes))
        return out


def yuv420_to_bgr(frames, fmt: str = "I420", device: int = 0):
    """cv2.cvtColor(COLOR_YUV2BGR_I420 / _NV12) on the GPU of host 4:2:0 frames:
    one (H*3/2, W) uint8 frame or an (n, H*3/2, W) stack -> (.., H, W, 3) BGR."""
    import numpy as np
    f = np.ascontiguousarray(frames, dtype=np.uint8)
    one = f.ndim == 2
    f = f[None] if one else f
    n, H, W = f.shape[0], f.shape[1] * 2 // 3, f.shape[2]
    if f.shape[1] != H * 3 // 2 or H % 2 or W % 2:
        raise ValueError(f"4:2:0 frames must be (H*3/2, W) with H, W even, got {f.shape[1:]}")
    out = np.empty((n, H, W, 3), np.uint8)
    check(lib().dvc_yuv420_to_bgr(f.ctypes.data, W, FORMATS[fmt], 0, W, H, n, f[0].nbytes, out.ctypes.data, 3 * W,
                                  3 * W * H, int(device), None, 0))
    return out[0] if one else out


def bgr_to_i420(frames, device: int = 0):
    """cv2.cvtColor(COLOR_BGR2YUV_I420) on the GPU of host BGR frames: (H, W, 3) or
    (n, H, W, 3) uint8 -> (.., H*3/2, W) I420."""
    import numpy as np
    f = np.ascontiguousarray(frames, dtype=np.uint8)
    one = f.ndim == 3
    f = f[None] if one else f
    n, H, W = f.shape[:3]
    if H % 2 or W % 2 or f.shape[3] != 3:
        raise ValueError(f"BGR frames must be (H, W, 3) with H, W even, got {f.shape[1:]}")
    out = np.zeros((n, H * 3 // 2, W), np.uint8)
    check(lib().dvc_bgr_to_i420(f.ctypes.data, 3 * W, 3 * W * H, W, H, n, out.ctypes.data, W, 0, out[0].nbytes,
                                int(device), None, 0))
    return out[0] if one else out


class JpegEncoder(Handle):
    """cv2.VideoWriter's codec end on the GPU (dvc_jpeg): host numpy frames,
    (n, H, W, 3) BGR or (n, H, W) single-channel, -> one ``bytes`` per frame, the
    frame's JFIF entropy data and EOI; ``header`` (SOI..SOS, constant per
    encoder) in front of it makes a complete baseline JPEG image.
    ``optimize=True`` (DVC_FLAG_JPEG_OPT_HUFFMAN): Huffman tables built on the
    GPU from the symbols of every run of ``max_batch`` frames of a call;
    ``header`` then ends with DRI, every frame's bytes begin with its run's DHT
    and SOS segments, ``bound`` includes them, and ``header`` + frame is a
    complete image as before. The bytes depend on ``max_batch`` and on how
    frames are grouped into calls, the decoded pixels do not.
    ``target_bytes`` (dvc_jpeg_create_rate): a byte target per frame in place of
    ``quality`` (then ignored; ``self.quality`` is None). Every run of
    ``max_batch`` frames of a call is coded at the quality of ``quality_range``
    that the search of DESIGN.md "Rate target" finds on the GPU; ``header`` then
    has no DQT and no SOS, every frame's bytes begin with DQT, DQT, [DHT,] SOS,
    and :meth:`rate_stats` tells what was chosen. The target bounds the size
    before byte stuffing with the fixed tables, not the file's."""

    _destroy = "dvc_jpeg_destroy"

    def __init__(self, width: int, height: int, is_color: bool = True, quality: int = 75, max_batch: int = 8,
                 device: int = 0, optimize: bool = False, device_ptrs: bool = False, stream=None,
                 target_bytes=None, quality_range=(10, 95)):
        """``device_ptrs`` (DVC_FLAG_DEVICE_PTRS): :meth:`encode_stream` takes torch
        CUDA tensors and is asynchronous on the handle's stream; ``stream``: the
        caller's HIP stream (``torch.cuda.Stream.cuda_stream``), joined."""
        self.target_bytes = None if target_bytes is None else int(target_bytes)
        self.quality_range = (int(quality_range[0]), int(quality_range[1]))
        self.quality = int(quality) if target_bytes is None else None
        self.W, self.H, self.is_color = int(width), int(height), bool(is_color)
        self.fmt = FMT_BGR if is_color else FMT_GRAY
        self.optimize = bool(optimize)
        self.device, self.device_ptrs, self.max_batch = int(device), bool(device_ptrs), max(1, int(max_batch))
        self._out = None
        flags = (DVC_FLAG_JPEG_OPT_HUFFMAN if self.optimize else 0) | (DVC_FLAG_DEVICE_PTRS if device_ptrs else 0) \
            | (DVC_FLAG_JOIN_STREAM if stream is not None else 0)
        hs = ctypes.c_void_p(int(stream)) if stream is not None else None
        if self.target_bytes is None:
            self._create(lib().dvc_jpeg_create, self.W, self.H, self.fmt, int(quality), self.max_batch, self.device, hs,
                         flags)
        else:
            if not hasattr(lib(), "dvc_jpeg_create_rate"):
                raise DvcError(DVC_E_UNSUPPORTED, "the loaded library has no dvc_jpeg_create_rate")
            if self.target_bytes < 0:
                raise ValueError(f"target_bytes {self.target_bytes} is negative")
            self._create(lib().dvc_jpeg_create_rate, self.W, self.H, self.fmt, self.target_bytes, *self.quality_range,
                         self.max_batch, self.device, hs, flags)
        h, n = self._h, ctypes.c_size_t()
        check(lib().dvc_jpeg_header(h, None, 0, ctypes.byref(n)))
        buf = (ctypes.c_uint8 * n.value)()
        check(lib().dvc_jpeg_header(h, buf, n.value, ctypes.byref(n)))
        self.header = bytes(buf)
        check(lib().dvc_jpeg_bound(self.W, self.H, self.fmt, ctypes.byref(n)))
        self.bound = int(n.value) + (JPEG_RATE_PREFIX_MAX if self.target_bytes is not None else
                                     JPEG_OPT_PREFIX_MAX if self.optimize else 0)

    def rate_stats(self) -> dict:
        """dvc_jpeg_rate_stats: the cumulative counters of a ``target_bytes`` encoder
        (waits for the handle's stream)."""
        if not hasattr(lib(), "dvc_jpeg_rate_stats"):
            raise DvcError(DVC_E_UNSUPPORTED, "the loaded library has no dvc_jpeg_rate_stats")
        if self._h is None and getattr(self, "_closed_stats", None) is not None:
            return dict(self._closed_stats)      # (a closed encoder still tells what it did)
        buf = (ctypes.c_uint64 * len(JPEG_RATE_STATS))()
        check(lib().dvc_jpeg_rate_stats(self._h, buf))
        return dict(zip(JPEG_RATE_STATS, (int(v) for v in buf)))

    def close(self) -> None:
        if self._h is not None and getattr(self, "target_bytes", None) is not None and self.device >= 0:
            try:
                self._closed_stats = self.rate_stats()
            except DvcError:
                pass
        super().close()

    def tables(self, counts) -> bytes:
        """dvc_jpeg_opt_tables: the DHT segment the encoder would write for the symbol
        counts ``counts[4][256]`` (DC class 0, AC class 0, DC class 1, AC class 1)."""
        import numpy as np
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        if c.shape != (4, 256):
            raise ValueError(f"counts {c.shape}: (4, 256) expected")
        n = ctypes.c_size_t()
        buf = (ctypes.c_uint8 * 2048)()
        check(lib().dvc_jpeg_opt_tables(self._h, c.ctypes.data_as(_PU64), buf, len(buf), ctypes.byref(n)))
        return bytes(buf[:n.value])

    @staticmethod
    def alloc(shape):
        """Page-locked frames for :meth:`encode` (DMA'd directly, no staging copy)."""
        return pinned(shape)

    def encode(self, frames) -> list:
        import numpy as np
        if self.device_ptrs:
            raise ValueError("encode takes host frames: a device_ptrs handle has encode_stream")
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        shape = (self.H, self.W, 3) if self.is_color else (self.H, self.W)
        if f.shape == shape:
            f = f[None]
        if f.shape[1:] != shape:
            raise ValueError(f"frames {f.shape} do not match {shape}")
        n = f.shape[0]
        if n == 0:
            return []
        row = f[0][0].nbytes
        sizes = np.zeros(n, np.uint32)
        # slots of the raw frame size almost always fit; the worst case is several times that
        for stride in (min(self.bound, max(4096, f[0].nbytes)), self.bound):
            if self._out is None or self._out.shape[0] < n or self._out.shape[1] != stride:
                self._out = pinned((n, stride))   # kept for the next call
            out = self._out
            rc = lib().dvc_jpeg_encode(self._h, f.ctypes.data, row, f[0].nbytes, n, out.ctypes.data, stride,
                                       sizes.ctypes.data)
            if rc != DVC_E_NOMEM or stride == self.bound:
                check(rc)
                break
        return [out[i, :int(sizes[i])].tobytes() for i in range(n)]

    def encode_stream(self, frames, out, offsets, pitch: int = 0) -> int:
        """dvc_jpeg_encode_stream: ``n`` frames -> complete samples (``header`` + what
        :meth:`encode` returns) back to back in ``out``, sample t at
        ``out[offsets[t]:offsets[t + 1]]``; returns ``n``. ``frames``: (n, H, W, 3) or
        (n, H, W) uint8, or with ``pitch`` rows of that many bytes, (n, H, pitch).
        ``out``: flat uint8, its length is ``cap``; ``offsets``: n + 1 words. On a
        ``device_ptrs`` handle they are torch CUDA tensors (``offsets`` int64) and the
        call is asynchronous: samples that do not fit ``out`` are not written and
        :meth:`sync` raises DVC_E_NOMEM. On a host handle they are numpy arrays
        (``offsets`` uint64) and the call itself raises it; ``offsets`` is complete
        either way."""
        import numpy as np
        from . import _buffers as B
        if not hasattr(lib(), "dvc_jpeg_encode_stream"):
            raise DvcError(DVC_E_UNSUPPORTED, "the loaded library has no dvc_jpeg_encode_stream")
        row = (3 if self.is_color else 1) * self.W
        tail = (self.H, int(pitch)) if pitch else ((self.H, self.W, 3) if self.is_color else (self.H, self.W))
        if pitch and pitch < row:
            raise ValueError(f"pitch {pitch} below a row's {row} bytes")
        if self.device_ptrs:
            fa, n = B.device_buf(frames, tail, self.device, "frames")
            oa = B.device_buf(out, tuple(out.shape[-1:]) if hasattr(out, "shape") else (), self.device, "out",
                              batched=False)[0]
            cap = int(out.numel()) if hasattr(out, "numel") else int(out[1])
            pa = B.device_words(offsets, n + 1, self.device, "offsets")
        else:
            if self._h is None or not isinstance(frames, np.ndarray) or frames.dtype != np.uint8 \
                    or frames.shape[1:] != tail or not frames.flags.c_contiguous:
                raise ValueError(f"frames: expected a C-contiguous uint8 numpy array of shape (n,) + {tail}")
            n = int(frames.shape[0])
            if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 1 \
                    or not out.flags.c_contiguous or not out.flags.writeable:
                raise ValueError("out: expected a writeable flat uint8 numpy array")
            if not isinstance(offsets, np.ndarray) or offsets.dtype != np.uint64 or offsets.ndim != 1 \
                    or offsets.size < n + 1 or not offsets.flags.c_contiguous or not offsets.flags.writeable:
                raise ValueError(f"offsets: expected a writeable uint64 numpy array of at least {n + 1} words")
            fa, oa, cap, pa = frames.ctypes.data, out.ctypes.data, int(out.size), offsets.ctypes.data
        rowp = int(pitch) if pitch else row
        check(lib().dvc_jpeg_encode_stream(self._h, fa, rowp, rowp * self.H, n, oa, cap, pa))
        return n

    def sync(self) -> None:
        """Wait for the handle's stream; raises what an asynchronous call could not (DVC_E_NOMEM)."""
        check(lib().dvc_jpeg_sync(self._h))


class JpegDecoder(Handle):
    """cv2.VideoCapture's codec end on the GPU (dvc_jpegd): whole JPEG samples
    (``bytes``, as Mp4MjpegReader.read_sample returns them) -> numpy frames,
    (H, W, 3) BGR or (H, W) for a single-component stream, the bytes Pillow
    gives. The header (SOI..SOS) is parsed on the host, again only when a
    sample's header bytes differ from the last one's; a stream outside the
    decoder's set raises DvcError with code DVC_E_UNSUPPORTED. ``camera=True``
    (DVC_FLAG_JPEGD_CAMERA) widens that set to what cameras and AVI files emit:
    4:2:2 and 4:4:4 sampling and frames without DHT segments."""

    _destroy = "dvc_jpegd_destroy"

    def __init__(self, max_width: int, max_height: int, max_batch: int = 8, device: int = 0, camera: bool = False,
                 device_ptrs: bool = False, stream=None):
        """``device_ptrs`` (DVC_FLAG_DEVICE_PTRS): the handle decodes with
        :meth:`decode_device`, asynchronously on its stream; ``stream``: the caller's
        HIP stream (``torch.cuda.Stream.cuda_stream``), joined."""
        self.max_batch = max(1, int(max_batch))
        self.device, self.device_ptrs = int(device), bool(device_ptrs)
        self._in = self._out = None
        self._hdr, self.W, self.H, self.fmt = None, 0, 0, FMT_BGR
        flags = (DVC_FLAG_JPEGD_CAMERA if camera else 0) | (DVC_FLAG_DEVICE_PTRS if device_ptrs else 0) \
            | (DVC_FLAG_JOIN_STREAM if stream is not None else 0)
        self._create(lib().dvc_jpegd_create, int(max_width), int(max_height), self.max_batch, self.device,
                     ctypes.c_void_p(int(stream)) if stream is not None else None, flags)

    def decode_device(self, data, header_len: int, sizes, out, status, n: int) -> None:
        """dvc_jpegd_decode with device pointers, asynchronous: ``n`` whole samples that
        share the current header (:meth:`set_header`), sample t from the start of slot t
        of ``data`` — a torch CUDA uint8 tensor (slots, stride), uploaded as read from
        the file — decoded from byte ``header_len`` of its slot on. ``sizes``: CUDA
        int32, the bytes of each sample behind its header (the caller keeps
        ``header_len + sizes[t] <= stride``); ``out``: CUDA uint8 (>= n, H, W, 3), or
        (>= n, H, W) for a single-component stream; ``status``: CUDA int32, 0 or a
        negative DVC_E_* per frame (a damaged frame is not written). :meth:`sync`
        waits."""
        from . import _buffers as B
        if not self.device_ptrs:
            raise ValueError("decode_device needs a device_ptrs handle")
        if self._hdr is None or int(header_len) != len(self._hdr):
            raise ValueError("header_len is not the current header's length")
        n = int(n)
        if not 0 < n <= self.max_batch:
            raise ValueError(f"{n} samples: 1..{self.max_batch} a call")
        stride = int(data.shape[1]) if hasattr(data, "shape") and len(data.shape) == 2 else 0
        if stride <= header_len:
            raise ValueError("data: expected (slots, stride) with stride above header_len")
        da = B.device_buf(data, (stride,), self.device, "data", n=n)[0]
        shape = (self.H, self.W, 3) if self.fmt == FMT_BGR else (self.H, self.W)
        oa = B.device_buf(out, shape, self.device, "out", n=n)[0]
        sa = B.device_words(sizes, n, self.device, "sizes", "int32")
        ta = B.device_words(status, n, self.device, "status", "int32")
        pitch = shape[1] * (3 if self.fmt == FMT_BGR else 1)
        check(lib().dvc_jpegd_decode(self._h, da + int(header_len), stride, sa, n, oa, pitch, pitch * self.H, ta))

    def sync(self) -> None:
        """Wait for the handle's stream. A damaged frame of an asynchronous call is
        reported in its ``status`` word; the first such status is raised here, once."""
        check(lib().dvc_jpegd_sync(self._h))

    def set_header(self, sample: bytes) -> int:
        """Parse ``sample``'s header; returns its length (where the entropy data starts)."""
        n, w, hh, fmt = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().dvc_jpegd_set_header(self._h, sample, len(sample), ctypes.byref(n), ctypes.byref(w), ctypes.byref(hh),
                                         ctypes.byref(fmt)))
        self._hdr, self.W, self.H, self.fmt = bytes(sample[:n.value]), w.value, hh.value, fmt.value
        return n.value

    def _run(self, samples):
        """Samples that share the current header -> frames (None from the first damaged one on)."""
        import numpy as np
        hl, n = len(self._hdr), len(samples)
        stride = (max(len(s) for s in samples) - hl + 3) & ~3
        if self._in is None or self._in.shape[0] < n or self._in.shape[1] < stride:
            self._in = pinned((max(n, self.max_batch), max(stride, 4096)))
        shape = (self.H, self.W, 3) if self.fmt == FMT_BGR else (self.H, self.W)
        if self._out is None or self._out.shape[0] < n or self._out.shape[1:] != shape:
            self._out = pinned((max(n, self.max_batch),) + shape)
        sizes, status = np.zeros(n, np.uint32), np.zeros(n, np.int32)
        for i, s in enumerate(samples):
            sizes[i] = len(s) - hl
            self._in[i, :sizes[i]] = np.frombuffer(s, np.uint8, sizes[i], hl)
        out = self._out
        rc = lib().dvc_jpegd_decode(self._h, self._in.ctypes.data, self._in.shape[1], sizes.ctypes.data, n,
                                    out.ctypes.data, out[0][0].nbytes, out[0].nbytes, status.ctypes.data)
        if rc != DVC_OK and not status.any():
            check(rc)
        return [out[i].copy() if status[i] == 0 else None for i in range(n)]

    def decode(self, samples) -> list:
        """One frame per sample; ``None`` for a sample whose data is damaged."""
        frames, run = [], []
        for s in list(samples) + [None]:
            same = s is not None and self._hdr is not None and len(s) > len(self._hdr) and \
                s[:len(self._hdr)] == self._hdr
            if run and not same:
                frames += self._run(run)
                run = []
            if s is None:
                break
            if not same:
                try:
                    hl = self.set_header(s)
                except DvcError as e:
                    if e.code == DVC_E_UNSUPPORTED:
                        raise
                    frames.append(None)      # no header: a damaged sample
                    continue
                if len(s) <= hl:
                    frames.append(None)
                    continue
            run.append(s)
        return frames


# dvc_quality_frame (include/dvc.h) as a numpy record
QUALITY_FRAME = [("sse", "<u8", (4,)), ("ssim_q32", "<i8"), ("windows", "<u4"), ("pixels", "<u4")]
# dvc_quality_regions: sse[class][channel] (class 0 kept, 1 static), ssim_q32 / windows of the
# kept, static and mixed windows, pixels[class]
QUALITY_REGIONS = [("sse", "<u8", (2, 4)), ("ssim_q32", "<i8", (3,)), ("windows", "<u4", (3,)), ("pixels", "<u4", (2,)),
                   ("reserved", "<u4")]


class QualityMeter(Handle):
    """The quality meter on the GPU (dvc_quality): reference and test frames,
    (n, H, W, 3) BGR uint8 with n <= ``max_batch`` — any strides whose pixels are
    3 contiguous bytes and whose rows are >= 3 W bytes apart are read as they
    are, page-locked buffers (:func:`pinned`) without a staging copy — -> one
    ``QUALITY_FRAME`` record per pair: the exact integers DESIGN.md "Quality
    metrics" defines; :mod:`quality` derives PSNR and SSIM from them."""

    _destroy = "dvc_quality_destroy"

    def __init__(self, width: int, height: int, device: int = 0, max_batch: int = 8):
        self.W, self.H, self.max_batch = int(width), int(height), int(max_batch)
        self._create(lib().dvc_quality_create, self.W, self.H, self.max_batch, int(device), None, 0)

    def _rows(self, frames):
        """``frames`` as (array, pitch, frame stride) the C-ABI can read in place."""
        import numpy as np
        f = np.asarray(frames)
        if f.dtype != np.uint8 or f.ndim != 4 or f.shape[1:] != (self.H, self.W, 3):
            raise ValueError(f"frames {f.shape} {f.dtype} do not match (n, {self.H}, {self.W}, 3) uint8")
        n, fs, pitch = f.shape[0], f.strides[0], f.strides[1]
        if f.strides[2:] != (3, 1) or pitch < 3 * self.W or (n > 1 and fs < pitch * (self.H - 1) + 3 * self.W):
            f = np.ascontiguousarray(f)
            fs, pitch = f.strides[0], f.strides[1]
        return f, pitch, fs

    def compare(self, ref, test):
        import numpy as np
        a, ap, as_ = self._rows(ref)
        b, bp, bs = self._rows(test)
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"{a.shape[0]} reference frames against {b.shape[0]} test frames")
        out = np.zeros(a.shape[0], QUALITY_FRAME)
        check(lib().dvc_quality_compare(self._h, a.ctypes.data, ap, as_, b.ctypes.data, bp, bs, a.shape[0],
                                        out.ctypes.data))
        return out

    def compare_regions(self, ref, test, mask, block, partial_static):
        """:meth:`compare` split by ``mask``, (n, H, W) uint8 (rows >= W bytes apart are
        read in place): one ``QUALITY_REGIONS`` record per pair, the squared error of
        the kept and of the static pixels and the SSIM of the kept, static and mixed
        windows (DESIGN.md "Quality metrics": a block of ``block`` x ``block`` pixels is
        static iff its mask bytes are all 0; ``partial_static`` 1 applies that to the
        partial blocks on the right and bottom edges, as the FD worker does, 0 keeps
        them, as the OF compressor does). Any n: more than ``max_batch`` pairs go in
        several calls."""
        import numpy as np
        a, ap, as_ = self._rows(ref)
        b, bp, bs = self._rows(test)
        m = np.asarray(mask)
        n = a.shape[0]
        if m.dtype != np.uint8 or m.shape != (n, self.H, self.W) or b.shape[0] != n:
            raise ValueError(f"{n} reference frames, {b.shape[0]} test frames and masks {m.shape} {m.dtype}: "
                             f"(n, {self.H}, {self.W}) uint8 masks are needed")
        ms, mp = m.strides[0], m.strides[1]
        if m.strides[2] != 1 or mp < self.W or (n > 1 and ms < mp * (self.H - 1) + self.W):
            m = np.ascontiguousarray(m)
            ms, mp = m.strides[0], m.strides[1]
        out = np.zeros(n, QUALITY_REGIONS)
        for t in range(0, n, self.max_batch):
            k = min(self.max_batch, n - t)
            check(lib().dvc_quality_compare_regions(self._h, a[t:].ctypes.data, ap, as_, b[t:].ctypes.data, bp, bs,
                                                    m[t:].ctypes.data, mp, ms, int(block), int(partial_static), k,
                                                    out[t:].ctypes.data))
        return out


def copy_rate(device: int = 0, nbytes: int = 1 << 30, reps: int = 20, nontemporal: bool = True) -> float:
    """dvc_copy_rate: this GPU's hand-written streaming-copy rate in GB/s (bytes
    read + written), the practical HBM ceiling the bench quotes beside 8 TB/s."""
    g = ctypes.c_double()
    check(lib().dvc_copy_rate(int(device), int(nbytes), int(reps), int(bool(nontemporal)), ctypes.byref(g)))
    return g.value


def gaussian_taps_q8(n: int, sigma: float) -> list:
    t = (ctypes.c_uint16 * n)()
    check(lib().dvc_gaussian_taps_q8(n, sigma, t))
    return list(t)
