"""ctypes binding of libubresnet_loss.so (the C ABI in include/ubresnet_loss.h): the pixel-wise focal loss and its normalised
means on the device -- a streaming pass that leaves one row of partials per workgroup, one workgroup that adds them in a fixed
order into a control block, and the backward that reads the reciprocal of the denominator from that block.

A library of its own next to the other ten (ubresnet_amd/_lib.py, _post.py, _data.py, _aug.py, _opt.py, _weight.py, _group.py,
_ema.py, _accum.py, _stats.py), with its own error string.  As there, NO fallback: a missing library or a failed call is a
RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UBL_LIB", os.path.join(HERE, "libubresnet_loss.so"))

BLOCK = 256          # UBL_BLOCK
UNROLL = 2           # UBL_UNROLL
MAX_GRID = 1024      # UBL_MAX_GRID
MAX_CLASSES = 16     # UBL_MAX_CLASSES
TRIP_PIXELS = BLOCK * UNROLL * 4
ROW_WORDS = 36       # UBL_ROW_WORDS
WORKSPACE_BYTES = MAX_GRID * ROW_WORDS * 8
CTL_WORDS = 40       # UBL_CTL_WORDS
CTL_BYTES = CTL_WORDS * 8
MEAN_PIXELS, MEAN_VALID, MEAN_WEIGHTS = 0, 1, 2
MODES = {"pixels": MEAN_PIXELS, "valid": MEAN_VALID, "weights": MEAN_WEIGHTS}
# the words of the control block (UBL_CTL_*)
CTL = dict(LOSS_SUM=0, WEIGHT_SUM=1, VALID=2, BAD=3, DENOM=4, INV_DENOM=5, LOSS=6, MODE=7, CLASS_LOSS=8, CLASS_PIXELS=24)
# the words of a workspace row (UBL_ROW_*)
ROW = dict(LOSS_SUM=0, WEIGHT_SUM=1, VALID=2, BAD=3, CLASS_LOSS=4, CLASS_PIXELS=20)

# every symbol include/ubresnet_loss.h declares (tests check that all of them are exported)
SYMBOLS = ["ubl_focal_fwd", "ubl_focal_bwd", "ubl_last_error", "ubl_version"]

_lib = None
_lock = threading.Lock()
vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float


def _declare(lib):
    lib.ubl_last_error.restype = C.c_char_p
    lib.ubl_last_error.argtypes = []
    lib.ubl_version.restype = C.c_int
    lib.ubl_version.argtypes = []
    lib.ubl_focal_fwd.restype = C.c_int
    lib.ubl_focal_fwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i64, f32, i32, vp, vp, vp, vp]
    lib.ubl_focal_bwd.restype = C.c_int
    lib.ubl_focal_bwd.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i64, f32, vp, vp]


def lib():
    """Load (once) and return the library; raises RuntimeError if it is not built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        "ubresnet_amd: HIP extension %s is missing; build it with "
                        "`python -m ubresnet_amd.build` (hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
                try:
                    l = C.CDLL(LIB_PATH)
                except OSError as e:
                    raise RuntimeError("ubresnet_amd: cannot load %s: %s" % (LIB_PATH, e))
                _declare(l)
                _lib = l
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().ubl_last_error().decode("utf-8", "replace")
        raise RuntimeError("ubresnet_amd HIP call failed (%d) %s: %s" % (rc, what, msg))


def grid(pixels: int) -> int:
    """workgroups (= workspace rows) of the streaming passes over `pixels` = N*H*W"""
    return min((int(pixels) + TRIP_PIXELS - 1) // TRIP_PIXELS, MAX_GRID)


def focal_fwd(predict: int, target: int, pixelweights: int, classw, N, Cn, H, W, ignore_index, gamma, mode, workspace: int,
              ctl: int, loss: int, stream=None):
    """ubl_focal_fwd on raw device addresses (classw: an address or None)"""
    check(lib().ubl_focal_fwd(predict, target, pixelweights, classw, int(N), int(Cn), int(H), int(W), int(ignore_index), float(gamma),
                              int(mode), workspace, ctl, loss, stream), "focal_fwd")


def focal_bwd(g_loss: int, ctl: int, predict: int, target: int, pixelweights: int, classw, N, Cn, H, W, ignore_index, gamma,
              g_predict: int, stream=None):
    """ubl_focal_bwd on raw device addresses"""
    check(lib().ubl_focal_bwd(g_loss, ctl, predict, target, pixelweights, classw, int(N), int(Cn), int(H), int(W), int(ignore_index),
                              float(gamma), g_predict, stream), "focal_bwd")


def read_ctl(raw: bytes) -> dict:
    """the control block (CTL_BYTES bytes, as copied to the host) as a dict of Python numbers and lists"""
    assert len(raw) >= CTL_BYTES
    f64 = struct.unpack_from("<%dd" % CTL_WORDS, raw)
    u64 = struct.unpack_from("<%dQ" % CTL_WORDS, raw)
    f32w = struct.unpack_from("<%df" % (2 * CTL_WORDS), raw)
    return dict(loss_sum=f64[CTL["LOSS_SUM"]], weight_sum=f64[CTL["WEIGHT_SUM"]], valid=u64[CTL["VALID"]], bad=u64[CTL["BAD"]],
                denom=f64[CTL["DENOM"]], inv_denom=f32w[2 * CTL["INV_DENOM"]], loss=f32w[2 * CTL["LOSS"]], mode=u64[CTL["MODE"]],
                class_loss=list(f64[CTL["CLASS_LOSS"]:CTL["CLASS_LOSS"] + MAX_CLASSES]),
                class_pixels=list(u64[CTL["CLASS_PIXELS"]:CTL["CLASS_PIXELS"] + MAX_CLASSES]))
