"""ctypes binding of libubresnet_det.so (the C ABI in include/ubresnet_det.h): detector effects on a prepared training batch.

A library of its own next to libubresnet_aug.so (ubresnet_amd/_aug.py) and the others, with its own error string.  As there, NO
fallback: a missing library or a failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the
library can be exercised on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UBX_LIB", os.path.join(HERE, "libubresnet_det.so"))

LANE_PIXELS = 4             # UBX_LANE_PIXELS
BLOCK = 256                 # UBX_BLOCK
MAX_GRID = 1024             # UBX_MAX_GRID
PHILOX_TAG = 0x55425844     # UBX_PHILOX_TAG

# every symbol include/ubresnet_det.h declares (tests check that all of them are exported)
SYMBOLS = ["ubx_apply", "ubx_last_error", "ubx_version"]

_lib = None
_lock = threading.Lock()
vp, u32, i64, f32 = C.c_void_p, C.c_uint32, C.c_int64, C.c_float


def _declare(lib):
    lib.ubx_last_error.restype = C.c_char_p
    lib.ubx_last_error.argtypes = []
    lib.ubx_version.restype = C.c_int
    lib.ubx_version.argtypes = []
    lib.ubx_apply.restype = C.c_int
    lib.ubx_apply.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, f32, C.c_int, u32, u32,
                              C.c_int, i64, C.c_int, f32, vp]


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
        msg = lib().ubx_last_error().decode("utf-8", "replace")
        raise RuntimeError("ubresnet_amd HIP call failed (%d) %s: %s" % (rc, what, msg))


def row_words(width: int) -> int:
    """words of one (image, plane) row of the table: the gain and ceil(W / 32) mask words"""
    return 1 + (int(width) + 31) // 32


def apply(image: int, label, weight, shape, table: int, sigma: float = 0.0, noise_all: bool = False, seed: int = 0, seq: int = 0,
          dead_label=None, dead_weight=None, stream=None):
    """ubx_apply on raw device addresses (ints; `label` / `weight` may be None where their dead value is None); `shape` =
    (B, P, H, W); `table` the device address of the uint32 [B, P, row_words(W)] table; dead_label / dead_weight None: keep"""
    b, p, h, w = (int(v) for v in shape)
    rc = lib().ubx_apply(image, label, weight, b, p, h, w, table, float(sigma), 1 if noise_all else 0, int(seed), int(seq),
                         0 if dead_label is None else 1, 0 if dead_label is None else int(dead_label),
                         0 if dead_weight is None else 1, 0.0 if dead_weight is None else float(dead_weight), stream)
    check(rc, "apply")
