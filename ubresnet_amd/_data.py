"""ctypes binding of libubresnet_data.so (the C ABI in include/ubresnet_data.h): device-side batch preparation of the loader.

A library of its own next to libubresnet_hip.so (ubresnet_amd/_lib.py) and libubresnet_post.so (ubresnet_amd/_post.py), with
its own error string.  As there, NO fallback: a missing library or a failed call is a RuntimeError.  Nothing here imports torch,
so the argument checks of the library can be exercised on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UBD_LIB", os.path.join(HERE, "libubresnet_data.so"))

LANE_PIXELS = 4      # UBD_LANE_PIXELS
BLOCK = 256          # UBD_BLOCK
MAX_GRID = 2048      # UBD_MAX_GRID

# every symbol include/ubresnet_data.h declares (tests check that all of them are exported)
SYMBOLS = ["ubd_prep_batch", "ubd_last_error", "ubd_version"]

_lib = None
_lock = threading.Lock()
vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


def _declare(lib):
    lib.ubd_last_error.restype = C.c_char_p
    lib.ubd_last_error.argtypes = []
    lib.ubd_version.restype = C.c_int
    lib.ubd_version.argtypes = []
    lib.ubd_prep_batch.restype = C.c_int
    lib.ubd_prep_batch.argtypes = [vp, vp, i64, i32, vp, C.c_int, i64, C.c_int, f32, vp, vp]


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
        msg = lib().ubd_last_error().decode("utf-8", "replace")
        raise RuntimeError("ubresnet_amd HIP call failed (%d) %s: %s" % (rc, what, msg))


def prep_batch(label_wire: int, label: int, n: int, label_offset: int = 0, image=None, planes: int = 1, hw: int = 1,
               threshold=None, weight_fill=None, stream=None):
    """ubd_prep_batch on raw device addresses (ints or None); `threshold` None switches the ADC threshold off"""
    rc = lib().ubd_prep_batch(label_wire, label, n, label_offset, image if threshold is not None else None, planes, hw,
                              0 if threshold is None else 1, 0.0 if threshold is None else float(threshold), weight_fill, stream)
    check(rc, "prep_batch")
