"""ctypes binding of libubresnet_post.so (the C ABI in include/ubresnet_post.h): event products of whole-view inference.

A library of its own next to libubresnet_hip.so (ubresnet_amd/_lib.py), with its own error string.  As there, NO fallback:
a missing library or a failed call is a RuntimeError.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UBP_LIB", os.path.join(HERE, "libubresnet_post.so"))

MAX_TILES = 64       # UBP_MAX_TILES
MAX_CLASSES = 16     # UBP_MAX_CLASSES

# every symbol include/ubresnet_post.h declares (tests check that all of them are exported)
SYMBOLS = ["ubp_stitch_products", "ubp_last_error", "ubp_version"]

_lib = None
_lock = threading.Lock()
vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float


def _declare(lib):
    lib.ubp_last_error.restype = C.c_char_p
    lib.ubp_last_error.argtypes = []
    lib.ubp_version.restype = C.c_int
    lib.ubp_version.argtypes = []
    lib.ubp_stitch_products.restype = C.c_int
    lib.ubp_stitch_products.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_int32), i32, vp, i32, f32, vp, vp, vp, i32, i32, i32, i32, vp]


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
        msg = lib().ubp_last_error().decode("utf-8", "replace")
        raise RuntimeError("ubresnet_amd HIP call failed (%d) %s: %s" % (rc, what, msg))
