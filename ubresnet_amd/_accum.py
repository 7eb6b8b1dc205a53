"""ctypes binding of libubresnet_accum.so (the C ABI in include/ubresnet_accum.h): gradient accumulation over the flat gradient
buffer on the device -- copy the first micro-batch into the accumulator, add the ones in between, write the scaled sum back into
the flat gradient buffer with the last.

A library of its own next to the other eight (ubresnet_amd/_lib.py, _post.py, _data.py, _aug.py, _opt.py, _weight.py, _group.py,
_ema.py), with its own error string.  As there, NO fallback: a missing library or a failed call is a RuntimeError.  Nothing here
imports torch, so the argument checks of the library can be exercised on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UBC_LIB", os.path.join(HERE, "libubresnet_accum.so"))

BLOCK = 256          # UBC_BLOCK
UNROLL = 4           # UBC_UNROLL
MAX_GRID = 1024      # UBC_MAX_GRID

# every symbol include/ubresnet_accum.h declares (tests check that all of them are exported)
SYMBOLS = ["ubc_set", "ubc_add", "ubc_finish", "ubc_last_error", "ubc_version"]

_lib = None
_lock = threading.Lock()
vp, i64, f32 = C.c_void_p, C.c_int64, C.c_float


def _declare(lib):
    lib.ubc_last_error.restype = C.c_char_p
    lib.ubc_last_error.argtypes = []
    lib.ubc_version.restype = C.c_int
    lib.ubc_version.argtypes = []
    lib.ubc_set.restype = C.c_int
    lib.ubc_set.argtypes = [vp, vp, i64, vp]
    lib.ubc_add.restype = C.c_int
    lib.ubc_add.argtypes = [vp, vp, i64, vp]
    lib.ubc_finish.restype = C.c_int
    lib.ubc_finish.argtypes = [vp, vp, i64, f32, vp]


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
        msg = lib().ubc_last_error().decode("utf-8", "replace")
        raise RuntimeError("ubresnet_amd HIP call failed (%d) %s: %s" % (rc, what, msg))


def set_(acc: int, grad: int, n: int, stream=None):
    """ubc_set on raw device addresses: acc = grad, bit for bit"""
    check(lib().ubc_set(acc, grad, int(n), stream), "set")


def add(acc: int, grad: int, n: int, stream=None):
    """ubc_add: acc += grad"""
    check(lib().ubc_add(acc, grad, int(n), stream), "add")


def finish(grad: int, acc: int, n: int, scale: float, stream=None):
    """ubc_finish: grad = (acc + grad) * scale; acc is left as it is"""
    check(lib().ubc_finish(grad, acc, int(n), float(scale), stream), "finish")
