"""ctypes binding of libubresnet_ema.so (the C ABI in include/ubresnet_ema.h): the exponential moving average of the parameters
on the device -- the decision about an update, the streaming update and the in-place exchange over flat buffers, and the same
two operations over a table of small tensors.

A library of its own next to the other seven (ubresnet_amd/_lib.py, _post.py, _data.py, _aug.py, _opt.py, _weight.py,
_group.py), with its own error string.  As there, NO fallback: a missing library or a failed call is a RuntimeError.  Nothing
here imports torch, so the argument checks of the library can be exercised on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UBE_LIB", os.path.join(HERE, "libubresnet_ema.so"))

BLOCK = 256          # UBE_BLOCK
UNROLL = 4           # UBE_UNROLL
MAX_GRID = 1024      # UBE_MAX_GRID
SEG_GRID = 256       # UBE_SEG_GRID
CTL_BYTES = 32       # UBE_CTL_BYTES
APPLY_OFFSET = 20    # byte offset of `apply` in ubo_ctl and in ubg_ctl: what ube_advance takes as apply_flag

# every symbol include/ubresnet_ema.h declares (tests check that all of them are exported)
SYMBOLS = ["ube_ctl_init", "ube_advance", "ube_update", "ube_swap", "ube_update_segs", "ube_swap_segs", "ube_last_error", "ube_version"]

# one row of the table of ube_update_segs / ube_swap_segs as a numpy dtype (host copy of the device array)
SEG = np.dtype([("shadow", "<u8"), ("live", "<u8"), ("count", "<i8"), ("reserved", "<i8")])


class Ctl(C.Structure):
    """struct ube_ctl: the control block"""
    _fields_ = [("apply", C.c_int32), ("w", C.c_float), ("d", C.c_float), ("reserved", C.c_int32), ("updates", C.c_int64),
                ("held", C.c_int64)]


_lib = None
_lock = threading.Lock()
vp, i64, f32 = C.c_void_p, C.c_int64, C.c_float


def _declare(lib):
    lib.ube_last_error.restype = C.c_char_p
    lib.ube_last_error.argtypes = []
    lib.ube_version.restype = C.c_int
    lib.ube_version.argtypes = []
    lib.ube_ctl_init.restype = C.c_int
    lib.ube_ctl_init.argtypes = [vp, i64, vp]
    lib.ube_advance.restype = C.c_int
    lib.ube_advance.argtypes = [vp, vp, f32, i64, vp]
    lib.ube_update.restype = C.c_int
    lib.ube_update.argtypes = [vp, vp, i64, vp, vp]
    lib.ube_swap.restype = C.c_int
    lib.ube_swap.argtypes = [vp, vp, i64, vp]
    lib.ube_update_segs.restype = C.c_int
    lib.ube_update_segs.argtypes = [vp, i64, vp, vp]
    lib.ube_swap_segs.restype = C.c_int
    lib.ube_swap_segs.argtypes = [vp, i64, vp]


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
        msg = lib().ube_last_error().decode("utf-8", "replace")
        raise RuntimeError("ubresnet_amd HIP call failed (%d) %s: %s" % (rc, what, msg))


def read_ctl(raw: bytes) -> Ctl:
    """a control block copied to the host (at least CTL_BYTES bytes) as a Ctl"""
    return Ctl.from_buffer_copy(bytes(raw[:CTL_BYTES]))


def seg_table(shadow, live, count) -> np.ndarray:
    """the table of ube_update_segs / ube_swap_segs as a numpy array of dtype SEG from three sequences (device addresses of the
    averaged and of the live tensor, number of fp32 values)"""
    t = np.zeros(len(count), dtype=SEG)
    t["shadow"], t["live"], t["count"] = shadow, live, count
    return t


def ctl_init(ctl: int, updates: int = 0, stream=None):
    check(lib().ube_ctl_init(ctl, int(updates), stream), "ctl_init")


def advance(ctl: int, apply_flag, decay: float, warmup: int, stream=None):
    """ube_advance on raw device addresses; `apply_flag` None: the update is applied whatever happened"""
    check(lib().ube_advance(ctl, apply_flag, float(decay), int(warmup), stream), "advance")


def update(shadow: int, param: int, n: int, ctl: int, stream=None):
    check(lib().ube_update(shadow, param, int(n), ctl, stream), "update")


def swap(a: int, b: int, n: int, stream=None):
    check(lib().ube_swap(a, b, int(n), stream), "swap")


def update_segs(table: int, nseg: int, ctl: int, stream=None):
    check(lib().ube_update_segs(table, int(nseg), ctl, stream), "update_segs")


def swap_segs(table: int, nseg: int, stream=None):
    check(lib().ube_swap_segs(table, int(nseg), stream), "swap_segs")
