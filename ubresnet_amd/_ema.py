"""ctypes binding of libubresnet_ema.so (the C ABI in include/ubresnet_ema.h): the exponential moving average of the parameters
on the device -- the decision about an update, the streaming update and the in-place exchange over flat buffers, and the same
two operations over a table of small tensors.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import Binding

BLOCK = 256          # UBE_BLOCK
UNROLL = 4           # UBE_UNROLL
MAX_GRID = 1024      # UBE_MAX_GRID
SEG_GRID = 256       # UBE_SEG_GRID
CTL_BYTES = 32       # UBE_CTL_BYTES
APPLY_OFFSET = 20    # byte offset of `apply` in ubo_ctl and in ubg_ctl: what ube_advance takes as apply_flag

# one row of the table of ube_update_segs / ube_swap_segs as a numpy dtype (host copy of the device array)
SEG = np.dtype([("shadow", "<u8"), ("live", "<u8"), ("count", "<i8"), ("reserved", "<i8")])


class Ctl(C.Structure):
    """struct ube_ctl: the control block"""
    _fields_ = [("apply", C.c_int32), ("w", C.c_float), ("d", C.c_float), ("reserved", C.c_int32), ("updates", C.c_int64),
                ("held", C.c_int64)]


vp, i64, f32 = C.c_void_p, C.c_int64, C.c_float
BINDING = Binding("UBE_LIB", "libubresnet_ema.so", "ube", {
    "ube_ctl_init": (C.c_int, [vp, i64, vp]),
    "ube_advance": (C.c_int, [vp, vp, f32, i64, vp]),
    "ube_update": (C.c_int, [vp, vp, i64, vp, vp]),
    "ube_swap": (C.c_int, [vp, vp, i64, vp]),
    "ube_update_segs": (C.c_int, [vp, i64, vp, vp]),
    "ube_swap_segs": (C.c_int, [vp, i64, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


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
