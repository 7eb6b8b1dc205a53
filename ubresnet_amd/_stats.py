"""ctypes binding of libubresnet_stats.so (the C ABI in include/ubresnet_stats.h): the guard of the BatchNorm running statistics
on the device -- the scan of the live statistics for non-finite values, the decision between commit and restore, and the move of
every row of a table of small tensors in the decided direction.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import Binding

BLOCK = 256          # UBS_BLOCK
SEG_GRID = 256       # UBS_SEG_GRID
CTL_BYTES = 32       # UBS_CTL_BYTES
KIND_F32 = 0         # UBS_KIND_F32: fp32 values, scanned
KIND_RAW = 1         # UBS_KIND_RAW: raw 4-byte units, never scanned

# one row of the table as a numpy dtype (host copy of the device array)
SEG = np.dtype([("shadow", "<u8"), ("live", "<u8"), ("count", "<i8"), ("kind", "<i8")])
# the control block as a numpy dtype
CTL = np.dtype([("keep", "<i4"), ("bad_rows", "<i4"), ("kept", "<i8"), ("restored", "<i8"), ("restored_for_stats", "<i8")])


class Ctl(C.Structure):
    """struct ubs_ctl: the control block"""
    _fields_ = [("keep", C.c_int32), ("bad_rows", C.c_int32), ("kept", C.c_int64), ("restored", C.c_int64),
                ("restored_for_stats", C.c_int64)]


vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
BINDING = Binding("UBS_LIB", "libubresnet_stats.so", "ubs", {
    "ubs_ctl_init": (C.c_int, [vp, vp]),
    "ubs_scan": (C.c_int, [vp, i64, vp, vp]),
    "ubs_note": (C.c_int, [vp, vp, i64, vp]),
    "ubs_decide": (C.c_int, [vp, vp, i64, vp, i32, vp]),
    "ubs_resolve": (C.c_int, [vp, i64, vp, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def read_ctl(raw: bytes) -> Ctl:
    """a control block copied to the host (at least CTL_BYTES bytes) as a Ctl"""
    return Ctl.from_buffer_copy(bytes(raw[:CTL_BYTES]))


def seg_table(shadow, live, count, kind) -> np.ndarray:
    """the table as a numpy array of dtype SEG from four sequences (device addresses of the shadow and of the live tensor, number
    of 4-byte units, KIND_F32 / KIND_RAW)"""
    t = np.zeros(len(count), dtype=SEG)
    t["shadow"], t["live"], t["count"], t["kind"] = shadow, live, count, kind
    return t


def ctl_init(ctl: int, stream=None):
    check(lib().ubs_ctl_init(ctl, stream), "ctl_init")


def scan(table: int, nseg: int, bad: int, stream=None):
    check(lib().ubs_scan(table, int(nseg), bad, stream), "scan")


def note(seen: int, bad: int, nseg: int, stream=None):
    check(lib().ubs_note(seen, bad, int(nseg), stream), "note")


def decide(ctl: int, bad: int, nseg: int, apply_flag, check_nonfinite: bool, stream=None):
    """ubs_decide on raw device addresses; `apply_flag` None: the step counts as applied"""
    check(lib().ubs_decide(ctl, bad, int(nseg), apply_flag, 1 if check_nonfinite else 0, stream), "decide")


def resolve(table: int, nseg: int, ctl: int, stream=None):
    check(lib().ubs_resolve(table, int(nseg), ctl, stream), "resolve")
