"""ctypes binding of libubresnet_overlap.so (the C ABI in include/ubresnet_overlap.h): two clusterings of an event matched on the
device -- the contingency table of two id maps over the same pixels, one row per pair of cluster numbers with its first pixel,
pixel count and charge, through a hash table in scratch whose read-out is numbered by first pixel.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch or numpy, so the argument checks of the library can be exercised on a
machine without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

LANES = 256                    # UBH_LANES
TRIP_PIXELS = 2048             # UBH_TRIP_PIXELS: pixels of one trip of a workgroup
MAX_GRID = 1024                # UBH_MAX_GRID
LDS_SLOTS = 64                 # UBH_LDS_SLOTS: pairs of the LDS table of a workgroup
COLUMNS = 6                    # UBH_COLUMNS
SLOT_WORDS = 5                 # UBH_SLOT_WORDS: uint64 words of a slot in scratch
MAX_PROBES = 128               # UBH_MAX_PROBES: UBH_PROBES = min(slots, 128)
MIN_SLOTS = 64                 # UBH_MIN_SLOTS
MAX_SLOTS = 1073741824         # UBH_MAX_SLOTS: 2^30
MAX_WEIGHT = 65535             # UBH_MAX_WEIGHT
MAX_SCALE = 256                # UBH_MAX_SCALE
MAX_PIXELS = 2 ** 31 - 1
COLUMN_NAMES = ("a", "b", "first", "pixels", "weighted", "Q")

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
BINDING = Binding("UBH_LIB", "libubresnet_overlap.so", "ubh", {
    "ubh_default_slots": (i64, [i64]),
    "ubh_scratch_bytes": (i64, [i32, i32, i32, i64]),
    "ubh_overlap": (C.c_int, [vp, vp, vp, C.c_float, vp, i64, vp, vp, vp, i64, i32, i32, i32, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def default_slots(capacity: int) -> int:
    """ubh_default_slots: the smallest power of two >= 2 * capacity and at least 1024"""
    n = lib().ubh_default_slots(int(capacity))
    if n <= 0:
        raise RuntimeError("ubresnet_amd: ubh_default_slots refused capacity=%r" % (capacity,))
    return n


def scratch_bytes(P: int, rows: int, cols: int, slots: int) -> int:
    """ubh_scratch_bytes"""
    n = lib().ubh_scratch_bytes(int(P), int(rows), int(cols), int(slots))
    if n <= 0:
        raise RuntimeError("ubresnet_amd: ubh_scratch_bytes refused P=%r, rows=%r, cols=%r, slots=%r" % (P, rows, cols, slots))
    return n


def overlap(ids_a: int, ids_b: int, view, adc_scale: float, table: int, capacity: int, count: int, status: int, scratch: int,
            slots: int, P: int, rows: int, cols: int, stream=None):
    """ubh_overlap on raw device addresses; view None for no charge"""
    check(lib().ubh_overlap(ids_a, ids_b, view, float(adc_scale), table, int(capacity), count, status, scratch, int(slots), int(P),
                            int(rows), int(cols), stream), "overlap")
