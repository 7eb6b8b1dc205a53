"""ctypes binding of libubresnet_match.so (the C ABI in include/ubresnet_match.h): clusters of different wire planes matched by
their time profiles on the device -- the charge of every large cluster per time bin, and for every pair of them from two planes the
shared bins, the overlap of the two profiles and each side's charge inside the shared bins.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch or numpy, so the argument checks of the library can be exercised on a
machine without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

LANES = 256                    # UBU_LANES
TRIP_PIXELS = 2048             # UBU_TRIP_PIXELS: pixels of one trip of a workgroup of the profile launch
MAX_GRID = 1024                # UBU_MAX_GRID
TILE = 64                      # UBU_TILE: candidates of one side of a tile of pairs
CHUNK_BINS = 64                # UBU_CHUNK_BINS: time bins of one staged chunk
MIN_PLANES = 2                 # UBU_MIN_PLANES
MAX_PLANES = 4                 # UBU_MAX_PLANES
MIN_SLOTS = 64                 # UBU_MIN_SLOTS
MAX_SLOTS = 4096               # UBU_MAX_SLOTS
MAX_TIME_BIN = 64              # UBU_MAX_TIME_BIN
MAX_SHIFT = 4096               # UBU_MAX_SHIFT
MAX_ROWS = 4096                # UBU_MAX_ROWS
MAX_COLS = 4096                # UBU_MAX_COLS
MAX_PLANE_PIXELS = 4194304     # UBU_MAX_PLANE_PIXELS: 2^22
MAX_BIN_PIXELS = 65536         # UBU_MAX_BIN_PIXELS: time_bin * cols
MAX_CLASSES = 16               # UBU_MAX_CLASSES
CLUSTER_FIXED = 8              # UBU_CLUSTER_FIXED
CAND_COLUMNS = 6               # UBU_CAND_COLUMNS
PAIR_COLUMNS = 4               # UBU_PAIR_COLUMNS
MAX_WEIGHT = 65535             # UBU_MAX_WEIGHT
MAX_SCALE = 256                # UBU_MAX_SCALE
CAND_NAMES = ("cluster", "plane", "Q", "bins", "t_min", "t_max")
PAIR_NAMES = ("both", "I", "Qi_in", "Qj_in")

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
BINDING = Binding("UBU_LIB", "libubresnet_match.so", "ubu", {
    "ubu_scratch_bytes": (i64, [i32, i32, i32, i32, i64, i64]),
    "ubu_match": (C.c_int, [vp, vp, i32, vp, i64, vp, C.c_float, i32, i32, i32, i64, i32, C.POINTER(C.c_int), i64, vp, vp, vp, vp, vp, vp, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def time_bins(rows: int, time_bin: int) -> int:
    """T = ceil(rows / time_bin)"""
    return -(-int(rows) // int(time_bin))


def scratch_bytes(P: int, rows: int, cols: int, time_bin: int, slots: int, capacity: int) -> int:
    """ubu_scratch_bytes"""
    n = lib().ubu_scratch_bytes(int(P), int(rows), int(cols), int(time_bin), int(slots), int(capacity))
    if n <= 0:
        raise RuntimeError("ubresnet_amd: ubu_scratch_bytes refused P=%r, rows=%r, cols=%r, time_bin=%r, slots=%r, capacity=%r: %s"
                           % (P, rows, cols, time_bin, slots, capacity, lib().ubu_last_error().decode("utf-8", "replace")))
    return n


def shifts(row_shift):
    """the host array of row_shift, or None for None (the library refuses a null pointer)"""
    return None if row_shift is None else (C.c_int * len(row_shift))(*[int(s) for s in row_shift])


def match(ids: int, clusters: int, cluster_width: int, count: int, capacity: int, view: int, adc_scale: float, P: int, rows: int, cols: int,
          min_pixels: int, time_bin: int, row_shift, slots: int, profile: int, candidates: int, pairs: int, ncand: int, status: int,
          scratch: int, stream=None):
    """ubu_match on raw device addresses; row_shift a sequence of P ints on the host"""
    check(lib().ubu_match(ids, clusters, int(cluster_width), count, int(capacity), view, float(adc_scale), int(P), int(rows), int(cols),
                          int(min_pixels), int(time_bin), shifts(row_shift), int(slots), profile, candidates, pairs, ncand, status, scratch,
                          stream), "match")
