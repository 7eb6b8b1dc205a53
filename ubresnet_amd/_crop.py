"""ctypes binding of libubresnet_crop.so (the C ABI in include/ubresnet_crop.h): training crops cut from a whole labelled view on
the device -- the summed-area table of the view's counting pixels per cell, seeded crop positions drawn against it, and the gather
of image, label and weight into the training batch.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch or numpy, so the argument checks of the library can be exercised on a
machine without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

LANES = 256                 # UBN_LANES
MIN_CELL, MAX_CELL = 4, 64  # UBN_MIN_CELL, UBN_MAX_CELL
MAX_CELL_COLS = 4096        # UBN_MAX_CELL_COLS
MAX_PLANES = 64             # UBN_MAX_PLANES
MAX_CROPS = 4096            # UBN_MAX_CROPS
MAX_TRIES = 64              # UBN_MAX_TRIES
TABLE_FIELDS = 8            # UBN_TABLE_FIELDS
PHILOX_TAG = 0x43524F50     # UBN_PHILOX_TAG
LABEL_NONE, LABEL_U8, LABEL_I64, LABEL_F32 = 0, 1, 2, 3
MAX_PIXELS = 2 ** 31 - 1
FIELDS = ("plane", "row0", "col0", "lit", "try", "accepted", "flip_rows", "flip_cols")

vp, i32, u32, f32, ci = C.c_void_p, C.c_int32, C.c_uint32, C.c_float, C.c_int
BINDING = Binding("UBN_LIB", "libubresnet_crop.so", "ubn", {
    "ubn_occupancy": (ci, [vp, vp, ci, i32, u32, ci, f32, ci, ci, ci, ci, vp, vp]),
    "ubn_choose": (ci, [vp, ci, ci, ci, ci, ci, ci, C.POINTER(i32), ci, ci, ci, i32, u32, u32, u32, ci, ci, vp, vp]),
    "ubn_gather": (ci, [vp, vp, ci, i32, vp, ci, ci, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def largest_cell(rows: int, cols: int, H: int, W: int) -> int:
    """the largest power of two in MIN_CELL..MAX_CELL that divides H, W, rows - H and cols - W; 0 where there is none"""
    g = MAX_CELL
    while g >= MIN_CELL:
        if H % g == 0 and W % g == 0 and (rows - H) % g == 0 and (cols - W) % g == 0:
            return g
        g //= 2
    return 0


def sat_shape(Q: int, rows: int, cols: int, cell: int):
    return (Q, rows // cell + 1, cols // cell + 1)


def occupancy(image: int, label, label_kind: int, label_offset: int, class_mask: int, stacked: bool, adc_threshold: float, P: int,
              rows: int, cols: int, cell: int, sat: int, stream=None):
    """ubn_occupancy on raw device addresses; `label` an address, or None with LABEL_NONE (no class mask)"""
    check(lib().ubn_occupancy(image, label, int(label_kind), int(label_offset), int(class_mask), 1 if stacked else 0, float(adc_threshold),
                              int(P), int(rows), int(cols), int(cell), sat, stream), "occupancy")


def choose(sat: int, Q: int, rows: int, cols: int, H: int, W: int, cell: int, planes, K: int, T: int, min_lit: int, seed: int,
           number: int, flip_rows: bool, flip_cols: bool, table: int, stream=None):
    """ubn_choose: `sat` and `table` raw device addresses, `planes` a sequence of ints on the host or None (all Q); `seed` a 64-bit
    and `number` a 32-bit unsigned int"""
    arr, n = None, 0
    if planes is not None:
        n = len(planes)
        arr = (i32 * max(n, 1))(*[int(p) for p in planes])
    seed = int(seed)
    check(lib().ubn_choose(sat, int(Q), int(rows), int(cols), int(H), int(W), int(cell), arr, n, int(K), int(T), int(min_lit),
                           seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, int(number), 1 if flip_rows else 0, 1 if flip_cols else 0, table,
                           stream), "choose")


def gather(image: int, label: int, label_kind: int, label_offset: int, weight, stacked: bool, P: int, rows: int, cols: int, H: int,
           W: int, table: int, K: int, out_image: int, out_label: int, out_weight: int, status: int, stream=None):
    """ubn_gather on raw device addresses; `weight` an address or None (every weight 1.0)"""
    check(lib().ubn_gather(image, label, int(label_kind), int(label_offset), weight, 1 if stacked else 0, int(P), int(rows), int(cols),
                           int(H), int(W), table, int(K), out_image, out_label, out_weight, status, stream), "gather")
