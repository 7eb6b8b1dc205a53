"""ctypes binding of libubresnet_sparse.so (the C ABI in include/ubresnet_sparse.h): sparse event I/O of whole-view inference on
the device -- a sorted (pixel index, value) list scattered into a dense view, dense event products compacted into the list of
their lit pixels in ascending index order, and that list expanded back into products.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch or numpy, so the argument checks of the library can be exercised on a
machine without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

LANES = 256              # UBZ_LANES
LANE_PIXELS = 4          # UBZ_LANE_PIXELS
PIXEL_BLOCK = 1024       # UBZ_PIXEL_BLOCK: pixels of one workgroup of the count and write passes
SCAN_WIDTH = 1024        # UBZ_SCAN_WIDTH: block counts of one trip of the one-workgroup scan
MAX_GRID = 4096          # UBZ_MAX_GRID
MAX_VPLANES = 64         # UBZ_MAX_VPLANES
MAX_PIXELS = 2 ** 31 - 1

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
BINDING = Binding("UBZ_LIB", "libubresnet_sparse.so", "ubz", {
    "ubz_scatter_view": (C.c_int, [vp, vp, i64, vp, vp, i32, i32, i32, vp, vp]),
    "ubz_compact_scratch_bytes": (i64, [i32, i32, i32]),
    "ubz_compact": (C.c_int, [vp, vp, vp, i32, f32, i32, i32, i32, i64, vp, vp, vp, vp, vp, i64, vp]),
    "ubz_expand": (C.c_int, [vp, vp, vp, i64, vp, i32, vp, vp, i32, i32, i32, vp, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def scatter_view(index: int, value: int, n: int, count, view: int, P: int, rows: int, cols: int, status: int, stream=None):
    """ubz_scatter_view on raw device addresses; `count` an address or None"""
    check(lib().ubz_scatter_view(index, value, int(n), count, view, int(P), int(rows), int(cols), status, stream), "scatter_view")


def compact_scratch_bytes(P: int, rows: int, cols: int) -> int:
    """what ubz_compact needs as scratch for a [P][rows][cols] image; an image it refuses is a RuntimeError"""
    nbytes = lib().ubz_compact_scratch_bytes(int(P), int(rows), int(cols))
    if nbytes <= 0:
        check(-1, "compact_scratch_bytes")
    return nbytes


def compact(label: int, confidence: int, adc, vplanes: int, adc_threshold: float, P: int, rows: int, cols: int, capacity: int,
            out_index: int, out_label: int, out_confidence: int, count: int, scratch: int, scratch_bytes: int, stream=None):
    """ubz_compact on raw device addresses; `adc` an address or None (every pixel lit)"""
    check(lib().ubz_compact(label, confidence, adc, int(vplanes), float(adc_threshold), int(P), int(rows), int(cols), int(capacity),
                            out_index, out_label, out_confidence, count, scratch, int(scratch_bytes), stream), "compact")


def expand(index: int, label: int, confidence: int, n: int, count, fill_label: int, out_label: int, out_confidence: int, P: int,
           rows: int, cols: int, status: int, stream=None):
    """ubz_expand on raw device addresses; `count` an address or None"""
    check(lib().ubz_expand(index, label, confidence, int(n), count, int(fill_label), out_label, out_confidence, int(P), int(rows),
                           int(cols), status, stream), "expand")
