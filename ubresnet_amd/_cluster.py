"""ctypes binding of libubresnet_cluster.so (the C ABI in include/ubresnet_cluster.h): connected components of event products on
the device -- the lit pixels of a class map grouped into clusters by union-find across tiles, the clusters numbered in ascending
root order and summarised in an integer table, and the cluster number of every entry of a pixel list.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch or numpy, so the argument checks of the library can be exercised on a
machine without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

TILE_H = 32              # UBI_TILE_H
TILE_W = 64              # UBI_TILE_W
LANES = 256              # UBI_LANES
BORDER_LANES = 128       # UBI_BORDER_LANES
PIXEL_BLOCK = 1024       # UBI_PIXEL_BLOCK: pixels of one workgroup of the pixel passes
SCAN_WIDTH = 1024        # UBI_SCAN_WIDTH: block counts of one trip of the one-workgroup scan
MAX_GRID = 4096          # UBI_MAX_GRID
MAX_CLASSES = 16         # UBI_MAX_CLASSES
TABLE_FIXED = 8          # UBI_TABLE_FIXED: root, pixels, row_min, row_max, col_min, col_max, conf_sum, nonfinite
MAX_PIXELS = 2 ** 31 - 1
COLUMNS = ("root", "pixels", "row_min", "row_max", "col_min", "col_max", "conf_sum", "nonfinite")

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
BINDING = Binding("UBI_LIB", "libubresnet_cluster.so", "ubi", {
    "ubi_scratch_bytes": (i64, [i32, i32, i32]),
    "ubi_label": (C.c_int, [vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, vp]),
    "ubi_tabulate": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, i64, vp, vp, i32, i32, i32, vp]),
    "ubi_gather_ids": (C.c_int, [vp, vp, vp, i64, vp, i64, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def scratch_bytes(P: int, rows: int, cols: int) -> int:
    """what ubi_tabulate needs as scratch for a [P][rows][cols] image; an image it refuses is a RuntimeError"""
    nbytes = lib().ubi_scratch_bytes(int(P), int(rows), int(cols))
    if nbytes <= 0:
        check(-1, "scratch_bytes")
    return nbytes


def label(label_: int, C_: int, fill_label: int, connectivity: int, by_class: bool, root: int, status: int, P: int, rows: int,
          cols: int, stream=None):
    """ubi_label on raw device addresses"""
    check(lib().ubi_label(label_, int(C_), int(fill_label), int(connectivity), int(bool(by_class)), root, status, int(P), int(rows),
                          int(cols), stream), "label")


def tabulate(label_: int, confidence: int, root: int, C_: int, fill_label: int, ids: int, table: int, capacity: int, count: int,
             scratch: int, P: int, rows: int, cols: int, stream=None):
    """ubi_tabulate on raw device addresses"""
    check(lib().ubi_tabulate(label_, confidence, root, int(C_), int(fill_label), ids, table, int(capacity), count, scratch, int(P),
                             int(rows), int(cols), stream), "tabulate")


def gather_ids(ids: int, index: int, list_count: int, list_capacity: int, out: int, pixels: int, stream=None):
    """ubi_gather_ids on raw device addresses"""
    check(lib().ubi_gather_ids(ids, index, list_count, int(list_capacity), out, int(pixels), stream), "gather_ids")
