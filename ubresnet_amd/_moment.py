"""ctypes binding of libubresnet_moment.so (the C ABI in include/ubresnet_moment.h): per-cluster charge and shape on the device --
the ADC of every cluster of an event summed into an integer table of charge, charge per class and first and second moments, the
lanes of a wave and then the waves of a workgroup combined before anything goes to memory.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch or numpy, so the argument checks of the library can be exercised on a
machine without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

LANES = 256                    # UBM_LANES
TRIP_PIXELS = 2048             # UBM_TRIP_PIXELS: pixels of one trip of a workgroup
MAX_GRID = 1024                # UBM_MAX_GRID
SLOTS = 64                     # UBM_SLOTS: clusters of the LDS table of a workgroup
MAX_CLASSES = 16               # UBM_MAX_CLASSES
TABLE_FIXED = 9                # UBM_TABLE_FIXED
MAX_ROWS = 4096                # UBM_MAX_ROWS
MAX_COLS = 4096                # UBM_MAX_COLS
MAX_PLANE_PIXELS = 4194304     # UBM_MAX_PLANE_PIXELS: 2^22
MAX_WEIGHT = 65535             # UBM_MAX_WEIGHT
MAX_SCALE = 256                # UBM_MAX_SCALE
MAX_PIXELS = 2 ** 31 - 1
COLUMNS = ("weighted", "clipped", "odd", "Q", "Qr", "Qc", "Qrr", "Qrc", "Qcc")

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
BINDING = Binding("UBM_LIB", "libubresnet_moment.so", "ubm", {
    "ubm_moments": (C.c_int, [vp, vp, vp, i32, C.c_float, vp, i64, vp, i32, i32, i32, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def moments(ids: int, label: int, view: int, C_: int, adc_scale: float, table: int, capacity: int, count: int, P: int, rows: int,
            cols: int, stream=None):
    """ubm_moments on raw device addresses"""
    check(lib().ubm_moments(ids, label, view, int(C_), float(adc_scale), table, int(capacity), count, int(P), int(rows), int(cols),
                            stream), "moments")
