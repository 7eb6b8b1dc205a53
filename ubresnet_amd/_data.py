"""ctypes binding of libubresnet_data.so (the C ABI in include/ubresnet_data.h): device-side batch preparation of the loader.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

LANE_PIXELS = 4      # UBD_LANE_PIXELS
BLOCK = 256          # UBD_BLOCK
MAX_GRID = 2048      # UBD_MAX_GRID

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
BINDING = Binding("UBD_LIB", "libubresnet_data.so", "ubd", {
    "ubd_prep_batch": (C.c_int, [vp, vp, i64, i32, vp, C.c_int, i64, C.c_int, f32, vp, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def prep_batch(label_wire: int, label: int, n: int, label_offset: int = 0, image=None, planes: int = 1, hw: int = 1,
               threshold=None, weight_fill=None, stream=None):
    """ubd_prep_batch on raw device addresses (ints or None); `threshold` None switches the ADC threshold off"""
    rc = lib().ubd_prep_batch(label_wire, label, n, label_offset, image if threshold is not None else None, planes, hw,
                              0 if threshold is None else 1, 0.0 if threshold is None else float(threshold), weight_fill, stream)
    check(rc, "prep_batch")
