"""ctypes binding of libubresnet_post.so (the C ABI in include/ubresnet_post.h): event products of whole-view inference.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

MAX_TILES = 64       # UBP_MAX_TILES
MAX_CLASSES = 16     # UBP_MAX_CLASSES

vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
BINDING = Binding("UBP_LIB", "libubresnet_post.so", "ubp", {
    "ubp_stitch_products": (C.c_int, [vp, i32, i32, i32, C.POINTER(C.c_int32), i32, vp, i32, f32, vp, vp, vp, i32, i32, i32, i32, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check
