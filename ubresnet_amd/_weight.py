"""ctypes binding of libubresnet_weight.so (the C ABI in include/ubresnet_weight.h): pixel weights of the loss made on the
device -- per-image class balance and an interface gain.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

MAX_CLASSES = 16     # UBW_MAX_CLASSES
MAX_RADIUS = 4       # UBW_MAX_RADIUS
# launch geometry of ubresnet_amd/csrc/ubr_weight_tile.h (not part of the C ABI; tests hold these against that file)
LANE_PIXELS = 4      # UBW_LANE_PIXELS
BLOCK = 256          # UBW_BLOCK
MAX_GRID = 2048      # UBW_MAX_GRID
TILE_W = 64          # UBW_TILE_W
TILE_H = 16          # UBW_TILE_H

vp, f32 = C.c_void_p, C.c_float
BINDING = Binding("UBW_LIB", "libubresnet_weight.so", "ubw", {
    "ubw_pixel_weights": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32, C.c_int, f32, C.c_int, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def pixel_weights(label: int, weight: int, counts: int, shape, num_classes: int, max_weight: float, radius: int, gain: float,
                  lo: int, stream=None):
    """ubw_pixel_weights on raw device addresses; `shape` is (B, H, W)"""
    b, h, w = (int(v) for v in shape)
    check(lib().ubw_pixel_weights(label, weight, counts, b, h, w, int(num_classes), float(max_weight), int(radius), float(gain),
                                  int(lo), stream), "pixel_weights")
