"""ctypes binding of libubresnet_det.so (the C ABI in include/ubresnet_det.h): detector effects on a prepared training batch.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

LANE_PIXELS = 4             # UBX_LANE_PIXELS
BLOCK = 256                 # UBX_BLOCK
MAX_GRID = 1024             # UBX_MAX_GRID
PHILOX_TAG = 0x55425844     # UBX_PHILOX_TAG

vp, u32, i64, f32 = C.c_void_p, C.c_uint32, C.c_int64, C.c_float
BINDING = Binding("UBX_LIB", "libubresnet_det.so", "ubx", {
    "ubx_apply": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, f32, C.c_int, u32, u32,
                            C.c_int, i64, C.c_int, f32, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def row_words(width: int) -> int:
    """words of one (image, plane) row of the table: the gain and ceil(W / 32) mask words"""
    return 1 + (int(width) + 31) // 32


def apply(image: int, label, weight, shape, table: int, sigma: float = 0.0, noise_all: bool = False, seed: int = 0, seq: int = 0,
          dead_label=None, dead_weight=None, stream=None):
    """ubx_apply on raw device addresses (ints; `label` / `weight` may be None where their dead value is None); `shape` =
    (B, P, H, W); `table` the device address of the uint32 [B, P, row_words(W)] table; dead_label / dead_weight None: keep"""
    b, p, h, w = (int(v) for v in shape)
    rc = lib().ubx_apply(image, label, weight, b, p, h, w, table, float(sigma), 1 if noise_all else 0, int(seed), int(seq),
                         0 if dead_label is None else 1, 0 if dead_label is None else int(dead_label),
                         0 if dead_weight is None else 1, 0.0 if dead_weight is None else float(dead_weight), stream)
    check(rc, "apply")
