"""ctypes binding of libubresnet_aug.so (the C ABI in include/ubresnet_aug.h): device-side augmentation of training batches.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import Binding

LANE_PIXELS = 4      # UBA_LANE_PIXELS
BLOCK = 256          # UBA_BLOCK
MAX_GRID = 1024      # UBA_MAX_GRID
MAX_BATCH = 256      # UBA_MAX_BATCH
MAX_PAD = 16383      # UBA_MAX_PAD

vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
BINDING = Binding("UBA_LIB", "libubresnet_aug.so", "uba", {
    "uba_augment_batch": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp,
                                    i32, C.c_int, f32, i32, f32, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def augment_batch(image: int, label_wire: int, weight, image_out: int, label_out: int, weight_out: int, shape, pad: int,
                  params, label_offset: int = 0, threshold=None, pad_label: int = 0, pad_weight: float = 0.0, stream=None):
    """uba_augment_batch on raw device addresses (ints; `weight` may be None); `shape` = (B, P, H, W); `params` a host
    int32 [B, 4] array of (flip_rows, flip_cols, off_r, off_c); `threshold` None switches the ADC threshold off"""
    b, p, h, w = (int(v) for v in shape)
    par = np.ascontiguousarray(params, dtype=np.int32)
    if par.shape != (b, 4):
        raise ValueError("augment_batch: params is %s, expected (%d, 4)" % (par.shape, b))
    rc = lib().uba_augment_batch(image, label_wire, weight, image_out, label_out, weight_out, b, p, h, w, int(pad),
                                 par.ctypes.data, int(label_offset), 0 if threshold is None else 1,
                                 0.0 if threshold is None else float(threshold), int(pad_label), float(pad_weight), stream)
    check(rc, "augment_batch")
