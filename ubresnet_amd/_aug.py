"""ctypes binding of libubresnet_aug.so (the C ABI in include/ubresnet_aug.h): device-side augmentation of training batches.

A library of its own next to libubresnet_hip.so (ubresnet_amd/_lib.py), libubresnet_post.so (ubresnet_amd/_post.py) and
libubresnet_data.so (ubresnet_amd/_data.py), with its own error string.  As there, NO fallback: a missing library or a failed
call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UBA_LIB", os.path.join(HERE, "libubresnet_aug.so"))

LANE_PIXELS = 4      # UBA_LANE_PIXELS
BLOCK = 256          # UBA_BLOCK
MAX_GRID = 1024      # UBA_MAX_GRID
MAX_BATCH = 256      # UBA_MAX_BATCH
MAX_PAD = 16383      # UBA_MAX_PAD

# every symbol include/ubresnet_aug.h declares (tests check that all of them are exported)
SYMBOLS = ["uba_augment_batch", "uba_last_error", "uba_version"]

_lib = None
_lock = threading.Lock()
vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float


def _declare(lib):
    lib.uba_last_error.restype = C.c_char_p
    lib.uba_last_error.argtypes = []
    lib.uba_version.restype = C.c_int
    lib.uba_version.argtypes = []
    lib.uba_augment_batch.restype = C.c_int
    lib.uba_augment_batch.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp,
                                      i32, C.c_int, f32, i32, f32, vp]


def lib():
    """Load (once) and return the library; raises RuntimeError if it is not built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        "ubresnet_amd: HIP extension %s is missing; build it with "
                        "`python -m ubresnet_amd.build` (hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
                try:
                    l = C.CDLL(LIB_PATH)
                except OSError as e:
                    raise RuntimeError("ubresnet_amd: cannot load %s: %s" % (LIB_PATH, e))
                _declare(l)
                _lib = l
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().uba_last_error().decode("utf-8", "replace")
        raise RuntimeError("ubresnet_amd HIP call failed (%d) %s: %s" % (rc, what, msg))


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
