"""ctypes binding of libubresnet_weight.so (the C ABI in include/ubresnet_weight.h): pixel weights of the loss made on the
device -- per-image class balance and an interface gain.

A library of its own next to libubresnet_hip.so (ubresnet_amd/_lib.py), libubresnet_post.so (ubresnet_amd/_post.py),
libubresnet_data.so (ubresnet_amd/_data.py), libubresnet_aug.so (ubresnet_amd/_aug.py) and libubresnet_opt.so
(ubresnet_amd/_opt.py), with its own error string.  As there, NO fallback: a missing library or a failed call is a
RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UBW_LIB", os.path.join(HERE, "libubresnet_weight.so"))

MAX_CLASSES = 16     # UBW_MAX_CLASSES
MAX_RADIUS = 4       # UBW_MAX_RADIUS
# launch geometry of ubresnet_amd/csrc/ubr_weight_tile.h (not part of the C ABI; tests hold these against that file)
LANE_PIXELS = 4      # UBW_LANE_PIXELS
BLOCK = 256          # UBW_BLOCK
MAX_GRID = 2048      # UBW_MAX_GRID
TILE_W = 64          # UBW_TILE_W
TILE_H = 16          # UBW_TILE_H

# every symbol include/ubresnet_weight.h declares (tests check that all of them are exported)
SYMBOLS = ["ubw_pixel_weights", "ubw_last_error", "ubw_version"]

_lib = None
_lock = threading.Lock()
vp, f32 = C.c_void_p, C.c_float


def _declare(lib):
    lib.ubw_last_error.restype = C.c_char_p
    lib.ubw_last_error.argtypes = []
    lib.ubw_version.restype = C.c_int
    lib.ubw_version.argtypes = []
    lib.ubw_pixel_weights.restype = C.c_int
    lib.ubw_pixel_weights.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32, C.c_int, f32, C.c_int, vp]


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
        msg = lib().ubw_last_error().decode("utf-8", "replace")
        raise RuntimeError("ubresnet_amd HIP call failed (%d) %s: %s" % (rc, what, msg))


def pixel_weights(label: int, weight: int, counts: int, shape, num_classes: int, max_weight: float, radius: int, gain: float,
                  lo: int, stream=None):
    """ubw_pixel_weights on raw device addresses; `shape` is (B, H, W)"""
    b, h, w = (int(v) for v in shape)
    check(lib().ubw_pixel_weights(label, weight, counts, b, h, w, int(num_classes), float(max_weight), int(radius), float(gain),
                                  int(lo), stream), "pixel_weights")
