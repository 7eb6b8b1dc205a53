"""ctypes binding of libubresnet_tta.so (the C ABI in include/ubresnet_tta.h): flip test-time augmentation of inference on the
device -- write a batch of input planes flipped, read the network's log-probabilities back un-flipped into a running merge that
ends as the log of the mean of the views' probabilities.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C
import math

from ._binding import Binding

BLOCK = 256          # UBT_BLOCK
UNROLL = 2           # UBT_UNROLL
MAX_GRID = 1024      # UBT_MAX_GRID
MAX_VIEWS = 4        # UBT_MAX_VIEWS
FLIP_ROWS, FLIP_COLS = 1, 2
# the names deploy.py takes for the views after the identity
FLIPS = {"rows": FLIP_ROWS, "cols": FLIP_COLS, "both": FLIP_ROWS | FLIP_COLS}

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
BINDING = Binding("UBT_LIB", "libubresnet_tta.so", "ubt", {
    "ubt_flip_planes": (C.c_int, [vp, vp, i64, i32, i32, i32, vp]),
    "ubt_merge_view": (C.c_int, [vp, vp, i64, i32, i32, i32, i32, i32, f32, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def parse_views(tta):
    """None / () -> () (off); a tuple of names from FLIPS -> the flip masks of the views, the identity first.  Duplicates, unknown
    names and anything that is not a tuple or list raise ValueError."""
    if tta is None:
        return ()
    if not isinstance(tta, (tuple, list)):
        raise ValueError("tta must be None or a tuple drawn from %s (got %r)" % (sorted(FLIPS), tta))
    if len(tta) == 0:
        return ()
    for name in tta:
        if not isinstance(name, str) or name not in FLIPS:
            raise ValueError("tta: unknown view %r; the views are %s" % (name, sorted(FLIPS)))
    if len(set(tta)) != len(tta):
        raise ValueError("tta: a view is named twice in %r" % (tuple(tta),))
    return (0,) + tuple(FLIPS[name] for name in tta)


def log_views(K: int) -> float:
    """the log_k argument of ubt_merge_view: log(K) in double; ctypes rounds it to float"""
    return math.log(float(K))


def flip_planes(src: int, dst: int, nplanes: int, H: int, W: int, flip: int, stream=None):
    """ubt_flip_planes on raw device addresses: dst = src with the rows and / or columns of every plane reversed"""
    check(lib().ubt_flip_planes(src, dst, int(nplanes), int(H), int(W), int(flip), stream), "flip_planes")


def merge_view(logp: int, acc: int, nplanes: int, H: int, W: int, flip: int, k: int, K: int, stream=None):
    """ubt_merge_view: view k of K, read un-flipped, into the running merge acc"""
    check(lib().ubt_merge_view(logp, acc, int(nplanes), int(H), int(W), int(flip), int(k), int(K), log_views(K), stream), "merge_view")
