"""ctypes binding of libubresnet_calib.so (the C ABI in include/ubresnet_calib.h): temperature calibration on the device -- the
negative log-likelihood of the class scores, its first and second derivative in the inverse temperature, summed over the lit,
labelled pixels at up to 64 inverse temperatures per call, and the streaming rescale of tile scores by one inverse temperature per
tile.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

MAX_CLASSES = 16     # UBF_MAX_CLASSES
REG_CLASSES = 4      # UBF_REG_CLASSES
MAX_TEMPS = 64       # UBF_MAX_TEMPS
MAX_GROUPS = 256     # UBF_MAX_GROUPS
MAX_IMAGES = 65535   # UBF_MAX_IMAGES
TRUTH_U8, TRUTH_I64 = 0, 1

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
BINDING = Binding("UBF_LIB", "libubresnet_calib.so", "ubf", {
    "ubf_scratch_bytes": (i64, [i32, i32, i32, i32]),
    "ubf_accumulate": (C.c_int, [vp, vp, i32, vp, C.c_float, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp]),
    "ubf_apply": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def scratch_bytes(N: int, H: int, W: int, K: int) -> int:
    """bytes of scratch one ubf_accumulate call of these extents needs (ubf_scratch_bytes, which refuses what the call refuses)"""
    n = lib().ubf_scratch_bytes(int(N), int(H), int(W), int(K))
    if n <= 0:
        check(-1, "scratch_bytes")
    return n


def accumulate(scores: int, truth: int, truth_kind: int, lit, lit_threshold: float, group: int, betas: int, K: int, N: int, Cn: int,
               H: int, W: int, G: int, table: int, counters: int, scratch: int, nbytes: int, stream=None):
    """ubf_accumulate on raw device addresses; `lit` None: every pixel counts"""
    check(lib().ubf_accumulate(scores, truth, int(truth_kind), lit, float(lit_threshold), group, betas, int(K), int(N), int(Cn), int(H),
                               int(W), int(G), table, counters, scratch, int(nbytes), stream), "accumulate")


def apply(src: int, dst: int, betas: int, n: int, Cn: int, th: int, tw: int, stream=None):
    """ubf_apply on raw device addresses; dst == src: in place"""
    check(lib().ubf_apply(src, dst, betas, int(n), int(Cn), int(th), int(tw), stream), "apply")
