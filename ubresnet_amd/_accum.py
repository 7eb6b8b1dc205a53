"""ctypes binding of libubresnet_accum.so (the C ABI in include/ubresnet_accum.h): gradient accumulation over the flat gradient
buffer on the device -- copy the first micro-batch into the accumulator, add the ones in between, write the scaled sum back into
the flat gradient buffer with the last.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

BLOCK = 256          # UBC_BLOCK
UNROLL = 4           # UBC_UNROLL
MAX_GRID = 1024      # UBC_MAX_GRID

vp, i64, f32 = C.c_void_p, C.c_int64, C.c_float
BINDING = Binding("UBC_LIB", "libubresnet_accum.so", "ubc", {
    "ubc_set": (C.c_int, [vp, vp, i64, vp]),
    "ubc_add": (C.c_int, [vp, vp, i64, vp]),
    "ubc_finish": (C.c_int, [vp, vp, i64, f32, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def set_(acc: int, grad: int, n: int, stream=None):
    """ubc_set on raw device addresses: acc = grad, bit for bit"""
    check(lib().ubc_set(acc, grad, int(n), stream), "set")


def add(acc: int, grad: int, n: int, stream=None):
    """ubc_add: acc += grad"""
    check(lib().ubc_add(acc, grad, int(n), stream), "add")


def finish(grad: int, acc: int, n: int, scale: float, stream=None):
    """ubc_finish: grad = (acc + grad) * scale; acc is left as it is"""
    check(lib().ubc_finish(grad, acc, int(n), float(scale), stream), "finish")
