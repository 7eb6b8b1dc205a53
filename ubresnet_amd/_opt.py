"""ctypes binding of libubresnet_opt.so (the C ABI in include/ubresnet_opt.h): the guarded flat optimizer step -- global
gradient norm, clipping by it and the skip of a non-finite step, decided on the device.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library and the bias-correction table
can be exercised on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._binding import Binding

BLOCK = 256          # UBO_BLOCK
UNROLL = 4           # UBO_UNROLL
MAX_GRID = 1024      # UBO_MAX_GRID
CTL_HEAD_BYTES = 80  # UBO_CTL_HEAD_BYTES
CTL_BYTES = CTL_HEAD_BYTES + 8 * MAX_GRID   # UBO_CTL_BYTES
MAX_TABLE = 4 << 20  # rows of a bias-correction table; more is refused


class Ctl(C.Structure):
    """struct ubo_ctl: the head of the control block (UBO_MAX_GRID fp64 partials follow it on the device)"""
    _fields_ = [("sumsq", C.c_double), ("norm", C.c_float), ("scale", C.c_float), ("gscale", C.c_float), ("apply", C.c_int32),
                ("clipped", C.c_int32), ("bc1", C.c_float), ("sqrt_bc2", C.c_float), ("reserved", C.c_int32),
                ("applied", C.c_int64), ("skipped", C.c_int64), ("clipped_total", C.c_int64), ("row", C.c_float * 4)]


vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
BINDING = Binding("UBO_LIB", "libubresnet_opt.so", "ubo", {
    "ubo_ctl_init": (C.c_int, [vp, i64, vp]),
    "ubo_grad_norm": (C.c_int, [vp, i64, f32, f32, C.c_int, vp, i64, vp, vp]),
    "ubo_adam_step": (C.c_int, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, vp, vp]),
    "ubo_sgd_step": (C.c_int, [vp, vp, vp, i64, f32, f32, f32, f32, C.c_int, vp, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def bias_table(beta1: float, beta2: float) -> np.ndarray:
    """Adam's bias corrections as ubr_adam_step forms them from its float arguments -- (float)(1 - pow(b1, t)) and
    (float)sqrt(1 - pow(b2, t)), pow and sqrt in double -- for t = 1 .. the first t at which both are 1.0f; they stay 1.0f
    from there on.  -> float32 [len, 2].  (math.pow is the C library's pow, the one the host code of the kernels calls.)"""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError("bias_table: betas (%r, %r) must lie in [0, 1)" % (beta1, beta2))
    rows, one, t = [], np.float32(1.0), 0
    while True:
        t += 1
        if t > MAX_TABLE:
            raise ValueError("bias_table: betas (%r, %r) need more than %d rows" % (beta1, beta2, MAX_TABLE))
        c1 = np.float32(1.0 - math.pow(b1, t))
        c2 = np.float32(math.sqrt(1.0 - math.pow(b2, t)))
        rows.append((c1, c2))
        if c1 == one and c2 == one:
            return np.array(rows, dtype=np.float32).reshape(-1, 2)


def read_ctl(raw: bytes) -> Ctl:
    """the head of a control block copied to the host (at least CTL_HEAD_BYTES bytes) as a Ctl"""
    return Ctl.from_buffer_copy(bytes(raw[:CTL_HEAD_BYTES]))


def ctl_init(ctl: int, applied: int = 0, stream=None):
    check(lib().ubo_ctl_init(ctl, int(applied), stream), "ctl_init")


def grad_norm(grad: int, n: int, grad_scale: float, max_norm, skip_nonfinite: bool, bc_table: int, bc_len: int, ctl: int, stream=None):
    """ubo_grad_norm on raw device addresses; `max_norm` None switches clipping off"""
    check(lib().ubo_grad_norm(grad, int(n), float(grad_scale), -1.0 if max_norm is None else float(max_norm),
                              1 if skip_nonfinite else 0, bc_table, int(bc_len), ctl, stream), "grad_norm")


def adam_step(param: int, grad: int, exp_avg: int, exp_avg_sq: int, n: int, lr, beta1, beta2, eps, weight_decay, ctl: int, stream=None):
    check(lib().ubo_adam_step(param, grad, exp_avg, exp_avg_sq, int(n), float(lr), float(beta1), float(beta2), float(eps),
                              float(weight_decay), ctl, stream), "adam_step")


def sgd_step(param: int, grad: int, momentum_buf, n: int, lr, momentum, dampening, weight_decay, nesterov, ctl: int, stream=None):
    check(lib().ubo_sgd_step(param, grad, momentum_buf, int(n), float(lr), float(momentum), float(dampening), float(weight_decay),
                             1 if nesterov else 0, ctl, stream), "sgd_step")
