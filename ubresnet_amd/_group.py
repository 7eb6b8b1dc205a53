"""ctypes binding of libubresnet_group.so (the C ABI in include/ubresnet_group.h): flat optimizer steps with parameter groups
and frozen parameters -- per-segment learning rate, weight decay, on/off switch and step count in one launch.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the tile planner (pure host code) and the argument checks of the
library can be exercised on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._binding import Binding

BLOCK = 256          # UBG_BLOCK
TILE_UNITS = 1024    # UBG_TILE_UNITS
MAX_GRID = 1024      # UBG_MAX_GRID
STEP_GRID = 2048     # UBG_STEP_GRID
CTL_HEAD_BYTES = 80  # UBG_CTL_HEAD_BYTES
CTL_BYTES = CTL_HEAD_BYTES + 8 * MAX_GRID   # UBG_CTL_BYTES

# the three 16-byte records as numpy dtypes (host copies of the device arrays)
TILE = np.dtype([("unit0", "<i8"), ("units", "<i4"), ("seg", "<i4")])
HYPER = np.dtype([("lr", "<f4"), ("weight_decay", "<f4"), ("active", "<i4"), ("reserved", "<i4")])
STATE = np.dtype([("applied", "<i8"), ("bc1", "<f4"), ("sqrt_bc2", "<f4")])


class Ctl(C.Structure):
    """struct ubg_ctl: the head of the control block, ubo_ctl's layout (UBG_MAX_GRID fp64 partials follow it on the device)"""
    _fields_ = [("sumsq", C.c_double), ("norm", C.c_float), ("scale", C.c_float), ("gscale", C.c_float), ("apply", C.c_int32),
                ("clipped", C.c_int32), ("bc1", C.c_float), ("sqrt_bc2", C.c_float), ("reserved", C.c_int32),
                ("applied", C.c_int64), ("skipped", C.c_int64), ("clipped_total", C.c_int64), ("row", C.c_float * 4)]


vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
BINDING = Binding("UBG_LIB", "libubresnet_group.so", "ubg", {
    "ubg_plan_tiles": (i64, [vp, vp, i64, vp, i64]),
    "ubg_state_set": (C.c_int, [vp, i64, i64, i64, vp, vp, i64, vp]),
    "ubg_state_get": (C.c_int, [vp, i64, vp, vp]),
    "ubg_grad_norm": (C.c_int, [vp, i64, vp, i64, vp, vp, i64, f32, f32, C.c_int, vp, i64, vp, vp]),
    "ubg_advance": (C.c_int, [vp, vp, i64, f32, vp, i64, vp, vp]),
    "ubg_adam_step": (C.c_int, [vp, vp, vp, vp, i64, vp, i64, vp, vp, i64, f32, f32, f32, vp, vp]),
    "ubg_sgd_step": (C.c_int, [vp, vp, vp, i64, vp, i64, vp, vp, i64, f32, f32, C.c_int, vp, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def read_ctl(raw: bytes) -> Ctl:
    """the head of a control block copied to the host (at least CTL_HEAD_BYTES bytes) as a Ctl"""
    return Ctl.from_buffer_copy(bytes(raw[:CTL_HEAD_BYTES]))


def tile_count(seg_units) -> int:
    """tiles that segments of these many units need"""
    return int(sum((int(u) + TILE_UNITS - 1) // TILE_UNITS for u in seg_units))


def plan_tiles(seg_unit0, seg_units, cap=None) -> np.ndarray:
    """ubg_plan_tiles (pure host code) -> the tile table as a numpy array of dtype TILE; `cap`: entries to provide room for
    (default: as many as are needed); a refused plan is a RuntimeError"""
    u0 = np.ascontiguousarray(seg_unit0, dtype=np.int64)
    un = np.ascontiguousarray(seg_units, dtype=np.int64)
    if u0.ndim != 1 or u0.shape != un.shape:
        raise ValueError("plan_tiles: seg_unit0 and seg_units must be 1-D and of one length")
    if cap is None:
        cap = tile_count(np.maximum(un, 0))
    tiles = np.zeros(max(int(cap), 1), dtype=TILE)
    nt = lib().ubg_plan_tiles(u0.ctypes.data, un.ctypes.data, len(u0), tiles.ctypes.data, int(cap))
    if nt < 0:
        check(int(nt), "plan_tiles")
    return tiles[:nt]


def state_set(state: int, nseg: int, seg0: int, count: int, applied: int, bc_table: int, bc_len: int, stream=None):
    check(lib().ubg_state_set(state, int(nseg), int(seg0), int(count), applied, bc_table, int(bc_len), stream), "state_set")


def state_get(state: int, nseg: int, stream=None) -> np.ndarray:
    """the segments' {applied, bc1, sqrt_bc2} as a numpy array of dtype STATE (synchronises the stream)"""
    out = np.zeros(int(nseg), dtype=STATE)
    check(lib().ubg_state_get(state, int(nseg), out.ctypes.data, stream), "state_get")
    return out


def grad_norm(grad: int, n: int, tiles: int, ntiles: int, hyper: int, state: int, nseg: int, grad_scale: float, max_norm,
              skip_nonfinite: bool, bc_table: int, bc_len: int, ctl: int, stream=None):
    """ubg_grad_norm on raw device addresses; `max_norm` None switches clipping off"""
    check(lib().ubg_grad_norm(grad, int(n), tiles, int(ntiles), hyper, state, int(nseg), float(grad_scale),
                              -1.0 if max_norm is None else float(max_norm), 1 if skip_nonfinite else 0, bc_table, int(bc_len),
                              ctl, stream), "grad_norm")


def advance(hyper: int, state: int, nseg: int, grad_scale: float, bc_table: int, bc_len: int, ctl: int, stream=None):
    check(lib().ubg_advance(hyper, state, int(nseg), float(grad_scale), bc_table, int(bc_len), ctl, stream), "advance")


def adam_step(param: int, grad: int, exp_avg: int, exp_avg_sq: int, n: int, tiles: int, ntiles: int, hyper: int, state: int,
              nseg: int, beta1, beta2, eps, ctl: int, stream=None):
    check(lib().ubg_adam_step(param, grad, exp_avg, exp_avg_sq, int(n), tiles, int(ntiles), hyper, state, int(nseg), float(beta1),
                              float(beta2), float(eps), ctl, stream), "adam_step")


def sgd_step(param: int, grad: int, momentum_buf, n: int, tiles: int, ntiles: int, hyper: int, state: int, nseg: int, momentum,
             dampening, nesterov, ctl: int, stream=None):
    check(lib().ubg_sgd_step(param, grad, momentum_buf, int(n), tiles, int(ntiles), hyper, state, int(nseg), float(momentum),
                             float(dampening), 1 if nesterov else 0, ctl, stream), "sgd_step")
