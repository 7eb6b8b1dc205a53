"""numpy replay of libubresnet_ema.so (include/ubresnet_ema.h): the schedule of ube_advance in Python floats -- the same fp64
operations as the device's, in the same order -- and the update as three np.float32 operations, each rounded once.  Geometry
and the control block's layout are restated here so that tests hold the header, the binding and this file against each other."""
import numpy as np

BLOCK, UNROLL, MAX_GRID, SEG_GRID, CTL_BYTES = 256, 4, 1024, 256, 32
TRIP = BLOCK * UNROLL                    # units (of four floats) a workgroup takes per trip
OFFSETS = dict(apply=0, w=4, d=8, reserved=12, updates=16, held=24)
APPLY_OFFSET = 20                        # `apply` in ubo_ctl and in ubg_ctl

f32 = np.float32


def schedule(decay, warmup, u):
    """-> (w, d) as np.float32 for the update that follows `u` applied ones; `decay` is taken as the fp32 value the C ABI gets"""
    d = float(f32(decay))
    if warmup >= 2:
        d = min(d, (1.0 + u) / (warmup + u))
    return f32(1.0 - d), f32(d)


def crossover(decay, warmup):
    """the first u at which (1 + u) / (warmup + u) is no longer below decay (None if there is none below 2^40)"""
    d = float(f32(decay))
    if warmup < 2 or d <= 1.0 / warmup:
        return 0 if warmup >= 2 else None
    u = int((d * warmup - 1.0) / (1.0 - d))
    u = max(u - 4, 0)
    while (1.0 + u) / (warmup + u) < d:
        u += 1
        if u > 1 << 40:
            return None
    return u


def update(s, p, w):
    """s + w * (p - s) in fp32, three roundings (numpy keeps subnormals); -> a new array"""
    s, p = np.asarray(s, dtype=f32), np.asarray(p, dtype=f32)
    with np.errstate(all="ignore"):
        return (s + f32(w) * (p - s)).astype(f32)


class Ctl(object):
    """the control block on the host"""

    def __init__(self, updates=0):
        self.apply, self.w, self.d, self.updates, self.held = 0, f32(0), f32(0), int(updates), 0

    def advance(self, flag, decay, warmup):
        """flag None: apply; else apply iff flag != 0.  -> apply"""
        if flag is None or flag != 0:
            self.w, self.d = schedule(decay, warmup, self.updates)
            self.updates += 1
            self.apply = 1
        else:
            self.held += 1
            self.apply = 0
        return self.apply


def flat_sizes():
    """float counts n for ube_update / ube_swap, from the geometry: one unit; a workgroup's trip less one unit, exactly, plus one;
    several workgroups with a ragged last grid trip below the grid cap; just past the cap (the grid-stride loop runs twice)"""
    return [4, 4 * (TRIP - 1), 4 * TRIP, 4 * (TRIP + 1), 4 * (5 * TRIP + 3 * BLOCK + 19), 4 * (MAX_GRID * TRIP + 37)]


def grid(n):
    units = n // 4
    return min((units + TRIP - 1) // TRIP, MAX_GRID)
