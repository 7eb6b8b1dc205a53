"""Reference of ubo_grad_norm's decision (include/ubresnet_opt.h) in fp64 / numpy, written from the header's rule, the
bias-correction table from ubr_adam_step's formula, and the table of cases that tests/test_gpu_opt_exact.py runs -- one entry per
kernel compiled into libubresnet_opt.so, which tests/test_cpu_opt.py holds against the library's symbol table.  No GPU and no
torch here.  Further down: the Adam and SGD steps of one element in numpy fp32, operation by operation, with the one fused
multiply-add of each rounded once from exact rational arithmetic -- what tests/opt_rule_host.cpp is held against.

Acceptance: sumsq, norm and everything a step writes are equal to the reference bit for bit; `scale` (one fp32 division on the
device) is within one fp32 ulp of the numpy fp32 formula and exactly 1.0 where nothing is clipped."""
import math
from fractions import Fraction

import numpy as np

# launch geometry and sizes, as include/ubresnet_opt.h states them (tests/test_cpu_opt.py holds these against the header)
BLOCK, UNROLL, MAX_GRID, CTL_HEAD_BYTES = 256, 4, 1024, 80
CTL_BYTES = CTL_HEAD_BYTES + 8 * MAX_GRID
# byte offsets of struct ubo_ctl
OFFSETS = dict(sumsq=0, norm=8, scale=12, gscale=16, apply=20, clipped=24, bc1=28, sqrt_bc2=32, reserved=36, applied=40,
               skipped=48, clipped_total=56, row=64)

# kernel (normal form of tools/kernel_symbols.py) -> ids of the cases in test_gpu_opt_exact.py that launch it
KERNEL_CASES = {
    "ctl_init_kernel": ["ctl-init"],
    "grad_sumsq_kernel": ["norm-sizes", "norm-fp64", "norm-grad-scale", "decide-sequence"],
    "grad_decide_kernel": ["norm-sizes", "decide-scale", "decide-sequence", "decide-nan-applies"],
    "guarded_adam_kernel": ["adam-bits", "adam-clipped", "adam-skip"],
    "guarded_sgd_kernel": ["sgd-bits", "sgd-clipped", "sgd-skip"],
}


def grid(n):
    """workgroups of the first launch for n floats"""
    n4 = n // 4
    return min((n4 + BLOCK * UNROLL - 1) // (BLOCK * UNROLL), MAX_GRID)


def norm_sizes():
    """n (floats) of the norm cases: the smallest; one float4 short of one workgroup's trip, exactly one, one over (a second
    workgroup with a single lane at work); and the capped grid with a second trip in which EVERY workgroup has work and the last
    one a ragged tail of 37 lanes"""
    trip = BLOCK * UNROLL
    full = MAX_GRID * trip
    two = full + (MAX_GRID - 1) * BLOCK + 37
    return {"n4": 4, "trip-1": 4 * (trip - 1), "trip": 4 * trip, "trip+1": 4 * (trip + 1), "two-trips": 4 * two}


def bias_table(beta1, beta2):
    """(float)(1 - pow(b1, t)), (float)sqrt(1 - pow(b2, t)) with b = (double)(float)beta, for t = 1 .. the first t at which both
    are 1.0f -> float32 [len, 2]"""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    rows, t = [], 0
    while True:
        t += 1
        c1, c2 = np.float32(1.0 - b1 ** t), np.float32(math.sqrt(1.0 - b2 ** t))
        rows.append((c1, c2))
        if c1 == 1.0 and c2 == 1.0:
            return np.array(rows, np.float32)
        assert t < (4 << 20)


def decide(sumsq, grad_scale, max_norm, skip_nonfinite, state, table):
    """the second launch of ubo_grad_norm on the host.  sumsq a Python float (fp64); state a dict with applied, skipped,
    clipped_total, bc1, sqrt_bc2 (updated in place); table float32 [len, 2].  -> dict of the fields the launch writes"""
    f = np.float32
    with np.errstate(all="ignore"):
        root = math.sqrt(sumsq) if sumsq >= 0 and math.isfinite(sumsq) else (float("inf") if sumsq == float("inf") else float("nan"))
        norm = f(abs(float(f(grad_scale))) * root)
        if max_norm < 0:
            scale = f(1.0)
        else:
            scale = np.fmin(f(max_norm) / (norm + f(1e-6)), f(1.0)).astype(np.float32)      # fminf: a NaN quotient gives 1.0f
        gscale = f(grad_scale) * scale
    apply = not (skip_nonfinite and not math.isfinite(sumsq))
    clipped = bool(apply and scale < 1.0)
    if apply:
        state["applied"] += 1
        state["clipped_total"] += int(clipped)
        row = table[min(state["applied"], len(table)) - 1]
        state["bc1"], state["sqrt_bc2"] = f(row[0]), f(row[1])
    else:
        state["skipped"] += 1
    return dict(sumsq=sumsq, norm=f(norm), scale=f(scale), gscale=f(gscale), apply=int(apply), clipped=int(clipped), **state)


def fma32(a, b, c):
    """a * b + c of three finite float32 values, rounded to float32 ONCE (ties to even), as fmaf does: the sum is formed in
    exact rational arithmetic.  (An fp64 multiply-add would round twice.)  Results in the normal or subnormal range only."""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        return np.float32(0.0)
    e = max(math.floor(math.log2(abs(x))), -126)
    while Fraction(2) ** e > abs(x) and e > -126:          # log2 of a value next to a power of two may land on the wrong side
        e -= 1
    while Fraction(2) ** (e + 1) <= abs(x):
        e += 1
    q = Fraction(2) ** (e - 23)                                # the spacing of float32 in [2^e, 2^(e+1))
    n = x / q
    r = math.floor(n)
    if n - r > Fraction(1, 2) or (n - r == Fraction(1, 2) and r % 2 == 1):
        r += 1
    out = np.float32(float(r * q))                             # r * q has at most 25 bits: exact in fp64, and a float32 by construction
    assert Fraction(float(out)) == r * q and np.isfinite(out)
    return out


def adam_element(p, g, m, v, gscale, wd, b1, b2, eps, lr, bc1, sqrt_bc2):
    """one element of ubo_adam_step / ubg_adam_step; every argument a np.float32 -> (p, m, v)"""
    one = np.float32(1.0)
    step_size = lr / bc1
    gr = fma32(wd, p, g * gscale)
    m = m + (one - b1) * (gr - m)
    v = b2 * v + (one - b2) * gr * gr
    denom = np.sqrt(v) / sqrt_bc2 + eps
    p = p - step_size * (m / denom)
    return p, m, v


def sgd_element(p, g, b, gscale, wd, lr, momentum, dampening, has_buf, first, nesterov):
    """one element of ubo_sgd_step / ubg_sgd_step -> (p, b); b comes back unchanged without a momentum buffer"""
    one = np.float32(1.0)
    gr = fma32(wd, p, g * gscale)
    if has_buf:
        b = gr if first else momentum * b + (one - dampening) * gr
        gr = fma32(momentum, b, gr) if nesterov else b
    return p - lr * gr, b
