"""Float64 reference of libubresnet_dice.so (include/ubresnet_dice.h): the batch-wide soft counts TP, FP, FN per class, the finish
(Tversky index, loss, the two backward coefficients per class), the gradient, and the error bounds the GPU tests and the host
program are held to.  numpy only; a helper module for the tests (imported by name; not a conftest).

The bounds.  u = 2^-24.  As in tests/loss_ref.py no accuracy table of the device library is installed, so expf and expm1f are
each taken as within 2 ulp, a relative error of at most 4u (LIB); every fp32 multiply is within u; an fp64 sum of n terms adds at
most n 2^-53 relatively.  Hats are computed values.

  An addend.  pw p^ with p^ = expf(lp) (1 + 4u), then one multiply: relative error (4 + 1) u = 5u.  pw q^ with
  q^ = clamp(-expm1f(lp)) (clamping towards the interval that holds q does not move it away from q): 5u as well.  Gradual underflow
  (a subnormal p^, q^ or product) adds up to FLOOR = 2^-147 times max(1, pw) absolutely per addend.
  A sum.  Every addend of TP_c, FP_c and FN_c is non-negative, so the relative errors carry to the sum X of k addends:
      |X^ - X| <= dX = (C_ACC 5u + n 2^-53) X + k FLOOR max(1, max pw),     n = N*H*W, C_ACC = 1.03 for the second-order terms.
  The finish is fp64 on these sums; its own roundings (a few tens of operations) are covered by E64 = 64 * 2^-53 relatively.
  alpha, beta and eps are the fp32 arguments, exact in fp64, and >= 0, so Nn = TP + eps, M = alpha FP + beta FN and Dn = TP + M + eps
  are sums of non-negative terms:  dN = dTP,  dM = alpha dFP + beta dFN,  dD = dTP + dM,  and Dn^ >= Dlo = Dn - dD.
      T = Nn / Dn:                     |T^ - T| <= (dN + T dD) / Dlo + E64 T
      1 - T = M / Dn:                  |.| <= (dM + (M / Dn) dD) / Dlo + E64
      loss = (float) sum_c a_c M_c / Dn_c:   sum_c a_c (the line above) + u |loss| + 2^-149 (the rounding to fp32)
      x / Dn^2 for x = P1 = beta Nn + M (dP1 = beta dN + dM) or x = alpha Nn:
          |x^ / Dn^2^ - x / Dn^2| <= dx / Dlo^2 + x (Dn + Dlo) dD / (Dn^2 Dlo^2) <= (dx + 2 x dD / Dlo) / Dlo^2   (times 1.01: x^ for x)
      K1 = -(a P1 / Dn^2), K0 = a alpha Nn / Dn^2, each rounded to fp32 once: + (u + E64) |K| + 2^-149.
      a_c = w_c present_c / S is formed from exact fp32 class weights and an exact integer count: E64 covers it.
  Dn == 0 is possible only with every addend exactly 0 (then dD = 0 too): T = 1, the coefficients 0, exactly.
  The gradient.  g = ((g_loss pw) p^) K^: three multiplies and one expf, 7u relatively, plus the error of K^ scaled by |g_loss pw p|,
  plus FLOOR max(1, |g_loss pw|) max(1, |K|) for a subnormal p^ or product.

These are derived from the operations as written, never fitted to what a kernel returns: a ratio above 1 is a finding about the
kernel.
"""
import numpy as np

U32 = 2.0 ** -24
C_ACC = 1.03
LIB = 4.0                 # relative error of a library call, in units of u: 2 ulp
FLOOR = 2.0 ** -147
E64 = 64 * 2.0 ** -53
TERM_U = LIB + 1.0        # an addend: one library call and one multiply
GRAD_U = LIB + 3.0        # a gradient element: one library call and three multiplies

BLOCK, UNROLL, MAX_GRID = 256, 2, 1024          # UBK_BLOCK, UBK_UNROLL, UBK_MAX_GRID
TRIP_PIXELS = BLOCK * UNROLL * 4
MAX_CLASSES, REG_CLASSES = 16, 4


def grid(pixels):
    return min((pixels + TRIP_PIXELS - 1) // TRIP_PIXELS, MAX_GRID)


def miss(lp):
    """q = 1 - exp(lp), clamped to [0, 1]; NaN stays NaN"""
    with np.errstate(all="ignore"):
        x = -np.expm1(np.asarray(lp, dtype=np.float64))
        return np.where(x < 0, 0.0, np.where(x > 1, 1.0, x))


def term_bound(value, pw):
    """bound of one addend pw * p or pw * q whose exact value is `value`"""
    return C_ACC * U32 * TERM_U * np.abs(value) + FLOOR * np.maximum(1.0, np.abs(pw))


def finish(tp, fp, fn, pixels, classw, alpha, beta, eps, present_only, d_tp=None, d_fp=None, d_fn=None):
    """the finish rule on fp64 sums (arrays of C) -> dict with T, K1, K0 (fp64, not rounded), loss, S, a, and, given the bounds of
    the sums, lim_T, lim_K1, lim_K0, lim_loss"""
    tp, fp, fn = (np.asarray(v, dtype=np.float64) for v in (tp, fp, fn))
    C = tp.shape[0]
    alpha, beta, eps = float(np.float32(alpha)), float(np.float32(beta)), float(np.float32(eps))
    w = np.ones(C) if classw is None else np.asarray(classw, dtype=np.float32).astype(np.float64)
    present = (np.asarray(pixels) > 0) if present_only else np.ones(C, dtype=bool)
    S = float(np.where(present, w, 0.0).sum())
    live = S != 0.0
    with np.errstate(all="ignore"):
        a = np.where(present & live, w / (S if live else 1.0), 0.0)
        nn, m = tp + eps, alpha * fp + beta * fn
        dn = tp + m + eps
        zero = dn == 0.0
        safe = np.where(zero, 1.0, dn)
        T = np.where(zero, 1.0, nn / safe)
        dead = zero | (not live)
        one_minus = np.where(dead, 0.0, m / safe)
        p1 = beta * nn + m
        K1 = np.where(dead, 0.0, -(a * p1) / safe ** 2)
        K0 = np.where(dead, 0.0, (a * (alpha * nn)) / safe ** 2)
        loss = float((a * one_minus).sum()) if live else 0.0
    out = dict(T=T, K1=K1, K0=K0, loss=loss, S=S, a=a, present=present)
    if d_tp is None:
        return out
    d_tp, d_fp, d_fn = (np.asarray(v, dtype=np.float64) for v in (d_tp, d_fp, d_fn))
    with np.errstate(all="ignore"):
        dN, dM = d_tp, alpha * d_fp + beta * d_fn
        dD = dN + dM
        dlo = dn - dD
        ok = dlo > 0
        dl = np.where(ok, dlo, 1.0)
        lim_T = np.where(zero & (dD == 0), 0.0, np.where(ok, (dN + T * dD) / dl + E64 * T, np.inf))
        lim_1mT = np.where(dead, 0.0, np.where(ok, (dM + one_minus * dD) / dl + E64, np.inf))
        dP1 = beta * dN + dM
        lim_K1 = np.where(dead, 0.0, np.where(ok, 1.01 * a * (dP1 + 2 * p1 * dD / dl) / dl ** 2 + (U32 + E64) * np.abs(K1) + 2.0 ** -149, np.inf))
        lim_K0 = np.where(dead, 0.0, np.where(ok, 1.01 * a * alpha * (dN + 2 * nn * dD / dl) / dl ** 2 + (U32 + E64) * np.abs(K0) + 2.0 ** -149, np.inf))
        lim_loss = float((a * lim_1mT).sum()) + U32 * abs(loss) + 2.0 ** -149 if live else 0.0
    out.update(lim_T=lim_T, lim_K1=lim_K1, lim_K0=lim_K0, lim_loss=lim_loss)
    return out


def sums(predict, target, pixelweights, ignore_index):
    """predict [N,C,H,W], target [N,H,W] int64, pixelweights [N,H,W] (numpy arrays) -> dict: the fp64 sums and counts, their bounds,
    and what backward() needs; nothing here depends on alpha, beta, eps, the class weights or present_only"""
    predict = np.asarray(predict, dtype=np.float64)
    N, C, H, W = predict.shape
    target = np.asarray(target)
    ok = (target != ignore_index) & (target >= 0) & (target < C)
    bad = int(((target != ignore_index) & ~ok).sum())
    pw = np.asarray(pixelweights, dtype=np.float64)
    n_all = N * H * W
    pw_max = max(1.0, float(np.abs(pw[ok]).max())) if ok.any() else 1.0
    rel = C_ACC * U32 * TERM_U + n_all * 2.0 ** -53
    tp, fp, fn, pixels = np.zeros(C), np.zeros(C), np.zeros(C), [0] * C
    with np.errstate(all="ignore"):
        p = np.exp(predict)
        for c in range(C):
            is_c = ok & (target == c)
            other = ok & (target != c)
            pixels[c] = int(is_c.sum())
            tp[c] = (pw * p[:, c])[is_c].sum()
            fn[c] = (pw * miss(predict[:, c]))[is_c].sum()
            fp[c] = (pw * p[:, c])[other].sum()
    valid = int(ok.sum())
    counts = np.asarray(pixels, dtype=np.float64)
    return dict(tp=tp, fp=fp, fn=fn, pixels=pixels, valid=valid, bad=bad, d_tp=rel * tp + counts * FLOOR * pw_max,
                d_fn=rel * fn + counts * FLOOR * pw_max, d_fp=rel * fp + (valid - counts) * FLOOR * pw_max, ok=ok, pw=pw, p=p, target=target,
                weighted_pixels=[float(pw[ok & (target == c)].sum()) for c in range(C)])


def complete(s, classw, alpha=0.5, beta=0.5, eps=1.0, present_only=True):
    """sums()'s dict and the parameters of the finish -> the dict of forward()"""
    out = dict(s)
    out.update(finish(s["tp"], s["fp"], s["fn"], s["pixels"], classw, alpha, beta, eps, present_only, s["d_tp"], s["d_fp"], s["d_fn"]))
    return out


def forward(predict, target, pixelweights, classw, ignore_index, alpha=0.5, beta=0.5, eps=1.0, present_only=True):
    """-> dict: everything the control block holds, in fp64, the bounds of the sums and of what the finish derives from them"""
    return complete(sums(predict, target, pixelweights, ignore_index), classw, alpha, beta, eps, present_only)


def backward(g_loss, fwd):
    """fwd: forward()'s dict -> (g_predict [N,C,H,W] fp64, its bound, the [N,H,W] map of contributing pixels): at a contributing
    pixel g_c = g_loss pw p_c (c == t ? K1_c : K0_c), 0 in every channel elsewhere"""
    ok, pw, p, target = fwd["ok"], fwd["pw"], fwd["p"], fwd["target"]
    N, C, H, W = p.shape
    onehot = target[:, None] == np.arange(C)[None, :, None, None]
    with np.errstate(all="ignore"):
        K = np.where(onehot, fwd["K1"][None, :, None, None], fwd["K0"][None, :, None, None])
        limK = np.where(onehot, fwd["lim_K1"][None, :, None, None], fwd["lim_K0"][None, :, None, None])
        s = float(g_loss) * pw[:, None]
        g = np.where(ok[:, None], s * p * K, 0.0)
        lim = C_ACC * U32 * GRAD_U * np.abs(g) + np.abs(s * p) * limK * (1.0 + 1e-6) + FLOOR * np.maximum(1.0, np.abs(s)) * np.maximum(1.0, np.abs(K))
        lim = np.where(ok[:, None], lim, 0.0)
    return g, lim, ok
