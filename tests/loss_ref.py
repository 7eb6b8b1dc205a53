"""Float64 reference of libubresnet_loss.so (include/ubresnet_loss.h): the per-pixel focal term, its derivative, the three
denominators, the by-products of the control block, the finish rule, and the error bounds the GPU tests and the host program are
held to.  numpy only; a helper module for the tests (imported by name; not a conftest).

The bounds.  u = 2^-24 (kref.U32).  No copy of HIP's or OCML's accuracy tables is installed with the toolchain the tests run
against, so expf, expm1f, exp2f and log2f are each taken as within 2 ulp, i.e. a relative error of at most 4u (kref's convention:
"within 2 ulp (<= 4u relative)"); the HIP documentation is expected to give 1 ulp each, so this is twice that.  Every other step of
ubr_loss_term.h is one fp32 operation, relative error at most u.  Hats are computed values.

  q^ = clamp(-expm1f(lp)):  q (1 + 4u)   (clamping towards the interval that holds q does not move it away from q).
  m^ = q^gamma:
     gamma == 0:  1, exact.        gamma == 1:  q^, 4u.        gamma == 2:  fl(q^ q^), 4u + 4u + u = 9u.
     otherwise    log2f(q^) = log2 q + 4u / ln 2  (from q^)  + 4u |log2 q|  (the call);   fl(gamma * .): + u |gamma log2 q|;
                  an absolute error E in the exponent is a relative error E ln 2 in 2^E, and |log2 q| ln 2 = |ln q|:
                  gamma (4u + 5u |ln q|);   exp2f: + 4u.         eta = u (4 + gamma (4 + 5 |ln q|)).
     q^ == 0 (lp >= 0):  m is 0 or 1, exact: eta = 0.
  term = ((-(lp m^)) w_c) pw:  three more roundings (two at gamma == 0, where lp * 1 is exact):
     |term^ - term| <= C_ACC u |term| (a + gamma (b + c |ln q|)),   a = 7, b = 4, c = 5 in the general branch;
     2u, 7u, 12u times |term| for gamma = 0, 1, 2.       (C_ACC = 1.03 covers the second-order terms, as in kref.)
  d = m (c - 1), c = gamma p lp / q:
     p^ = expf(lp): 4u;  a = fl(gamma p^): + u;  b = fl(lp / q^): 4u + u;  c^ = fl(a b): + u  -- 11u |c|;
     e = fl(c^ - 1): + u |e|;   d^ = fl(m^ e): + (eta + u) |d|.      |d^ - d| <= |m| (11u |c| + u |e|) + |d| (eta + u).
     q^ == 0: d = -m, exact.   p^ == 0 or subnormal (lp below about -87): c is below 2^-120 and is lost in the u |e| above.
  g = (((g_loss inv_denom) pw) w_c) d:  four roundings, and inv_denom = fl(1 / fl(denom)) is within 1.5u of 1 / denom (the
     reference below divides in fp64):   |g^ - g| <= |S| |d^ - d| + 6u |g|,  S = g_loss pw w_c / denom.
  Gradual underflow (a subnormal product) adds up to 2^-150 absolutely per operation, scaled by the factors that follow it:
     FLOOR * max(1, |lp|) max(1, |w_c|) max(1, |pw|) for the term, FLOOR * (1 + |c|) for d (m^ = q^ q^ may underflow before it
     meets e), FLOOR * max(1, |S|) more for g, with FLOOR = 2^-147.
  The sums are fp64: each adds at most 2^-53 per addition, which N*H*W * 2^-53 * sum |term| covers many times over.

These are derived from the operations as written, never fitted to what a kernel returns: a ratio above 1 is a finding about the
kernel.  (The coefficient c of |ln q| is 5 = 2 * 2 ulp + 1 rounding; it would be 1 only with a correctly rounded log2f.)
"""
import numpy as np

U32 = 2.0 ** -24
C_ACC = 1.03
LIB = 4.0                 # relative error of a library call, in units of u: 2 ulp
FLOOR = 2.0 ** -147
A_TERM, B_TERM, C_LN = 7.0, 4.0, 5.0

BLOCK, UNROLL, MAX_GRID = 256, 2, 1024          # UBL_BLOCK, UBL_UNROLL, UBL_MAX_GRID
TRIP_PIXELS = BLOCK * UNROLL * 4
MAX_CLASSES = 16
MODES = ("pixels", "valid", "weights")


def grid(pixels):
    return min((pixels + TRIP_PIXELS - 1) // TRIP_PIXELS, MAX_GRID)


def miss(lp):
    """q = 1 - exp(lp), clamped to [0, 1]; NaN stays NaN"""
    with np.errstate(all="ignore"):
        x = -np.expm1(np.asarray(lp, dtype=np.float64))
        return np.where(x < 0, 0.0, np.where(x > 1, 1.0, x))


def modulator(q, gamma):
    with np.errstate(all="ignore"):
        if gamma == 0:
            return np.ones_like(q)
        return np.where(q == 0, 0.0, np.power(q, float(gamma)))


def term(lp, gamma, w=1.0):
    """-(1 - exp(lp))^gamma * lp * w"""
    lp = np.asarray(lp, dtype=np.float64)
    with np.errstate(all="ignore"):
        return -(lp * modulator(miss(lp), gamma)) * w


def deriv(lp, gamma):
    """d term / d lp at w = 1: m (gamma p lp / q - 1); -m where q == 0"""
    lp = np.asarray(lp, dtype=np.float64)
    q = miss(lp)
    m = modulator(q, gamma)
    with np.errstate(all="ignore"):
        p = np.exp(lp)
        c = np.where(p == 0, 0.0, float(gamma) * p * (lp / np.where(q == 0, 1.0, q)))
        return np.where(q == 0, -m, m * (c - 1.0))


def _eta(q, gamma):
    """relative error of m^ in units of u"""
    if gamma == 0:
        return np.zeros_like(q)
    if gamma == 1:
        return np.where(q == 0, 0.0, LIB)
    if gamma == 2:
        return np.where(q == 0, 0.0, 2 * LIB + 1)
    with np.errstate(all="ignore"):
        lnq = np.abs(np.log(np.where(q == 0, 1.0, q)))
    return np.where(q == 0, 0.0, LIB + float(gamma) * (B_TERM + C_LN * lnq))


def term_bound(lp, gamma, w_c=1.0, pw=1.0):
    lp = np.asarray(lp, dtype=np.float64)
    q = miss(lp)
    t = np.abs(term(lp, gamma, np.abs(np.asarray(w_c, dtype=np.float64) * pw)))
    roundings = 2.0 if gamma == 0 else 3.0
    floor = FLOOR * np.maximum(1.0, np.abs(lp)) * np.maximum(1.0, np.abs(w_c)) * np.maximum(1.0, np.abs(pw))
    return C_ACC * U32 * t * (_eta(q, gamma) + roundings) + floor


def deriv_bound(lp, gamma):
    lp = np.asarray(lp, dtype=np.float64)
    q = miss(lp)
    m = modulator(q, gamma)
    d = deriv(lp, gamma)
    with np.errstate(all="ignore"):
        p = np.exp(lp)
        c = np.where((p == 0) | (q == 0), 0.0, float(gamma) * p * (lp / np.where(q == 0, 1.0, q)))
    lim = np.abs(m) * ((2 * LIB + 3) * np.abs(c) + np.abs(c - 1.0)) + np.abs(d) * (_eta(q, gamma) + 1.0)
    return np.where(q == 0, 0.0, C_ACC * U32 * lim + FLOOR * (1.0 + np.abs(c)))


def mean(mode, loss_sum, weight_sum, valid, total):
    """the finish rule of ubr_loss_term.h, step for step -> (denom fp64, inv_denom fp32, loss fp32)"""
    denom = float(total) if mode == "pixels" else (float(valid) if mode == "valid" else float(weight_sum))
    if denom == 0.0:
        return denom, np.float32(0.0), np.float32(0.0)
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / np.float32(denom)
        return denom, inv, np.float32(np.float64(loss_sum) * (np.float64(1.0) / np.float64(denom)))


def forward(predict, target, pixelweights, classw, ignore_index, gamma, mode):
    """predict [N,C,H,W], target [N,H,W] int64, pixelweights [N,H,W], classw [C] or None (numpy arrays) -> dict: everything the
    control block holds, in fp64, plus the per-pixel terms, their bound, the mask of contributing pixels and the weights"""
    predict = np.asarray(predict, dtype=np.float64)
    N, C, H, W = predict.shape
    ok = (target != ignore_index) & (target >= 0) & (target < C)
    bad = int(((target != ignore_index) & ~ok).sum())
    t = np.clip(target, 0, C - 1)
    lp = np.take_along_axis(predict, t[:, None], axis=1)[:, 0]
    w_c = np.asarray(classw, dtype=np.float64)[t] if classw is not None else np.ones(t.shape)
    pw = np.asarray(pixelweights, dtype=np.float64)
    wp = (w_c.astype(np.float32) * pw.astype(np.float32)).astype(np.float64)          # the kernel's one fp32 product
    with np.errstate(all="ignore"):
        terms = np.where(ok, term(lp, gamma, w_c * pw), 0.0)
        lim = np.where(ok, term_bound(lp, gamma, w_c, pw), 0.0)
    loss_sum, weight_sum, valid = float(terms.sum()), float(np.where(ok, wp, 0.0).sum()), int(ok.sum())
    denom = float(N * H * W) if mode == "pixels" else (float(valid) if mode == "valid" else weight_sum)
    class_pixels = [int((ok & (t == c)).sum()) for c in range(C)]
    class_loss = [float(terms[ok & (t == c)].sum()) for c in range(C)]
    abs_sum = float(np.abs(terms).sum())
    return dict(loss_sum=loss_sum, weight_sum=weight_sum, valid=valid, bad=bad, denom=denom,
                loss=(loss_sum / denom if denom != 0 else 0.0), class_loss=class_loss, class_pixels=class_pixels,
                per_class_loss=[s / n if n else float("nan") for s, n in zip(class_loss, class_pixels)],
                terms=terms, lim=lim, lim_sum=float(lim.sum()) + N * H * W * 2.0 ** -53 * abs_sum, abs_sum=abs_sum, ok=ok, w_c=w_c, pw=pw,
                lp=lp, t=t)


def backward(g_loss, fwd, gamma, C):
    """fwd: forward()'s dict -> (g_predict [N,C,H,W] fp64: g at the target channel of contributing pixels, 0 elsewhere; its bound;
    the boolean map of the elements that may be non-zero)"""
    ok, lp, t = fwd["ok"], fwd["lp"], fwd["t"]
    denom = fwd["denom"]
    N, H, W = ok.shape
    g = np.zeros((N, C, H, W), dtype=np.float64)
    lim = np.zeros((N, C, H, W), dtype=np.float64)
    hot = np.zeros((N, C, H, W), dtype=bool)
    if denom == 0:
        np.put_along_axis(hot, t[:, None], ok[:, None], axis=1)
        return g, lim, hot
    with np.errstate(all="ignore"):
        S = float(g_loss) * fwd["pw"] * fwd["w_c"] / denom
        d = deriv(lp, gamma)
        val = np.where(ok, S * d, 0.0)
        vlim = np.where(ok, np.abs(S) * deriv_bound(lp, gamma) + C_ACC * U32 * 6.0 * np.abs(val) + FLOOR * np.maximum(1.0, np.abs(S)), 0.0)
    np.put_along_axis(g, t[:, None], val[:, None], axis=1)
    np.put_along_axis(lim, t[:, None], vlim[:, None], axis=1)
    np.put_along_axis(hot, t[:, None], ok[:, None], axis=1)
    return g, lim, hot
