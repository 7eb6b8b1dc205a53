"""Float64 reference of libubresnet_calib.so (include/ubresnet_calib.h) and of the solver of ubresnet_amd/calibration.py: the sums
of NLL, g and h over the counting pixels, the rescale of tile scores, the root of the Hermite interpolant, the error bound of every
output, and the kernel -> case table that tests/test_cpu_calib.py holds against the symbol table of the built library.  numpy only;
a helper module for the tests (imported by name; not a conftest).

The bounds.  u = 2^-24.  As in tests/tta_ref.py and tests/loss_ref.py each library call (expf, logf) is taken as within 2 ulp, a
relative error of at most LIB u = 4u, and each fp32 add, subtract, multiply or (correctly rounded) divide as half an ulp, a
relative error of at most u.  Hats are computed values; everything else is the fp64 reference.  Per pixel and beta, with
d_c = l_c - max l, z_c = beta d_c <= 0, e_c = exp(z_c) <= 1, S = sum e_c in [1, C], p_c = e_c / S:

  d^_c: u |d_c|.   z^_c = fl(beta d^_c): 2u |z_c|.   e^_c = expf(z^_c): relative (LIB + 2 |z_c|) u.
  S^: the terms' errors and C - 1 adds:  relative rS u,  rS = sum_c p_c (LIB + 2 |z_c|) + (C - 1).
  L^ = logf(S^): LIB u L + rS u  (d log S = dS / S).

  ubf_apply   out_c = fl(z^_c - L^):                u (2 |z_c| + LIB L + rS + |out_c|)
  NLL = fl(L^ - fl(beta d^_t)):                     u (rS + LIB L + 2 |z_t| + |NLL|)
  A^ = sum e^_c d^_c: each product relative (LIB + 2 |z_c| + 2) u, C - 1 adds;  dA = u sum_c p_c |d_c| (LIB + 2 |z_c| + 2 + C - 1)
     is its error after the division by S;  mean^ = fl(A^ / S^):  dmean = dA + u |mean| (rS + 1)
  g = fl(mean^ - d^_t):                             dmean + u (|d_t| + |g|)
  r^_c = fl(d^_c - mean^): dr_c = u |d_c| + dmean + u |r_c|;  r^2: 2 |r_c| dr_c + u r_c^2;  e^_c r^2: relative LIB + 2 |z_c| + 1
     more; C - 1 adds; the division by S^ (rS + 1):
  h:   sum_c p_c (2 |r_c| dr_c + u r_c^2 (LIB + 2 |z_c| + 2 + C - 1)) + u h (rS + 1)

  Gradual underflow: an intermediate below 2^-126 is carried with an absolute error of 2^-149 instead; at most 6 C of them per
  output, each scaled by at most 1 + D^2, D = max |d_c|:  FLOOR = 6 C 2^-149 (1 + D^2).
  Everything times C_ACC = 1.03 for the second-order terms, as in kref.

  The fp64 sums: the fp32 terms convert exactly; a sum of n terms carries the terms' bounds plus (n + SLACK) 2^-53 sum |term| for
  the additions in any order (SLACK = 16 covers the levels of the tree: lanes, waves, rows, sequences, the table).

Derived from the operations as written, never fitted to what the kernel returns: a ratio above 1 is a finding.

The arg-max margin of ubf_apply.  fl(l - m), fl(beta x) and fl(x - L) are monotone, so the order of two classes can never invert;
it can only tie, when the runner-up's |z| is below half an ulp of L.  L <= ln 16 < 4, so ulp(L) <= 2^-22; z = beta (l_2 - l_1)
within 2u relative.  A top-2 margin above MARGIN(beta) = 2^-22 / beta therefore keeps the arg-max (a factor two to spare).
"""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
C_ACC = 1.03
LIB = 4.0
SLACK = 16
QNAN_BITS = 0x7FC00000

BLOCK, UNROLL, LANE_PIXELS = 256, 2, 4                 # ubf::BLOCK, UNROLL, LANE_PIXELS of csrc/ubr_calib_plan.h
TRIP_PIXELS = BLOCK * UNROLL * LANE_PIXELS
MAX_ROWS, MAX_TEMPS, MAX_CLASSES, REG_CLASSES = 768, 64, 16, 4


def margin(beta):
    return 2.0 ** -22 / float(beta)


def default_temps():
    return [4.0 ** (i / 16.0 - 1.0) for i in range(33)]


def betas32(temps):
    return np.array([1.0 / t for t in temps], dtype=np.float64).astype(np.float32)


def accum_kernel(ct, i64):
    """normal form of tools/kernel_symbols.py"""
    return "accum_kernel<%d, %s>" % (ct, "long long" if i64 else "unsigned char")


def apply_kernel(ct, vec):
    return "apply_kernel<%d, %s>" % (ct, "true" if vec else "false")


def class_form(C):
    return C if C <= REG_CLASSES else 0


# ------------------------------------------------------------------------------------------------------------------------
# the accumulate cases of tests/test_gpu_calib_exact.py: shape (N, C, H, W), K, truth kind, lit, groups
# ------------------------------------------------------------------------------------------------------------------------
ACC_CASES = {
    "one-pixel": dict(shape=(1, 2, 1, 1), K=1, i64=False, lit="none", G=1),
    "nothing-counts": dict(shape=(2, 3, 5, 8), K=3, i64=True, lit="dark", G=2),
    "odd-width": dict(shape=(2, 3, 7, 33), K=32, i64=False, lit="cut", G=2),                   # scalar path: 231 % 4 != 0
    "partial-trip": dict(shape=(1, 4, 40, 60), K=5, i64=True, lit="cut", G=1),                 # 2400 pixels: a second, partial trip
    "two-workgroups": dict(shape=(2, 3, 64, 96), K=33, i64=True, lit="cut", G=3, groups=(2, 0)),   # 3 trips per image, vector path
    "all-lit-c1": dict(shape=(1, 1, 4, 8), K=2, i64=False, lit="none", G=1),
    "c1-i64": dict(shape=(1, 1, 5, 9), K=1, i64=True, lit="none", G=1),
    "c2-i64": dict(shape=(1, 2, 8, 12), K=4, i64=True, lit="cut", G=1),
    "c2-u8": dict(shape=(3, 2, 8, 12), K=4, i64=False, lit="cut", G=3),
    "c3-u8": dict(shape=(1, 3, 16, 20), K=7, i64=False, lit="none", G=1),
    "c4-u8": dict(shape=(2, 4, 16, 24), K=33, i64=False, lit="cut", G=1),
    "c4-i64": dict(shape=(1, 4, 9, 7), K=3, i64=True, lit="none", G=1),
    "c5-u8": dict(shape=(1, 5, 12, 16), K=6, i64=False, lit="cut", G=1),                        # the runtime-C form
    "c16-i64": dict(shape=(2, 16, 6, 10), K=64, i64=True, lit="none", G=2),
    # more images than partial rows: one workgroup per image, which walks both trips of it (the second holds one pixel)
    "strided-trips": dict(shape=(1100, 2, 1, 2049), K=1, i64=False, lit="sparse", G=1),
}


def _acc_kernel_cases():
    cases = {accum_kernel(ct, i64): [] for ct in range(REG_CLASSES + 1) for i64 in (False, True)}
    cases["finish_kernel"] = []
    for name, c in sorted(ACC_CASES.items()):
        cases[accum_kernel(class_form(c["shape"][1]), c["i64"])].append(name)
        cases["finish_kernel"].append(name)
    return cases


APPLY_CASES = {}
for _c in (1, 2, 3, 4, 5, 16):
    APPLY_CASES["apply-c%d-vec" % _c] = dict(shape=(3, _c, 8, 12), offset=0)
    APPLY_CASES["apply-c%d-scalar" % _c] = dict(shape=(2, _c, 7, 9), offset=0)
APPLY_CASES["apply-misaligned"] = dict(shape=(2, 4, 8, 12), offset=1)                               # hw % 4 == 0 on the scalar path
APPLY_CASES["apply-two-trips"] = dict(shape=(5, 3, 32, 40), offset=0)                               # 1600 units: a second, partial trip


def apply_vector_path(name):
    c = APPLY_CASES[name]
    return (c["shape"][2] * c["shape"][3]) % 4 == 0 and c["offset"] == 0


def _kernel_cases():
    cases = _acc_kernel_cases()
    for ct in range(REG_CLASSES + 1):
        for vec in (False, True):
            cases[apply_kernel(ct, vec)] = []
    for name, c in sorted(APPLY_CASES.items()):
        cases[apply_kernel(class_form(c["shape"][1]), apply_vector_path(name))].append(name)
    return cases


KERNEL_CASES = _kernel_cases()
THR = np.float32(10.0)


def acc_inputs(name):
    """seeded inputs of an accumulate case: scores float32 (log-softmax of logits ~ N(0, 3^2), a tenth of the pixels 40 nat apart
    so that expf underflows at beta = 4), truth with values >= C, 255 / negative among them, lit per the case, two non-finite
    scores (a NaN, a +inf) at counting pixels when there are at least 8 pixels, the group of each image, K betas"""
    c = ACC_CASES[name]
    N, C, H, W = c["shape"]
    rs = np.random.RandomState(sum(ord(ch) for ch in name) * 7 + 1)
    z = rs.standard_normal((N, C, H, W)) * 3.0
    far = rs.rand(N, 1, H, W) < 0.1
    z = np.where(far, z * 40.0 / 3.0, z)
    z = z - z.max(1, keepdims=True)
    scores = (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)
    t = rs.randint(0, C, size=(N, H, W)).astype(np.int64)
    bad = rs.rand(N, H, W) < 0.15
    if c["i64"]:
        t = np.where(bad, rs.choice([-1, C, C + 300, -(1 << 40), (1 << 40) + 1], size=(N, H, W)), t)
    else:
        t = np.where(bad, rs.choice([C, 255, min(C + 1, 255)], size=(N, H, W)), t)
    truth = t.astype(np.int64 if c["i64"] else np.uint8)
    if c["lit"] == "none":
        lit = None
    elif c["lit"] == "dark":
        lit = (rs.rand(N, H, W) * 10.0).astype(np.float32)                     # up to the threshold, never above
        lit.reshape(-1)[0] = THR
        lit.reshape(-1)[1] = np.nan
    elif c["lit"] == "sparse":
        lit = (rs.rand(N, H, W) * 10.2).astype(np.float32)                     # two in a hundred above the threshold
        lit[:, 0, -1] = 11.0                                                   # and the one pixel of every second trip
    else:
        lit = (rs.rand(N, H, W) * 40.0).astype(np.float32)                     # three quarters above the threshold
        lit.reshape(-1)[0] = THR
        lit.reshape(-1)[-1] = np.nextafter(THR, np.float32(np.inf))
    if N * H * W >= 8 and c["lit"] != "dark":
        counts = np.ones((N, H, W), bool) if lit is None else lit > THR
        valid = (t >= 0) & (t < C)
        where = np.argwhere(counts & valid)
        (n0, y0, x0), (n1, y1, x1) = where[len(where) // 3], where[2 * len(where) // 3]
        scores[n0, rs.randint(C), y0, x0] = np.nan
        scores[n1, rs.randint(C), y1, x1] = np.inf
    groups = np.array(c.get("groups", tuple(range(N)) if c["G"] == N else (0,) * N), dtype=np.uint8)
    K = c["K"]
    temps = default_temps() if K == 33 else [4.0 ** (2.0 * (k + 0.5) / K - 1.0) for k in range(K)]
    return dict(scores=scores, truth=truth, lit=lit, groups=groups, betas=betas32(temps), G=c["G"], thr=float(THR))


def pixel_terms(l, t, betas):
    """l [M, C] scores, t [M] classes, betas [K] -> (terms [M, K, 3] = NLL, g, h in fp64, their bounds [M, K, 3])"""
    l = np.asarray(l, dtype=np.float64)
    M, C = l.shape
    b = np.asarray(betas, dtype=np.float64)[None, :, None]
    d = (l - l.max(1, keepdims=True))[:, None, :]                             # [M, 1, C]
    z = b * d
    e = np.exp(z)
    S = e.sum(-1)
    p = e / S[..., None]
    L = np.log(S)
    dt = d[np.arange(M), 0, t][:, None]
    zt = b[..., 0] * dt
    nll = L - zt
    mean = (p * d).sum(-1)
    g = mean - dt
    r = d - mean[..., None]
    h = (p * r * r).sum(-1)
    az, ad, ar = np.abs(z), np.abs(d), np.abs(r)
    rS = (p * (LIB + 2 * az)).sum(-1) + (C - 1)
    b_nll = U32 * (rS + LIB * L + 2 * np.abs(zt) + np.abs(nll))
    dA = U32 * (p * ad * (LIB + 2 * az + 2 + (C - 1))).sum(-1)
    dmean = dA + U32 * np.abs(mean) * (rS + 1)
    b_g = dmean + U32 * (np.abs(dt) + np.abs(g))
    dr = U32 * ad + dmean[..., None] + U32 * ar
    b_h = (p * (2 * ar * dr + U32 * r * r * (LIB + 2 * az + 2 + (C - 1)))).sum(-1) + U32 * h * (rS + 1)
    floor = 6 * C * 2.0 ** -149 * (1 + ad.max(-1) ** 2)
    terms = np.stack([nll, g, h], -1)
    bounds = C_ACC * (np.stack([b_nll, b_g, b_h], -1) + floor[..., None])
    return terms, bounds


def accumulate(scores, truth, lit, thr, groups, betas, G, table=None, counters=None, bound=None):
    """-> (table float64 [G, K, 3], counters uint64 [G, 3], bound [G, K, 3]); the three are added to when given"""
    N, C, H, W = scores.shape
    K = len(betas)
    table = np.zeros((G, K, 3)) if table is None else table
    counters = np.zeros((G, 3), dtype=np.uint64) if counters is None else counters
    bound = np.zeros((G, K, 3)) if bound is None else bound
    t = truth.astype(np.int64)
    with np.errstate(invalid="ignore"):
        counts = np.ones((N, H, W), bool) if lit is None else lit > np.float32(thr)
    valid = (t >= 0) & (t < C)
    finite = np.isfinite(scores).all(1)
    for n in range(N):
        g = int(groups[n])
        if g >= G:
            continue
        ok = counts[n] & valid[n] & finite[n]
        counters[g] += np.array([ok.sum(), (counts[n] & ~valid[n]).sum(), (counts[n] & valid[n] & ~finite[n]).sum()], dtype=np.uint64)
        if ok.any():
            terms, b = pixel_terms(scores[n][:, ok].T, t[n][ok], betas)
            m = terms.shape[0]
            table[g] += terms.sum(0)
            bound[g] += b.sum(0) + (m + SLACK) * U64 * np.abs(terms).sum(0)
    return table, counters, bound


def apply(x, betas):
    """x [n, C, H, W] float32, betas [n] -> (fp64 out by the rules of the header (NaN where the rule says the quiet NaN), bound)"""
    x64 = np.asarray(x, dtype=np.float64)
    n, C = x64.shape[:2]
    b = np.asarray(betas, dtype=np.float64).reshape(n, 1, 1, 1)
    with np.errstate(all="ignore"):
        bad = (np.isnan(x64) | (np.isinf(x64) & (x64 > 0))).any(1, keepdims=True)
        m = x64.max(1, keepdims=True)
        gone = np.isinf(m) & (m < 0) & ~bad
        d = np.where(np.isinf(x64) & (x64 < 0), -np.inf, x64 - np.where(np.isfinite(m), m, 0.0))
        z = b * d
        e = np.exp(z)
        S = e.sum(1, keepdims=True)
        L = np.log(S)
        out = z - L
        p = e / S
        zf = np.where(np.isfinite(z), z, 0.0)
        rS = (p * (LIB + 2 * np.abs(zf))).sum(1, keepdims=True) + (C - 1)
        bound = C_ACC * (U32 * (2 * np.abs(zf) + LIB * L + rS + np.abs(np.where(np.isfinite(out), out, 0.0))) + 6 * C * 2.0 ** -149)
        out = np.where(out < -3.4028235677973366e38, -np.inf, out)            # below the fp32 range: the fp32 product overflowed
        out = np.where(gone, -np.inf, np.where(bad, np.nan, out))
        bound = np.where(np.isfinite(out), bound, 0.0)
    return out, bound


# ------------------------------------------------------------------------------------------------------------------------
# the solver
# ------------------------------------------------------------------------------------------------------------------------
def hermite_root(b0, b1, g0, g1, h0, h1):
    """the real root in [b0, b1] of the cubic Hermite interpolant, from its monomial coefficients (numpy.roots)"""
    if g0 == 0.0:
        return b0
    if g1 == 0.0:
        return b1
    w = b1 - b0
    m0, m1 = w * h0, w * h1
    coef = [2 * g0 + m0 - 2 * g1 + m1, -3 * g0 - 2 * m0 + 3 * g1 - m1, m0, g0]
    roots = np.roots(coef)
    real = sorted(float(r.real) for r in roots if abs(r.imag) <= 1e-9 * max(1.0, abs(r.real)) and -1e-12 <= r.real <= 1 + 1e-12)
    assert real, "no root in the interval"
    # bisection finds A root; with h >= 0 at both ends and g0 < 0 < g1 the interpolant has one or three: the tests use data with one
    assert len(real) == 1 or max(real) - min(real) < 1e-9, real
    return b0 + min(max(real[0], 0.0), 1.0) * w


def solve(betas, g, h, counted):
    """(beta, at_edge, empty, interval) by the rule of calibration.solve_group; interval: the (lo, hi) betas of the sign change or None"""
    if int(counted) == 0:
        return 1.0, False, True, None
    order = np.argsort(betas)
    b, gs, hs = np.asarray(betas, float)[order], np.asarray(g, float)[order], np.asarray(h, float)[order]
    zero = np.flatnonzero(gs == 0.0)
    if len(zero):
        return float(b[zero[0]]), False, False, None
    change = np.flatnonzero((gs[:-1] < 0) & (gs[1:] > 0))
    if len(change) == 0:
        return float(b[0] if gs[0] > 0 else b[-1]), True, False, None
    i = int(change[0])
    return hermite_root(b[i], b[i + 1], gs[i], gs[i + 1], hs[i], hs[i + 1]), False, False, (float(b[i]), float(b[i + 1]))


def nll_sum(l, t, beta):
    """the exact NLL sum of scores l [M, C] with truth t at one beta, fp64"""
    z = float(beta) * (np.asarray(l, np.float64) - np.asarray(l, np.float64).max(1, keepdims=True))
    return float((np.log(np.exp(z).sum(1)) - z[np.arange(len(t)), t]).sum())


def drawn_labels(rs, l, T0):
    """labels drawn from softmax(l / T0)"""
    z = np.asarray(l, np.float64) / T0
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    return (rs.rand(len(l), 1) > np.cumsum(p, 1)).sum(1).clip(0, l.shape[1] - 1)
