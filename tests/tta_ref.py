"""Float64 reference of libubresnet_tta.so (include/ubresnet_tta.h): the flip of a stack of planes, the merge of K flipped views of
log-probabilities into the log of their mean probability, the fp32 edge rules, the error bound of one merged element, and the
table of cases that tests/test_gpu_tta_exact.py runs -- which tests/test_cpu_tta.py holds against the symbol table of the built
library.  numpy only; a helper module for the tests (imported by name; not a conftest).

The bound.  u = 2^-24 (kref.U32).  As in tests/loss_ref.py, each library call (expf, log1pf) is taken as within 2 ulp, a relative
error of at most 4u, and each fp32 add or subtract as half an ulp, a relative error of at most u.  Hats are computed values.
One step v = lae(a, x) of ubr_tta.hip, with a^ the running merge (absolute error E on entry) and x a view's fp32 value (exact:
the reference starts from the same fp32 numbers):

  lae(a, x) = log(exp(a) + exp(x)) has the partial derivatives exp(a) / (exp(a) + exp(x)) and its complement, both in [0, 1]:
     the error E of a^ moves the exact value of the step by at most E.
  d^ = fl(lo - hi):  |d| u.        e^ = expf(d^):  relative 4u from the call, |d| u from its argument;  e = exp(d) <= 1.
  l^ = log1pf(e^):   d/de log(1 + e) = 1 / (1 + e), so e's relative error r = (4 + |d|) u arrives as r e / (1 + e) (at most
     r / 2 at e = 1, and |d| e <= 1 / e^1 keeps the second part below 0.37 u), and the call adds 4u l, l = log1p(e) <= ln 2.
  v^ = fl(hi + l^):  u |v|.
     step(d, v) = u ((4 + |d|) e / (1 + e) + 4 l + |v|).
  hi == lo:  hi + (float)M_LN2, the constant within u ln 2 (covered by 4u l) and the add u |v|: the same expression bounds it.
     The branch is taken on computed values: where the exact a differs from x by less than E the exact lae differs from
     hi + ln 2 by less than E, which the first line covers.
  lo == -inf: v = hi, no operation;  a NaN operand gives NaN.  No error.
  Gradual underflow: expf's 2 ulp, log1pf's 2 ulp on a subnormal value and the add's half are each counted at the spacing
     2^-149 instead: FLOOR = 2^-146 per step covers 4.5 of them.
  After the last view  w^ = fl(v^ - log_k), log_k = fl((float) log K) within u log K:  + u log K + u |w|.

  E_0 = 0;   E_k = E_(k-1) + step(d_k, v_k) + FLOOR  for k = 1 .. K-1;   bound = C_ACC (E_(K-1) + u (log K + |w|))  (K > 1),
  every d_k, v_k, w from the fp64 reference, and C_ACC = 1.03 for the second-order terms as in kref.  K = 1 and view 0 are copies:
  bound 0.  Derived from the operations as written, never fitted to what the kernel returns: a ratio above 1 is a finding.
"""
import numpy as np

U32 = 2.0 ** -24
C_ACC = 1.03
LIB = 4.0                 # relative error of a library call, in units of u: 2 ulp
FLOOR = 2.0 ** -146

BLOCK, UNROLL, MAX_GRID, MAX_VIEWS = 256, 2, 1024, 4          # UBT_BLOCK, UBT_UNROLL, UBT_MAX_GRID, UBT_MAX_VIEWS
TRIP = BLOCK * UNROLL
FLIP_ROWS, FLIP_COLS = 1, 2
LN2_F32 = np.float32(np.log(2.0))

# nplanes x H x W of the flip and merge cases; `offset`: the buffers start one float past a 16-byte boundary
SHAPES = {
    "one": dict(shape=(1, 1, 1), offset=0),                                  # degenerate single element
    "odd": dict(shape=(3, 3, 7), offset=0),                                  # scalar path, odd W
    "vec8": dict(shape=(2, 5, 8), offset=0),                                 # vector path, two vectors per row
    "vec20": dict(shape=(6, 4, 20), offset=0),                               # vector path, row length not a power of two
    "misaligned": dict(shape=(2, 32, 64), offset=1),                         # W % 4 == 0 on the scalar path
    "second-trip": dict(shape=(1, 3, MAX_GRID * BLOCK * 4 + 12), offset=0),  # the grid-stride loop's second, partial trip
}


def vector_path(name):
    s = SHAPES[name]
    return s["shape"][2] % 4 == 0 and s["offset"] == 0


def units(name):
    n, H, W = SHAPES[name]["shape"]
    return n * H * (W // 4 if vector_path(name) else W)


def grid(nunits):
    return min((nunits + TRIP - 1) // TRIP, MAX_GRID)


def kernel_name(flip, vec, merge):
    """normal form of tools/kernel_symbols.py"""
    return "tta_kernel<%d, %s, %s>" % (flip, "true" if vec else "false", "true" if merge else "false")


def view_flips(K, first):
    """the flips of the K views of a merge case: a different one per view, starting at `first`"""
    return [(first + k) % 4 for k in range(K)]


def _kernel_cases():
    """kernel -> ids of the cases of tests/test_gpu_tta_exact.py that launch it.  test_flip[shape-flip] launches the copy form;
    test_merge[shape-K-first] launches the copy form for view 0 and the merge form for the others."""
    cases = {kernel_name(f, v, m): [] for f in range(4) for v in (False, True) for m in (False, True)}
    for name in SHAPES:
        vec = vector_path(name)
        for flip in range(4):
            cases[kernel_name(flip, vec, False)].append("flip[%s-%d]" % (name, flip))
        for K, first in merge_cases(name):
            for k, flip in enumerate(view_flips(K, first)):
                cases[kernel_name(flip, vec, k > 0)].append("merge[%s-%d-%d]" % (name, K, first))
    return cases


# (K, flip of view 0): between them every flip is a first view and a later view on either path
MERGE_CASES = [(1, 0), (1, 3), (2, 1), (2, 2), (3, 2), (4, 0), (4, 3)]


def merge_cases(name):
    """the merge cases of a shape: all of MERGE_CASES, one per K at the large shape (its paths are those of "vec20")"""
    return [(1, 0), (2, 1), (3, 2), (4, 3)] if name == "second-trip" else MERGE_CASES


KERNEL_CASES = _kernel_cases()


def flip_planes(a, flip):
    """a [nplanes, H, W] -> the flipped copy (any dtype: nothing is looked at)"""
    if flip & FLIP_ROWS:
        a = a[:, ::-1, :]
    if flip & FLIP_COLS:
        a = a[:, :, ::-1]
    return np.array(a, order="C", copy=True)                          # (ascontiguousarray keeps a negative stride on a length-1 axis)


def lae64(a, b):
    """log(exp(a) + exp(b)) in fp64 by the rules of the header"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        hi, lo = np.maximum(a, b), np.minimum(a, b)                # NaN if either is
        d = np.where(np.isinf(lo) & (lo < 0), -np.inf, np.where(hi == lo, 0.0, lo - hi))
        out = np.where(np.isinf(lo) & (lo < 0), hi, hi + np.log1p(np.exp(d)))
        return np.where(np.isnan(a) | np.isnan(b), np.nan, out)


def merge(views, flips=None):
    """views: K arrays [nplanes, H, W] as the network wrote them (view k computed on the input flipped by flips[k]; None: none is
    flipped) -> (fp64 log of the mean probability in unflipped coordinates, the bound of the module docstring per element)"""
    K = len(views)
    assert 1 <= K <= MAX_VIEWS
    flips = [0] * K if flips is None else flips
    x = [flip_planes(np.asarray(v), f).astype(np.float64) for v, f in zip(views, flips)]
    acc, err = x[0], np.zeros(x[0].shape)
    if K == 1:
        return acc, err
    with np.errstate(all="ignore"):
        for k in range(1, K):
            nxt = lae64(acc, x[k])
            d = np.abs(acc - x[k])
            live = np.isfinite(d)                                  # lo == -inf, +inf or NaN: no rounding happens
            d = np.where(live, d, 0.0)
            e = np.exp(-d)
            step = U32 * ((LIB + d) * e / (1.0 + e) + LIB * np.log1p(e) + np.abs(np.where(live, nxt, 0.0))) + FLOOR
            err = err + np.where(live, step, 0.0)
            acc = nxt
        out = acc - np.log(float(K))
        err = C_ACC * (err + U32 * (np.log(float(K)) + np.abs(np.where(np.isfinite(out), out, 0.0))))
    return out, np.where(np.isfinite(out), err, 0.0)


def lae32(a, b):
    """the edge rules of lae in fp32, for operands where every branch but the last is exact: (-inf, -inf), (-inf, x), (x, x),
    (+inf, x), NaN.  Pairs that need expf / log1pf come out as NaN-tagged `general` = True."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(all="ignore"):
        hi, lo = np.maximum(a, b), np.minimum(a, b)
        nan = np.isnan(a) | np.isnan(b)
        gone = np.isinf(lo) & (lo < 0)
        same = (hi == lo) & ~gone
        top = np.isinf(hi) & (hi > 0) & ~same & ~gone                # expf(-inf) = 0, log1pf(0) = 0, +inf + 0 = +inf
        out = np.where(gone | top, hi, np.where(same, (hi + LN2_F32).astype(np.float32), np.float32(0))).astype(np.float32)
        out = np.where(nan, np.float32(np.nan), out).astype(np.float32)
    return out, ~(nan | gone | same | top)


def log_views(K):
    return np.float32(np.log(float(K)))


def logsoftmax_rows(rs, shape, sigma=4.0, classes=3, far_every=13):
    """[nplanes, H, W] fp32 log-probabilities: consecutive groups of `classes` planes are the log-softmax over the group of logits
    ~ N(0, sigma^2), computed in fp64 and rounded once (a last incomplete group keeps the first planes of a full one).  Every
    `far_every`-th pixel has logits 100 nat apart instead (0, -100, -200 in a random rotation), so that expf(lo - hi) underflows
    where two views disagree.  Rows wider than 2^16 repeat a block of 2^16 columns: the period does not divide such a W."""
    n, H, W = shape
    Wb = min(W, 1 << 16)
    out = np.empty(shape, dtype=np.float32)
    for p in range(0, n, classes):
        z = rs.standard_normal((classes, H, Wb)) * sigma
        far = (np.arange(H * Wb).reshape(H, Wb) % far_every) == 5
        rot = rs.randint(0, classes, size=(H, Wb))
        for c in range(classes):
            z[c] = np.where(far, -100.0 * ((c + rot) % classes), z[c])
        z = z - z.max(0, keepdims=True)
        lp = (z - np.log(np.exp(z).sum(0, keepdims=True))).astype(np.float32)
        if Wb < W:
            lp = np.tile(lp, (1, 1, -(-W // Wb)))[:, :, :W]
        out[p:p + classes] = lp[:min(classes, n - p)]
    return out
