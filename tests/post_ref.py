"""Float reference of ubp_stitch_products (include/ubresnet_post.h) in numpy, its acceptance rule, and the table of cases that
tests/test_gpu_post_exact.py runs -- one entry per kernel compiled into libubresnet_post.so, which tests/test_cpu_post.py holds
against the library's symbol table.  No GPU and no torch here.

Acceptance (the same for every user): labels and counts equal the reference exactly.  Confidence is bit-equal to the reference
(fp64 exp -> fp32 -> float16), except where the fp64 value of exp lies within NEAR_ULPS fp32 ulps of the midpoint between two
adjacent float16 values: there the neighbouring float16 is accepted too (expf on the device is documented to 1 ulp and the
reference's own rounding to fp32 adds half an ulp; 4 leaves room).  Such near-tie pixels may be at most NEAR_SHARE of a case's
lit pixels -- a condition on the case, not a tolerance.  Edge-value rows are chosen away from midpoints and get no exception."""
import numpy as np

NEAR_ULPS = 4
NEAR_SHARE = 0.005

# kernel (normal form of tools/kernel_symbols.py) -> ids of the cases in test_gpu_post_exact.py that launch it.  The library
# has one kernel: every call of ubp_stitch_products that passes its argument checks launches it.
KERNEL_CASES = {
    "stitch_products_kernel": ["ragged-C3", "ragged-C4", "hand-built", "stacked", "adc-null", "counts-null", "short-view",
                               "edge-values"],
}


def first_argmax(scores):
    """scores [C, ...] -> (label, winning value): start at class 0, replace on a strictly greater value"""
    best = np.zeros(scores.shape[1:], np.int64)
    bv = scores[0].copy()
    for c in range(1, scores.shape[0]):
        upd = scores[c] > bv                      # False for NaN on either side
        bv = np.where(upd, scores[c], bv)
        best = np.where(upd, c, best)
    return best, bv


def confidence_bits(bv):
    """winning log-probabilities (fp32) -> (float16 bits of the reference, the other float16 neighbour's bits, near-tie mask)"""
    with np.errstate(over="ignore", invalid="ignore"):
        e64 = np.exp(bv.astype(np.float64))
        e32 = e64.astype(np.float32)
        h = e32.astype(np.float16)
        h64 = h.astype(np.float64)
        below = h64 <= e64                        # the reference rounded down (or is exact): the other neighbour lies above
        other = np.where(below, np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(-np.inf))).astype(np.float16)
        mid = 0.5 * (h64 + other.astype(np.float64))
        ulp = np.spacing(np.abs(e32)).astype(np.float64)
        near = np.abs(e64 - mid) <= NEAR_ULPS * ulp
    near &= np.isfinite(mid) & np.isfinite(e64)
    return h.view(np.uint16), other.view(np.uint16), near


def reference(logp, C, th, tw, desc, adc, vplanes, thr, label, conf, counts, fill, P, rows, cols):
    """ubp_stitch_products on the host.  logp [ntiles,C,th,tw] f32; desc: 7-tuples; adc [P*vplanes,rows,cols] f32 or None;
    label uint8 / conf uint16 [P,rows,cols] and counts int64 [P,C] (or None) are the buffers' contents BEFORE the call.
    -> dict(label, conf, counts, alt, near, lit): `alt` / `near` the accepted neighbour and the near-tie mask per pixel"""
    label, conf = label.copy(), conf.copy()
    counts = None if counts is None else counts.copy()
    alt = conf.copy()
    near = np.zeros(label.shape, bool)
    litmap = np.zeros(label.shape, bool)
    for t, (p, r0, c0, kr0, kr1, kc0, kc1) in enumerate(desc):
        y1, x1 = min(kr1, rows - r0), min(kc1, cols - c0)
        if y1 <= kr0 or x1 <= kc0:
            continue
        oy, ox = slice(r0 + kr0, r0 + y1), slice(c0 + kc0, c0 + x1)
        if adc is None:
            lit = np.ones((y1 - kr0, x1 - kc0), bool)
        else:
            lit = np.zeros((y1 - kr0, x1 - kc0), bool)
            for v in range(vplanes):
                lit |= adc[p * vplanes + v][oy, ox] > np.float32(thr)
        best, bv = first_argmax(logp[t][:, kr0:y1, kc0:x1])
        h, o, nr = confidence_bits(bv)
        label[p][oy, ox] = np.where(lit, best, fill).astype(np.uint8)
        conf[p][oy, ox] = np.where(lit, h, 0).astype(np.uint16)
        alt[p][oy, ox] = np.where(lit, o, 0).astype(np.uint16)
        near[p][oy, ox] = lit & nr
        litmap[p][oy, ox] = lit
        if counts is not None:
            counts[p] += np.bincount(best[lit], minlength=C)[:C]
    return dict(label=label, conf=conf, counts=counts, alt=alt, near=near, lit=litmap)


def _is_nan16(bits):
    return ((bits & 0x7C00) == 0x7C00) & ((bits & 0x03FF) != 0)


def accept(got_label, got_conf, got_counts, ref, what="", exception=True):
    """assert the acceptance rule of the module docstring; -> share of near-tie pixels among the lit ones"""
    assert np.array_equal(got_label, ref["label"]), "%s: %d labels differ" % (what, int((got_label != ref["label"]).sum()))
    if ref["counts"] is not None:
        assert np.array_equal(got_counts, ref["counts"]), "%s: counts %s, reference %s" % (what, got_counts.tolist(), ref["counts"].tolist())
    nlit = int(ref["lit"].sum())
    share = float(ref["near"].sum()) / max(nlit, 1)
    same = (got_conf == ref["conf"]) | (_is_nan16(got_conf) & _is_nan16(ref["conf"]))
    if exception:
        assert share <= NEAR_SHARE, "%s: %.3f %% of the lit pixels are near-ties of the float16 rounding" % (what, 100 * share)
        same |= ref["near"] & (got_conf == ref["alt"])
    else:
        assert not ref["near"].any(), "%s: an edge value sits at a float16 midpoint" % what
    bad = np.argwhere(~same)
    assert bad.size == 0, "%s: %d confidences differ, first at %s: got 0x%04x, reference 0x%04x" % (
        what, len(bad), tuple(bad[0]), int(got_conf[tuple(bad[0])]), int(ref["conf"][tuple(bad[0])]))
    return share


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def logsoftmax_scores(rs, ntiles, C, th, tw):
    """standard_normal * 3 through an fp64 log-softmax, rounded to fp32"""
    z = rs.standard_normal((ntiles, C, th, tw)) * 3.0
    z = z - z.max(1, keepdims=True)
    return (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)


def adc_view(rs, nplanes, rows, cols, thr=10.0, hi=40.0, lit_share=0.5):
    """uniform ADC with about `lit_share` of the pixels above `thr`, a few exactly at `thr` (not lit) and a few NaN"""
    u = rs.uniform(0.0, 1.0, (nplanes, rows, cols))
    below = rs.uniform(0.0, 1.0, (nplanes, rows, cols)) >= lit_share
    a = np.where(below, u * thr, thr + u * (hi - thr)).astype(np.float32)
    flat = a.reshape(-1)
    idx = rs.choice(flat.size, size=min(12, flat.size), replace=False)
    flat[idx[:len(idx) // 2]] = np.float32(thr)
    flat[idx[len(idx) // 2:]] = np.float32(np.nan)
    return a


def regular_desc(P, row_origins, col_origins, th, tw, rows, cols, keep_windows):
    """descriptors of a regular tiling as deploy.view_tiles builds them (keep_windows = deploy._keep_windows)"""
    rk, ck = keep_windows(row_origins, th, rows), keep_windows(col_origins, tw, cols)
    return [(p, r0, c0, rl - r0, rh - r0, cl - c0, ch - c0)
            for p in range(P) for (r0, (rl, rh)) in zip(row_origins, rk) for (c0, (cl, ch)) in zip(col_origins, ck)]


# hand-placed scores that are not a log-softmax (C = 4): (scores, label, confidence bits or None for NaN)
_NAN, _INF = float("nan"), float("inf")
EDGE_ROWS = [
    ("two-way tie",        [1.0, 1.0, 0.0, -1.0],        0, 0x4170),     # half(e) = 2.71875
    ("C-way tie",          [0.5, 0.5, 0.5, 0.5],         0, 0x3E98),     # half(exp(.5)) = 1.6484375
    ("tie of later ones",  [-2.0, -1.0, -1.0, -3.0],     1, 0x35E3),     # half(exp(-1)) = 0.36791992
    ("NaN in class 0",     [_NAN, 5.0, 1.0, 0.0],        0, None),
    ("NaN in class 1",     [-1.0, _NAN, -0.5, -3.0],     2, 0x38DA),     # half(exp(-.5)) = 0.6064453
    ("-inf everywhere",    [-_INF, -_INF, -_INF, -_INF], 0, 0x0000),
    ("winner 0.0",         [-3.0, 0.0, -2.0, -5.0],      1, 0x3C00),
    ("winner -16.0",       [-20.0, -17.0, -16.0, -30.0], 2, 0x0002),     # 1.125e-7: a float16 subnormal (2 * 2^-24)
    ("winner +12.0",       [12.0, 3.0, 2.0, 1.0],        0, 0x7C00),     # exp(12) = 162754.8 > 65504: +inf
]
EDGE_FILLER = [-1.5, -2.5, -0.25, -3.0]                                   # every other pixel: label 2, half(exp(-.25))
