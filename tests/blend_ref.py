"""Float64 reference of overlap-tile inference (ubresnet_amd/deploy.py margin_tiling, include/ubresnet_blend.h): the tiling with a
margin, the blend weights in float64 and their fp32 log tables, the blend of tiles into a view in fp64, the fp32 edge rules, the
error bound of one blended element, and the table of cases that tests/test_gpu_blend_exact.py runs -- which
tests/test_cpu_blend.py holds against the symbol table of the built library.  numpy only; a helper module for the tests
(imported by name; not a conftest).

The bound reuses tests/tta_ref.py (u = 2^-24, a library call within 2 ulp = 4u relative, an fp32 add within u relative,
FLOOR = 2^-146 for gradual underflow, C_ACC = 1.03 for second-order terms).  Hats are computed values.  A view element starts at
a_0 (exact: -inf from ubv_blend_begin, or what the caller stored) with error E_0 = 0 and meets its covering tiles in order.
Tile j brings x (the tile's fp32 log-probability, exact: the reference starts from the same numbers) and the fp32 table
entries lwr, lwc:

  w^ = fl(lwr + lwc):  u |w|.          v^ = fl(x + w^):  u |v| from the add, and w^'s error arrives unchanged:
      operand(j) = u (|w| + |v|)       (zero where w = -inf: v = -inf exactly).
  a_j = lae(a_(j-1), v).  Both partial derivatives of lae lie in [0, 1], so the errors of a_(j-1) and of v^ move the exact value
      of the step by at most E_(j-1) + operand(j).  The step's own rounding is tta_ref's
      step(d, a_j) = u ((4 + |d|) e / (1 + e) + 4 log1p(e) + |a_j|),  d = |a_(j-1) - v|, e = exp(-d),  plus FLOOR;
      where an operand is -inf (the first tile after ubv_blend_begin, a zero weight) or NaN, or the other is +inf, no rounding
      happens and the step adds nothing.
  E_j = E_(j-1) + operand(j) + step_j (FLOOR in it),    bound = C_ACC * E_last.   There is no final subtraction.

Every d, w, v, a_j is from the fp64 reference.  Derived from the operations as written, never fitted to what the kernel
returns: a ratio above 1 is a finding.
"""
import numpy as np

import tta_ref as T

U32, C_ACC, LIB, FLOOR = T.U32, T.C_ACC, T.LIB, T.FLOOR
BLOCK, MAX_GRID, MAX_TILES, MAX_CLASSES = 256, 2048, 64, 16                # UBV_BLOCK, UBV_MAX_GRID, UBV_MAX_TILES, UBV_MAX_CLASSES
KINDS = ("linear", "hann")
SENTINEL = np.array([0xC2F6E979], np.uint32).view(np.float32)[0]            # about -123.456: what uncovered pixels hold
f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------------
# tiling
# ------------------------------------------------------------------------------------------------------------------------
def axis_origins(n, t, margin):
    if n <= t:
        return [0]
    k = -(-(n - t) // (t - 2 * margin)) + 1
    return sorted(set(int(round(i * ((n - t) / float(k - 1)))) for i in range(k)))


def margin_tiling(rows, cols, th, tw, margin):
    assert 0 <= 4 * margin <= min(th, tw)
    return axis_origins(rows, th, margin), axis_origins(cols, tw, margin)


def keep_windows(origins, t, n):
    """tile i keeps [lo, hi) of the view: the overlaps are split in the middle"""
    out = []
    for i, o in enumerate(origins):
        lo = 0 if i == 0 else (origins[i - 1] + t + o) // 2
        hi = min(n, o + t) if i == len(origins) - 1 else (o + t + origins[i + 1]) // 2
        out.append((lo, hi))
    return out


def view_desc(P, ro, co):
    """{plane, row0, col0} in the order of deploy.view_tiles"""
    return [(p, r0, c0) for p in range(P) for r0 in ro for c0 in co]


# ------------------------------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------------------------------
def axis_gains(origins, t, n, margin, kind):
    """[len(origins), t] float64: the unnormalised weight g of every tile coordinate"""
    R = -(-t // 2) - margin
    u = np.arange(t, dtype=f64)
    out = np.empty((len(origins), t))
    for i, o in enumerate(origins):
        d = np.minimum(u if o > 0 else np.full(t, np.inf), (t - 1 - u) if o + t < n else np.full(t, np.inf))
        g = np.where(d < margin, 0.0, np.minimum(d - margin + 1, R) / R)
        out[i] = np.sin(0.5 * np.pi * g) ** 2 if kind == "hann" else g
    return out


def axis_weights(origins, t, n, margin, kind):
    """[len(origins), t] float64: w_i = g_i / sum_j g_j over the tiles covering the same view coordinate (1 beyond the view)"""
    g = axis_gains(origins, t, n, margin, kind)
    total = np.zeros(n)
    for o, row in zip(origins, g):
        m = min(t, n - o)
        total[o:o + m] += row[:m]
    assert (total > 0).all()
    w = np.ones_like(g)
    for i, o in enumerate(origins):
        m = min(t, n - o)
        w[i, :m] = g[i, :m] / total[o:o + m]
    return w


def log_table(w):
    """float64 weights -> the fp32 table: log(w) rounded once, -inf where w = 0"""
    with np.errstate(divide="ignore"):
        return np.log(w).astype(f32)


def view_tables(P, ro, co, th, tw, rows, cols, margin, kind):
    """(lw_rows [ntiles, th], lw_cols [ntiles, tw]) fp32 in the order of view_desc"""
    lr, lc = log_table(axis_weights(ro, th, rows, margin, kind)), log_table(axis_weights(co, tw, cols, margin, kind))
    return (np.stack([lr[i] for _ in range(P) for i in range(len(ro)) for _ in co]),
            np.stack([lc[j] for _ in range(P) for _ in ro for j in range(len(co))]))


# ------------------------------------------------------------------------------------------------------------------------
# the blend
# ------------------------------------------------------------------------------------------------------------------------
def blend(out0, calls):
    """out0 [P, C, rows, cols] fp32: the buffer before the first call.  calls: [(logp [n, C, th, tw] f32, desc [(plane, row0,
    col0)], lw_rows [n, th] f32, lw_cols [n, tw] f32)].  -> (fp64 result, bound per element (0 where the result is not finite),
    number of covering tiles [P, rows, cols]).  Tile after tile, call after call: per element that is ascending descriptor order."""
    acc = out0.astype(f64)
    err = np.zeros(acc.shape)
    count = np.zeros((acc.shape[0],) + acc.shape[2:], np.int64)
    rows, cols = acc.shape[2:]
    with np.errstate(all="ignore"):
        for logp, desc, lwr, lwc in calls:
            th, tw = logp.shape[2:]
            for t, (p, r0, c0) in enumerate(desc):
                hh, ww = min(th, rows - r0), min(tw, cols - c0)
                sl = (p, slice(None), slice(r0, r0 + hh), slice(c0, c0 + ww))
                w = (lwr[t][:hh, None].astype(f64) + lwc[t][None, :ww].astype(f64))[None]
                v = logp[t][:, :hh, :ww].astype(f64) + w
                a = acc[sl]
                nxt = T.lae64(a, v)
                operand = np.where(np.isfinite(v) & np.isfinite(w), U32 * (np.abs(w) + np.abs(v)), 0.0)
                d = np.abs(a - v)
                live = np.isfinite(d)                              # an operand -inf, +inf or NaN: no rounding happens
                d = np.where(live, d, 0.0)
                e = np.exp(-d)
                step = U32 * ((LIB + d) * e / (1.0 + e) + LIB * np.log1p(e) + np.abs(np.where(live, nxt, 0.0))) + FLOOR
                err[sl] = err[sl] + operand + np.where(live, step, 0.0)
                acc[sl] = nxt
                count[p, r0:r0 + hh, c0:c0 + ww] += 1
    return acc, np.where(np.isfinite(acc), C_ACC * err, 0.0), count


def operand32(logp, lwr, lwc):
    """fl(x + fl(lwr + lwc)) in fp32 for one tile: logp [C, th, tw], lwr [th], lwc [tw]"""
    with np.errstate(all="ignore"):
        w = (lwr[:, None].astype(f32) + lwc[None, :].astype(f32)).astype(f32)
        return (logp.astype(f32) + w[None]).astype(f32)


lae32 = T.lae32                 # the fp32 edge rules are tta_ref's: (-inf, -inf), (-inf, x), (x, x), (+inf, x), NaN


# ------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_blend_exact.py
# ------------------------------------------------------------------------------------------------------------------------
def _grid(P, ro, co, drop=()):
    return [(p, r0, c0) for p in range(P) for r0 in ro for c0 in co if (r0, c0) not in drop]


_WIDE = MAX_GRID * BLOCK * 2 + 8               # floats: two such tiles are MAX_GRID * BLOCK + 4 vector units

# tile, view = (P, rows, cols), C, calls = lists of {plane, row0, col0}; `offset`: every buffer starts one float past a 16-byte
# boundary.  Tiles 5 x 7 in 11 x 17 at rows {0, 3, 6} x cols {0, 5, 10} overlap by 2 in both directions: pixels under 1, 2 and 4
# tiles; without the tile at (6, 10) the pixels (8..10, 12..13) are under none, and the tile at (8, 14) hangs over both edges.
# Tiles 8 x 12 in 16 x 24 at rows {0, 4, 8} x cols {0, 8, 12} likewise (overlaps of 4 rows, 4 and 8 columns; (12, 20..23) under none).
_S = dict(tile=(5, 7), rows=11, cols=17, ro=(0, 3, 6), co=(0, 5, 10), drop=((6, 10),), hang=(8, 14))
_V = dict(tile=(8, 12), rows=16, cols=24, ro=(0, 4, 8), co=(0, 8, 12), drop=((8, 12),), hang=(13, 20))


def _case(g, P, C, split, offset=0, shift=None):
    tiles = _grid(P, g["ro"], g["co"], g["drop"]) + [(P - 1,) + g["hang"]]
    if shift is not None:                       # one column origin that is no multiple of 4
        tiles = [(p, r0, shift if c0 == g["co"][1] else c0) for p, r0, c0 in tiles]
    calls = [tiles] if not split else [tiles[0::2], tiles[1::2]]
    return dict(tile=g["tile"], view=(P, g["rows"], g["cols"]), C=C, calls=calls, offset=offset)


CASES = {
    "scalar-C1": _case(_S, 1, 1, False),
    "scalar-C3-two-calls": _case(_S, 2, 3, True),
    "scalar-C16": _case(_S, 1, 16, False),
    "vector-C1": _case(_V, 1, 1, False),
    "vector-C3-two-calls": _case(_V, 2, 3, True),
    "vector-C16": _case(_V, 1, 16, False),
    "offset-C3": _case(_V, 1, 3, True, offset=1),                   # W % 4 == 0 on the scalar path
    "odd-origin-C3": _case(_V, 1, 3, False, shift=6),               # aligned buffers, a col0 that is no multiple of 4: scalar path
    # the grid-stride loops' second, partial trip: two overlapping one-row tiles; the view's second row is under no tile
    "second-trip": dict(tile=(1, _WIDE), view=(1, 2, _WIDE + _WIDE // 2), C=1, calls=[[(0, 0, 0), (0, 0, _WIDE // 2)]], offset=0),
}


def vector_path(name):
    c = CASES[name]
    return (c["offset"] == 0 and c["tile"][1] % 4 == 0 and c["view"][2] % 4 == 0
            and all(c0 % 4 == 0 for call in c["calls"] for _, _, c0 in call))


def begin_vector_path(name):
    c = CASES[name]
    return c["offset"] == 0 and (c["view"][0] * c["C"] * c["view"][1] * c["view"][2]) % 4 == 0


def units(name, call):
    c = CASES[name]
    th, tw = c["tile"]
    return len(c["calls"][call]) * th * (tw // 4 if vector_path(name) else tw)


def begin_units(name):
    c = CASES[name]
    n = c["view"][0] * c["C"] * c["view"][1] * c["view"][2]
    return n // 4 if begin_vector_path(name) else n


def grid(nunits):
    return min(-(-nunits // BLOCK), MAX_GRID)


def kernel_name(which, vec):
    """normal form of tools/kernel_symbols.py"""
    return "%s<%s>" % (which, "true" if vec else "false")


def _kernel_cases():
    """kernel -> ids of the cases of tests/test_gpu_blend_exact.py that launch it: every case calls ubv_blend_begin on its view
    and ubv_blend_tiles once per call"""
    cases = {kernel_name(k, v): [] for k in ("blend_begin_kernel", "blend_kernel") for v in (False, True)}
    for name in CASES:
        cases[kernel_name("blend_begin_kernel", begin_vector_path(name))].append(name)
        cases[kernel_name("blend_kernel", vector_path(name))].append(name)
    return cases


KERNEL_CASES = _kernel_cases()


def case_inputs(name):
    """-> [(logp, desc, lw_rows, lw_cols)] of the case, seeded by its name.  logp is tta_ref.logsoftmax_rows (every 13th pixel has
    classes 100 nat apart, at places that differ between overlapping tiles).  The log-weights are logs of uniform numbers, except:
    the first tile of the first call has weight one (+0) everywhere, and in every call the second tile's first row (of tiles with
    more than one) and the last tile's last column have weight zero (-inf)."""
    c = CASES[name]
    th, tw = c["tile"]
    Cn = c["C"]
    rs = np.random.RandomState(sum(map(ord, name)) % 65521)
    out = []
    for k, desc in enumerate(c["calls"]):
        n = len(desc)
        logp = T.logsoftmax_rows(rs, (n * Cn, th, tw), classes=Cn if Cn > 1 else 3).reshape(n, Cn, th, tw)
        lwr = np.log(rs.uniform(0.05, 1.0, (n, th))).astype(f32)
        lwc = np.log(rs.uniform(0.05, 1.0, (n, tw))).astype(f32)
        if k == 0:
            lwr[0], lwc[0] = f32(0), f32(0)
        if th > 1:
            lwr[1 % n, 0] = -np.inf
        lwc[n - 1, tw - 1] = -np.inf
        out.append((logp, list(desc), lwr, lwc))
    return out
