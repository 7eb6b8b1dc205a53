"""numpy restatement of libubresnet_crop.so (include/ubresnet_crop.h) and the case table of tests/test_gpu_crops_exact.py.
Integers only: the lit test and the float label rule are compares, the table is counts, the selection is Philox words (det_ref.philox)
and remainders, the gather moves bits.  Every comparison against it is np.array_equal: there is no tolerance in this module or in
the tests that use it.

  counting(...)    the predicate, bool [Q][rows][cols]
  sat(...)         int32 [Q][CR+1][CC+1] from cumulative sums; window_brute(...) counts the pixels of a window one by one
  choose(...)      the table int32 [K][8], try by try as the header states it
  gather(...)      image bits / int64 label / weight bits of the crops and the number of invalid rows

CASES: id -> what the case is; inputs(id) builds its arrays from a seed of the id.  KERNEL_CASES: kernel -> the ids that launch it."""
import zlib

import numpy as np

import det_ref

LANES, MIN_CELL, MAX_CELL, MAX_CELL_COLS, MAX_PLANES, MAX_CROPS, MAX_TRIES, TABLE_FIELDS = 256, 4, 64, 4096, 64, 4096, 64, 8
PHILOX_TAG = 0x43524F50
NONE, U8, I64, F32 = 0, 1, 2, 3
KIND_DTYPE = {U8: np.uint8, I64: np.int64, F32: np.float32}
THR = np.float32(10.0)
NO_LABEL = np.iinfo(np.int64).min
f32, u8, u32, i32, i64 = np.float32, np.uint8, np.uint32, np.int32, np.int64


# ------------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------------
def largest_cell(rows, cols, H, W):
    for g in (64, 32, 16, 8, 4):
        if H % g == 0 and W % g == 0 and (rows - H) % g == 0 and (cols - W) % g == 0:
            return g
    return 0


def geometry(rows, cols, H, W, g):
    """-> dict(CR, CC, NR, NC, hc, wc)"""
    assert g in (4, 8, 16, 32, 64) and H % g == 0 and W % g == 0 and (rows - H) % g == 0 and (cols - W) % g == 0
    return dict(CR=rows // g, CC=cols // g, NR=(rows - H) // g + 1, NC=(cols - W) // g + 1, hc=H // g, wc=W // g)


# ------------------------------------------------------------------------------------------------------------------------
# the predicate
# ------------------------------------------------------------------------------------------------------------------------
def convert_labels(label, offset):
    """int64 array of the converted labels of a uint8 / int64 / float32 array"""
    label = np.asarray(label)
    if label.dtype == np.uint8:
        return label.astype(i64) + i64(offset)
    if label.dtype == np.int64:
        return (label.view(np.uint64) + np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF)).view(i64)          # wraps
    assert label.dtype == np.float32
    with np.errstate(invalid="ignore"):
        ok = np.abs(label) < f32(2147483648.0)                      # NaN fails
        t = np.where(ok, np.trunc(np.where(ok, label, f32(0))), 0).astype(i64)
    return np.where(ok, t + i64(offset), i64(NO_LABEL))


def label_counts(L, mask):
    L = np.asarray(L, dtype=i64)
    inr = (L >= 0) & (L < 32)
    return inr & (((np.uint64(mask) >> np.where(inr, L, 0).astype(np.uint64)) & np.uint64(1)) != 0)


def counting(image, label, offset, mask, stacked, thr):
    """bool [Q][rows][cols]; label None: no class mask"""
    with np.errstate(invalid="ignore"):
        lit = image > f32(thr)
    if stacked:
        lit = lit.any(axis=0, keepdims=True)
    if label is not None:
        ok = label_counts(convert_labels(label, offset), mask)
        lit = lit & (ok[None] if stacked else ok)
    return lit


def sat(count, g):
    Q, rows, cols = count.shape
    cells = count.reshape(Q, rows // g, g, cols // g, g).sum(axis=(2, 4), dtype=np.int64)
    s = np.zeros((Q, rows // g + 1, cols // g + 1), np.int64)
    s[:, 1:, 1:] = cells.cumsum(axis=1).cumsum(axis=2)
    assert s.max(initial=0) < 2 ** 31
    return s.astype(i32)


def window_brute(count, q, r0, c0, H, W):
    return int(count[q, r0:r0 + H, c0:c0 + W].sum())


def window(s, geo, q, i, j):
    return int(s[q, i + geo["hc"], j + geo["wc"]]) - int(s[q, i, j + geo["wc"]]) - int(s[q, i + geo["hc"], j]) + int(s[q, i, j])


# ------------------------------------------------------------------------------------------------------------------------
# the selection
# ------------------------------------------------------------------------------------------------------------------------
def choose(s, geo, g, planes, K, T, min_lit, seed, number, flip_rows, flip_cols):
    """int32 [K][8].  planes: the eligible list (None: all count planes of s, in order)"""
    planes = list(range(s.shape[0])) if planes is None else list(planes)
    table = np.zeros((K, TABLE_FIELDS), i32)
    lo, hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for k in range(K):
        w = [v.reshape(-1) for v in det_ref.philox(lo, hi, number, k, np.arange(T), PHILOX_TAG)]
        best, best_n, accepted = None, -1, 0
        for t in range(T):
            plane = planes[int(w[0][t]) % len(planes)]
            i, j = int(w[1][t]) % geo["NR"], int(w[2][t]) % geo["NC"]
            n = window(s, geo, plane, i, j)
            accepted = int(n >= min_lit)
            if accepted or n > best_n:
                best_n = n
                best = [plane, i * g, j * g, n, t, 0, int(w[3][t]) & 1 & int(bool(flip_rows)), (int(w[3][t]) >> 1) & 1 & int(bool(flip_cols))]
            if accepted:
                break
        best[5] = accepted
        table[k] = best
    return table


# ------------------------------------------------------------------------------------------------------------------------
# the gather
# ------------------------------------------------------------------------------------------------------------------------
def row_is_valid(row, stacked, P, rows, cols, H, W):
    plane, r0, c0, fr, fc = int(row[0]), int(row[1]), int(row[2]), int(row[6]), int(row[7])
    return 0 <= plane < (1 if stacked else P) and 0 <= r0 <= rows - H and 0 <= c0 <= cols - W and fr in (0, 1) and fc in (0, 1)


def gather(image, label, offset, weight, stacked, table, H, W):
    """image fp32 [P][rows][cols]; label [P][rows][cols] or, stacked, [rows][cols]; weight fp32 of label's shape or None
    -> (image bits uint32 [K][C][H][W], label int64 [K][H][W], weight bits uint32 [K][H][W], invalid rows)"""
    P, rows, cols = image.shape
    K, C = len(table), (P if stacked else 1)
    bits = np.ascontiguousarray(image).view(u32)
    L = convert_labels(label, offset)
    wb = None if weight is None else np.ascontiguousarray(weight).view(u32)
    oi, ol, ow = np.zeros((K, C, H, W), u32), np.zeros((K, H, W), i64), np.zeros((K, H, W), u32)
    bad = 0
    for k, row in enumerate(table):
        if not row_is_valid(row, stacked, P, rows, cols, H, W):
            bad += 1
            continue
        plane, r0, c0, fr, fc = int(row[0]), int(row[1]), int(row[2]), int(row[6]), int(row[7])
        ys = r0 + (np.arange(H)[::-1] if fr else np.arange(H))
        xs = c0 + (np.arange(W)[::-1] if fc else np.arange(W))
        sel = np.ix_(ys, xs)
        oi[k] = bits[:, ys][:, :, xs] if stacked else bits[plane][sel][None]
        ol[k] = L[sel] if stacked else L[plane][sel]
        ow[k] = 0x3F800000 if wb is None else (wb[sel] if stacked else wb[plane][sel])
    return oi, ol, ow, bad


# ------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------
_BASE = dict(P=3, rows=48, cols=80, H=16, W=32, K=8, T=3, min_lit=0, seed=0, number=0, stacked=False, kind=U8, offset=0, mask=None,
             planes=None, flip_rows=True, flip_cols=True, thr=float(THR), weight=True, shift=0, content="random", table="chosen", status0=0)


def _case(**kw):
    c = dict(_BASE)
    c.update(kw)
    return c


# shift: floats between the 16-byte boundary and the first element of every view-sized input and every output
CASES = {
    "branch": _case(min_lit=256, seed=18, number=2, content="branch", kind=I64),
    "one-position": _case(P=1, rows=16, cols=32, K=5, min_lit=3, seed=3),
    "g4-tails": _case(P=2, rows=20, cols=36, H=8, W=12, K=9, T=4, min_lit=20, seed=5, kind=F32),
    "g64": _case(P=1, rows=128, cols=192, H=64, W=128, K=4, T=2, min_lit=700, seed=6),
    "wide-scan": _case(P=2, rows=8, cols=1040, H=4, W=16, K=8, T=3, min_lit=12, seed=4),       # 260 cells per row: four waves and two trips of the row scan
    "unaligned": _case(shift=1, K=6, min_lit=60, seed=7, kind=F32, mask=0b0110),
    "unaligned-i64": _case(shift=1, K=4, seed=8, kind=I64, mask=0b0010, rows=32, cols=68, H=16, W=36),
    "stacked": _case(stacked=True, K=7, min_lit=120, seed=9, kind=U8, mask=0b0110),
    "stacked-f32": _case(stacked=True, K=3, seed=10, kind=F32, weight=False),
    "label-u8": _case(kind=U8, offset=-1, mask=0b0011, content="labels", seed=11),
    "label-i64": _case(kind=I64, offset=-1, mask=0b0011, content="labels", seed=12),
    "label-f32-edges": _case(kind=F32, offset=-1, mask=0b0011, content="labels", seed=13),
    "class-mask": _case(kind=I64, mask=(1 << 31) | 0b0100, content="labels", min_lit=40, seed=14),
    "no-mask-no-weight": _case(mask=None, weight=False, K=4, seed=15),
    "lit-rule": _case(content="rule", P=1, K=4, min_lit=50, seed=16),
    "k1-t1": _case(K=1, T=1, seed=17, min_lit=10 ** 6),
    "k257": _case(K=257, T=2, rows=32, cols=48, H=16, W=16, P=2, min_lit=30, seed=19),
    "t64": _case(K=3, T=64, min_lit=10 ** 6, seed=20),
    "switches-off": _case(flip_rows=False, flip_cols=False, seed=21, K=16),
    "switches-on": _case(flip_rows=True, flip_cols=True, seed=21, K=16),
    "rows-only": _case(flip_rows=True, flip_cols=False, seed=21, K=16),
    "planes-list": _case(planes=[2, 0], seed=22, K=16, min_lit=10),
    "own-table": _case(table="own", status0=(1 << 40) + 5, kind=F32, seed=23, K=12),
    "own-table-stacked": _case(table="own", stacked=True, status0=0, kind=U8, seed=24, K=12),
    "all-lit": _case(content="all", P=2, K=4, min_lit=512, seed=25),
    "all-dark": _case(content="dark", P=2, K=4, min_lit=1, seed=26),
    "other-number": _case(min_lit=256, seed=18, number=3, content="branch", kind=I64),
    "seed-hi": _case(seed=(5 << 32) | 18, number=2, min_lit=20, K=6),
}

_CHOSEN = [k for k, c in CASES.items() if c["table"] == "chosen"]
KERNEL_CASES = {
    "count_rows_kernel": _CHOSEN,
    "sum_columns_kernel": _CHOSEN,
    "choose_kernel": _CHOSEN,
    "gather_kernel": list(CASES),
}

EDGE_BITS = np.array([0x80000000, 0x00000001, 0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00000000], u32)
# float labels that the rule must take apart: NaN, -0.0, fractions toward zero, 2^31 and beyond, the infinities, the largest float
# below 2^31, a subnormal; then what they convert to with offset -1
EDGE_LABELS = np.array([np.nan, -0.0, 3.9, -1.5, 2147483648.0, -2147483648.0, np.inf, -np.inf, 2147483520.0, 1e-40, 1.0, 2.0, 32.9, 33.0], f32)
EDGE_LABELS_MINUS_1 = [NO_LABEL, -1, 2, -2, NO_LABEL, NO_LABEL, NO_LABEL, NO_LABEL, 2147483519, -1, 0, 1, 31, 32]
INT_LABELS = np.array([0, 1, 2, 3, 31, 32, 33, 255, -1, -2, 2 ** 40, -2 ** 63, 2 ** 63 - 1], i64)


def rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def inputs(name):
    """dict(image, label, weight (None: NULL), table (the caller's own, or None), + the case's fields, g, geo, Q)"""
    c, rs = dict(CASES[name]), rng(name)
    P, rows, cols, H, W = c["P"], c["rows"], c["cols"], c["H"], c["W"]
    lshape = (rows, cols) if c["stacked"] else (P, rows, cols)
    content = c["content"]
    thr = f32(c["thr"])
    if content == "branch":
        image = np.zeros((P, rows, cols), f32)
        image[0, :16, :32] = 20.0
        image[1, 47, 79] = 20.0
    elif content == "all":
        image = np.full((P, rows, cols), 11.0, f32)
    elif content == "dark":
        image = np.full((P, rows, cols), thr, f32)
    elif content == "rule":
        vals = np.array([thr, np.nextafter(thr, f32(np.inf)), np.nextafter(thr, f32(-np.inf)), np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0,
                         11.0, 9.0, 3.0e38, -3.0e38], f32)
        image = vals[rs.randint(0, len(vals), (P, rows, cols))]
        with np.errstate(invalid="ignore"):
            assert (vals > thr).tolist() == [False, True, False, False, False, True, False, False, False, True, False, True, False]
    else:
        image = np.where(rs.uniform(size=(P, rows, cols)) < 0.15, thr + rs.uniform(0.5, 90.0, (P, rows, cols)),
                         thr - rs.uniform(0.0, 12.0, (P, rows, cols))).astype(f32)
        flat = image.reshape(-1).view(u32)
        flat[rs.choice(flat.size, len(EDGE_BITS), replace=False)] = EDGE_BITS       # bits a float copy could lose
    dtype = KIND_DTYPE[c["kind"]]
    if content == "labels":
        pool = EDGE_LABELS if c["kind"] == F32 else (INT_LABELS if c["kind"] == I64 else np.array([0, 1, 2, 3, 31, 32, 33, 255], u8))
        label = pool[rs.randint(0, len(pool), lshape)].astype(dtype)
        image = np.where(rs.uniform(size=(P, rows, cols)) < 0.6, f32(50.0), f32(0.0)).astype(f32)
    else:
        label = rs.randint(0, 4, lshape).astype(dtype)
    weight = None
    if c["weight"]:
        weight = rs.uniform(0.0, 10.0, lshape).astype(f32)
        wf = weight.reshape(-1).view(u32)
        wf[rs.choice(wf.size, len(EDGE_BITS), replace=False)] = EDGE_BITS
    g = largest_cell(rows, cols, H, W)
    table = None
    if c["table"] == "own":
        K = c["K"]
        # in-range rows at offsets that are no multiple of any cell, every flip; then one row bad in each field
        table = np.zeros((K, TABLE_FIELDS), i32)
        table[:, 0] = rs.randint(0, 1 if c["stacked"] else P, K)
        table[:, 1], table[:, 2] = rs.randint(0, rows - H + 1, K), rs.randint(0, cols - W + 1, K)
        table[:, 3:6] = rs.randint(-5, 5, (K, 3))                       # lit, try, accepted are not read
        table[:, 6], table[:, 7] = np.arange(K) & 1, (np.arange(K) >> 1) & 1
        table[0, 1:3] = (rows - H, cols - W)                            # the last position
        table[1, 1:3] = (1, 3)
        table[2, 0] = 1 if c["stacked"] else P                         # plane too large
        table[3, 0] = -1
        table[4, 1] = rows - H + 1
        table[5, 1] = -1
        table[6, 2] = cols - W + 1
        table[7, 2] = -2147483648
        table[8, 6] = 2
        table[9, 7] = -1
        table[10, 1] = 2147483647
    c.update(image=image, label=label, weight=weight, table=table, g=g, geo=geometry(rows, cols, H, W, g), Q=1 if c["stacked"] else P,
             own=table is not None)
    return c


def reference(a):
    """everything the three calls leave behind for inputs(): dict(sat, table, image, label, weight, status)"""
    mask_label = a["label"] if a["mask"] is not None else None
    count = counting(a["image"], mask_label, a["offset"], a["mask"] or 0, a["stacked"], a["thr"])
    s = sat(count, a["g"])
    if a["own"]:
        table = a["table"]
    else:
        table = choose(s, a["geo"], a["g"], a["planes"], a["K"], a["T"], a["min_lit"], a["seed"], a["number"], a["flip_rows"], a["flip_cols"])
    oi, ol, ow, bad = gather(a["image"], a["label"], a["offset"], a["weight"], a["stacked"], table, a["H"], a["W"])
    return dict(count=count, sat=s, table=table, image=oi, label=ol, weight=ow, status=a["status0"] + bad, bad=bad)
