"""numpy references of the three calls of libubresnet_sparse.so (include/ubresnet_sparse.h) and the case table of
tests/test_gpu_sparse_exact.py.  The calls only move data, so a reference is the rule written down once more and every comparison
is np.array_equal on bit views: there is no tolerance in this module or in the tests that use it.

  scatter_view / expand: the entries used are the first min(count, n) (n where count is None); entry i is valid iff its index is
      in range and above its raw predecessor's; invalid entries are not written and counted into status.  `named` marks the
      elements that any used in-range entry names: with status changed those, and only those, are unspecified.
  compact: lit iff adc is None or any of the pixel's vplanes values is > thr (NaN is not); the lit pixels in ascending index
      order into the first min(total, capacity) entries, the rest untouched, count = total.

CASES: id -> what the case is; case_inputs(id) builds its arrays from a seed of the id.  B is the pixel block and S the scan width
of the plan (csrc/ubr_sparse_plan.h): the images are 1, B - 1, B, B + 1 pixels, exactly S and S + 1 blocks, and small ones with
cols in {1, 3, 61, 67} so that no row is 16-byte aligned.  KERNEL_CASES: kernel -> the ids that launch it."""
import zlib

import numpy as np

LANES, LANE_PIXELS, PIXEL_BLOCK, SCAN_WIDTH, MAX_GRID = 256, 4, 1024, 1024, 4096
B, S = PIXEL_BLOCK, SCAN_WIDTH
THR = np.float32(10.0)
f32, u8, u16, u32, i32 = np.float32, np.uint8, np.uint16, np.uint32, np.int32


# ------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------
def used_entries(n, count):
    return n if count is None else min(int(count), n)


def valid_entries(index, m, pixels):
    """bool [m]: in range and above the raw predecessor"""
    idx = index[:m].astype(np.int64)
    ok = (idx >= 0) & (idx < pixels)
    if m > 1:
        ok[1:] &= idx[1:] > idx[:-1]
    return ok


def named_elements(index, m, pixels):
    idx = index[:m].astype(np.int64)
    named = np.zeros(pixels, bool)
    named[idx[(idx >= 0) & (idx < pixels)]] = True
    return named


def scatter_view(index, value_bits, count, pixels, status0):
    """-> (view bits uint32 [pixels], status, named)"""
    m = used_entries(len(index), count)
    ok = valid_entries(index, m, pixels)
    view = np.zeros(pixels, u32)
    view[index[:m][ok]] = value_bits[:m][ok]
    return view, int(status0) + int((~ok).sum()), named_elements(index, m, pixels)


def expand(index, label, conf_bits, count, fill_label, pixels, status0):
    """-> (label uint8 [pixels], confidence bits uint16 [pixels], status, named)"""
    m = used_entries(len(index), count)
    ok = valid_entries(index, m, pixels)
    out_l = np.full(pixels, fill_label, u8)
    out_c = np.zeros(pixels, u16)
    out_l[index[:m][ok]] = label[:m][ok]
    out_c[index[:m][ok]] = conf_bits[:m][ok]
    return out_l, out_c, int(status0) + int((~ok).sum()), named_elements(index, m, pixels)


def lit_mask(adc, vplanes, thr, P, rows, cols):
    """bool [P*rows*cols]; adc [P*vplanes, rows, cols] float32 or None"""
    if adc is None:
        return np.ones(P * rows * cols, bool)
    with np.errstate(invalid="ignore"):
        above = adc.reshape(P, vplanes, rows * cols) > f32(thr)          # NaN > thr is False
    return above.any(axis=1).reshape(-1)


def compact(label, conf_bits, adc, vplanes, thr, P, rows, cols, out_index, out_label, out_conf):
    """the three output arrays (their length is the capacity) are updated in place; -> total"""
    lit = np.flatnonzero(lit_mask(adc, vplanes, thr, P, rows, cols))
    k = min(len(lit), len(out_index))
    out_index[:k] = lit[:k].astype(i32)
    out_label[:k] = label.reshape(-1)[lit[:k]]
    out_conf[:k] = conf_bits.reshape(-1)[lit[:k]]
    return len(lit)


# ------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------
IMG_1, IMG_BM1, IMG_B, IMG_BP1 = (1, 1, 1), (1, 341, 3), (1, 1024, 1), (1, 1025, 1)
IMG_61, IMG_67, IMG_STACK = (3, 37, 61), (3, 29, 67), (1, 37, 61)
IMG_S, IMG_SP1 = (1, S * B, 1), (3, 5217, 67)                  # exactly S blocks; S + 1 blocks, the largest case
IMG_FILL = (1, 62603, 67)                                      # its fp32 view is more 16-byte units than one trip of the fill's grid

# compact: image, vplanes (0: adc is NULL), occupancy, capacity ("total", "total-1", 1), offset of adc in floats
# scatter / expand: image, entries, count (None, "small", "large"), status0, offset of the outputs in elements
CASES = {
    "c-1px-lit": dict(call="compact", image=IMG_1, vplanes=1, occ="all", cap="total", offset=0),
    "c-1px-dark": dict(call="compact", image=IMG_1, vplanes=1, occ="dark", cap="total", offset=0),
    "c-Bm1-checker": dict(call="compact", image=IMG_BM1, vplanes=1, occ="checker", cap="total", offset=0),
    "c-B-random": dict(call="compact", image=IMG_B, vplanes=1, occ="random", cap="total", offset=0),
    "c-Bp1-last": dict(call="compact", image=IMG_BP1, vplanes=1, occ="last", cap="total", offset=0),
    "c-first": dict(call="compact", image=IMG_61, vplanes=1, occ="first", cap="total", offset=0),
    "c-all-lit": dict(call="compact", image=IMG_67, vplanes=1, occ="all", cap="total", offset=0),
    "c-all-dark": dict(call="compact", image=IMG_67, vplanes=1, occ="dark", cap="total", offset=0),
    "c-null-adc": dict(call="compact", image=IMG_61, vplanes=0, occ="all", cap="total", offset=0),
    "c-per-wave": dict(call="compact", image=IMG_61, vplanes=1, occ="wave", cap="total", offset=0),
    "c-stacked": dict(call="compact", image=IMG_STACK, vplanes=3, occ="random30", cap="total", offset=0),
    "c-lit-rule": dict(call="compact", image=IMG_67, vplanes=1, occ="rule", cap="total", offset=0),
    "c-unaligned": dict(call="compact", image=IMG_B, vplanes=1, occ="random30", cap="total", offset=1),
    "c-S-blocks": dict(call="compact", image=IMG_S, vplanes=1, occ="blocks", cap="total", offset=0),
    "c-Sp1-random": dict(call="compact", image=IMG_SP1, vplanes=1, occ="random", cap="total", offset=0),
    "c-cap-short": dict(call="compact", image=IMG_61, vplanes=1, occ="random30", cap="total-1", offset=0),
    "c-cap-1": dict(call="compact", image=IMG_BM1, vplanes=1, occ="checker", cap=1, offset=0),
    "s-empty": dict(call="scatter", image=IMG_67, entries="none", count=None, status0=0, offset=0),
    "s-ends": dict(call="scatter", image=IMG_BM1, entries="ends", count=None, status0=0, offset=1),
    "s-random": dict(call="scatter", image=IMG_61, entries="random", count=None, status0=5, offset=0),
    "s-count-small": dict(call="scatter", image=IMG_61, entries="random", count="small", status0=0, offset=0),
    "s-count-large": dict(call="scatter", image=IMG_61, entries="random", count="large", status0=0, offset=0),
    "s-invalid": dict(call="scatter", image=IMG_67, entries="invalid", count=None, status0=(1 << 40) + 3, offset=0),
    "s-stride": dict(call="scatter", image=IMG_SP1, entries="every", count=None, status0=0, offset=0),
    "s-fill-stride": dict(call="scatter", image=IMG_FILL, entries="ends", count=None, status0=0, offset=0),
    "e-empty": dict(call="expand", image=IMG_67, entries="none", count=None, status0=0, offset=0),
    "e-ends": dict(call="expand", image=IMG_BM1, entries="ends", count=None, status0=0, offset=3),
    "e-random": dict(call="expand", image=IMG_61, entries="random", count="small", status0=7, offset=0),
    "e-count-large": dict(call="expand", image=IMG_61, entries="random", count="large", status0=0, offset=0),
    "e-invalid": dict(call="expand", image=IMG_67, entries="invalid", count=None, status0=9, offset=0),
    "e-stride": dict(call="expand", image=IMG_SP1, entries="every", count=None, status0=0, offset=0),
}

_COMPACT = [k for k, c in CASES.items() if c["call"] == "compact"]
_SCATTER = [k for k, c in CASES.items() if c["call"] == "scatter"]
_EXPAND = [k for k, c in CASES.items() if c["call"] == "expand"]
KERNEL_CASES = {
    "count_kernel": _COMPACT,
    "scan_kernel": _COMPACT,
    "write_kernel": _COMPACT,
    "fill_kernel": _SCATTER + _EXPAND,
    "scatter_kernel<false>": [k for k in _SCATTER if CASES[k]["entries"] != "none"],
    "scatter_kernel<true>": [k for k in _EXPAND if CASES[k]["entries"] != "none"],
}

# values whose bits a float copy could lose: -0.0, the least subnormal, a NaN with a payload, a negative quiet NaN, the infinities
EDGE_BITS = np.array([0x80000000, 0x00000001, 0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00000000], u32)


def rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def pixels_of(image):
    return image[0] * image[1] * image[2]


def occupancy(occ, image, rs):
    """the lit mask a compact case asks for, bool [pixels]"""
    n = pixels_of(image)
    q = np.arange(n)
    if occ == "all":
        return np.ones(n, bool)
    if occ == "dark":
        return np.zeros(n, bool)
    if occ == "first":
        return q == 0
    if occ == "last":
        return q == n - 1
    if occ == "checker":
        P, rows, cols = image
        r, c = (q // cols) % rows, q % cols
        return (r + c) % 2 == 0
    if occ == "wave":                                            # one lit pixel among the 256 of every wave, at a moving place
        return q % 256 == (q // 256 * 37) % 256
    if occ == "blocks":                                          # pixel blocks alternate full and empty
        return (q // PIXEL_BLOCK) % 2 == 0
    if occ in ("random", "random30"):
        return rs.uniform(size=n) < (0.013 if occ == "random" else 0.3)
    raise KeyError(occ)


def compact_inputs(name):
    """dict(label, conf, adc (None: NULL), vplanes, thr, image, lit, capacity, offset)"""
    c, rs = CASES[name], rng(name)
    P, rows, cols = c["image"]
    n = pixels_of(c["image"])
    label = rs.randint(0, 256, n).astype(u8)
    conf = rs.randint(0, 1 << 16, n).astype(u16)
    vplanes = c["vplanes"]
    if vplanes == 0:
        adc, lit = None, np.ones(n, bool)
    elif c["occ"] == "rule":
        # threshold ties, the next float above and below, NaNs, infinities, zeros, among ordinary values on both sides
        vals = np.array([THR, np.nextafter(THR, f32(np.inf)), np.nextafter(THR, f32(-np.inf)), np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0,
                         11.0, 9.0, 3.0e38, -3.0e38], f32)
        adc = vals[rs.randint(0, len(vals), n)].reshape(P, rows, cols)
        lit = lit_mask(adc, 1, THR, P, rows, cols)
        want = np.zeros(len(vals), bool)
        want[[1, 5, 9, 11]] = True                               # what is lit, by hand: nextafter above, +inf, 11, 3e38
        with np.errstate(invalid="ignore"):
            assert np.array_equal(lit_mask(vals.reshape(1, 1, -1), 1, THR, 1, 1, len(vals)), want)
    else:
        want = occupancy(c["occ"], c["image"], rs)
        above = (THR + rs.uniform(0.5, 50.0, (P, vplanes, rows * cols))).astype(f32)
        below = (THR - rs.uniform(0.0, 20.0, (P, vplanes, rows * cols))).astype(f32)
        pick = rs.uniform(size=(P, vplanes, rows * cols)) < 0.5  # which of a lit pixel's planes are above: at least one
        pick[:, rs.randint(0, vplanes, 1)[0]] |= ~pick.any(axis=1)
        adc = np.where(pick & want.reshape(P, 1, rows * cols), above, below).reshape(P * vplanes, rows, cols)
        lit = lit_mask(adc, vplanes, THR, P, rows, cols)
        assert np.array_equal(lit, want)
    total = int(lit.sum())
    cap = {"total": max(total, 1), "total-1": total - 1}.get(c["cap"], c["cap"])
    assert cap >= 1
    return dict(label=label, conf=conf, adc=adc, vplanes=max(vplanes, 1), thr=float(THR), image=c["image"], lit=lit, total=total,
                capacity=cap, offset=c["offset"])


def list_inputs(name):
    """dict(index, value (fp32 bits), label, conf, count (None or an int), status0, image, offset, fill_label) of a scatter or
    expand case; value serves the scatter, label and conf the expand"""
    c, rs = CASES[name], rng(name)
    n = pixels_of(c["image"])
    kind = c["entries"]
    if kind == "none":
        index = np.zeros(0, i32)
    elif kind == "ends":
        index = np.array(sorted(set([0, 1, n // 2, n - 2, n - 1]) & set(range(n))), i32)
    elif kind == "every":
        index = np.arange(n, dtype=i32)
    elif kind == "random":
        index = np.flatnonzero(rs.uniform(size=n) < 0.3).astype(i32)
    elif kind == "invalid":
        # out of range low and high, an equal neighbour, a descending pair, and a valid entry after each of them
        index = np.array([-1, 0, 5, 5, 9, 7, 8, 200, 100, n - 1, n, n + 7, -2147483648, 2147483647, 300, n - 1], i32)
    else:
        raise KeyError(kind)
    m = len(index)
    value = rs.randint(0, 1 << 32, m, dtype=np.uint64).astype(u32)
    value[:min(m, len(EDGE_BITS))] = EDGE_BITS[:min(m, len(EDGE_BITS))]
    label = rs.randint(0, 256, m).astype(u8)
    conf = rs.randint(0, 1 << 16, m).astype(u16)
    conf[:min(m, 4)] = np.array([0x8000, 0x0001, 0x7E01, 0x7C00], u16)[:min(m, 4)]       # -0, least subnormal, NaN, inf as halves
    count = {None: None, "small": m // 2, "large": m + 1000}[c["count"]]
    return dict(index=index, value=value, label=label, conf=conf, count=count, status0=c["status0"], image=c["image"], offset=c["offset"],
                fill_label=255 if name != "e-random" else 7)
