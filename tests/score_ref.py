"""The numpy statement of ubq_score_event's rule (include/ubresnet_score.h), integers only, and the inputs and the case table the
GPU module tests/test_gpu_score_exact.py runs.  Nothing here touches a device or the library."""
import numpy as np

TILE_H, TILE_W = 32, 128
MAX_CLASSES, MAX_BINS, MAX_RADIUS = 16, 32, 8
U8, I64 = 0, 1
KIND_DTYPE = {U8: np.uint8, I64: np.int64}
NONE = -1

# compiled kernel -> ids of the cases of tests/test_gpu_score_exact.py that launch it
_IDS = ["grid-C1", "grid-C3", "grid-C16", "one-pixel", "narrow", "contacts", "all-unlit", "all-lit", "misaligned", "values", "many-tiles"]
KERNEL_CASES = {
    "score_kernel<unsigned char>": ["%s-u8" % i for i in _IDS],
    "score_kernel<long long>": ["%s-i64" % i for i in _IDS],
}
KIND_OF_CASE = {c: (U8 if c.endswith("-u8") else I64) for ids in KERNEL_CASES.values() for c in ids}

# the base shapes: two tiles and a ragged one in each direction; 150 columns take the element loads, 152 the 4-pixel loads
BASE_SHAPES = [(2, TILE_H + 5, TILE_W + 22), (2, TILE_H + 5, TILE_W + 24)]
GRID_X = 256                       # workgroups per plane at most: a plane of more tiles has workgroups that walk several
MANY_TILES_SHAPE = (1, 17 * TILE_H + 3, 16 * TILE_W + 5)       # 18 x 17 = 306 tiles: workgroups 0..49 take two
GRID_BINS = [1, 10, 32]
GRID_RADII = [0, 1, 2, 8]
CONF_BITS = [0x0000, 0x0001, 0x03FF, 0x0400, 0x3BFF, 0x3C00, 0x3C01, 0x7BFF, 0x7C00, 0x7E00, 0x8000, 0xBC00]


def words(P, C, bins):
    return P * (2 * C * C + 6 * bins + 4)


def equal_edges(bins):
    """the inner edges of `bins` equal-width bins on [0, 1], rounded to half, as bit patterns"""
    return [int(np.float16(i / float(bins)).view(np.uint16)) for i in range(1, bins)]


def fix(h):
    """the value of the non-negative finite half with bits h, times 2^24, as an integer (uint64)"""
    h = np.asarray(h).astype(np.uint64)
    e, m = h >> np.uint64(10), h & np.uint64(1023)
    return np.where(e == 0, m, (np.uint64(1024) + m) << (np.maximum(e, np.uint64(1)) - np.uint64(1)))


def classes(truth, C):
    """truth (uint8 or int64, any shape) -> int64 class, NONE where the value is no class: the test is on the array's own width"""
    t = np.asarray(truth)
    valid = (t >= 0) & (t < C)
    return np.where(valid, t.astype(np.int64) & 0xFF, NONE)


def interface(cls, lo, radius):
    """the contact rule on [P, rows, cols] classes: a pixel of a class >= lo with a different class >= lo in its window"""
    sig = cls >= lo                                           # (NONE is below every lo)
    if radius <= 0:
        return np.zeros(cls.shape, bool)
    bit = np.where(sig, np.left_shift(1, np.where(sig, cls, 0)), 0).astype(np.int64)
    P, rows, cols = cls.shape
    pad = np.zeros((P, rows + 2 * radius, cols + 2 * radius), np.int64)
    pad[:, radius:radius + rows, radius:radius + cols] = bit
    seen = np.zeros_like(bit)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            seen |= pad[:, dy:dy + rows, dx:dx + cols]
    return sig & ((seen & ~bit) != 0)


def unpack(table, P, C, bins):
    """flat uint64 table -> (conf [P,2,C,C], rel [P,2,bins,3], tally [P,4]) views"""
    t = np.asarray(table).reshape(P, -1)
    cw = 2 * C * C
    return t[:, :cw].reshape(P, 2, C, C), t[:, cw:cw + 6 * bins].reshape(P, 2, bins, 3), t[:, cw + 6 * bins:]


def reference(label, conf, truth, C, fill, radius, lo, edges, table0):
    """-> the table after one ubq_score_event: uint64 [words(P, C, bins)], table0 plus this event; wraps modulo 2^64"""
    P, rows, cols = label.shape
    bins = len(edges) + 1
    table = np.array(table0, dtype=np.uint64).copy().reshape(-1)
    assert table.size == words(P, C, bins)
    cf, rel, tally = unpack(table, P, C, bins)
    cls = classes(truth, C)
    lab = label.astype(np.int64)
    lit = lab != fill
    dark = ~lit & (cls >= 1)
    ignored = lit & ((cls == NONE) | (lab >= C))
    scored = lit & ~ignored
    s = interface(cls, lo, radius).astype(np.int64)
    h = conf.astype(np.int64)
    h = np.where(h == 0x8000, 0, h)
    nonfinite = ((h & 0x8000) != 0) | ((h & 0x7C00) == 0x7C00)
    b = np.zeros(h.shape, np.int64)
    for e in edges:
        b += (e <= h)
    fx = fix(np.where(nonfinite, 0, h))
    one = np.uint64(1)
    with np.errstate(over="ignore"):
        for p in range(P):
            tally[p, 0] += np.uint64(scored[p].sum())
            tally[p, 1] += np.uint64(ignored[p].sum())
            tally[p, 2] += np.uint64(dark[p].sum())
            tally[p, 3] += np.uint64((scored[p] & nonfinite[p]).sum())
            m = scored[p]
            np.add.at(cf[p], (s[p][m], cls[p][m], lab[p][m]), one)
            m = scored[p] & ~nonfinite[p]
            np.add.at(rel[p], (s[p][m], b[p][m], 0), one)
            np.add.at(rel[p], (s[p][m], b[p][m], 1), (lab[p][m] == cls[p][m]).astype(np.uint64))
            np.add.at(rel[p], (s[p][m], b[p][m], 2), fx[p][m])
    return table


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def bad_truths(kind, C):
    """values that are no class; 2^40 + 1 has the low byte of class 1: narrowed before the range check it would be scored"""
    return [C, 255] if kind == U8 else [-1, C, 255, 2 ** 40 + 1]


def make_event(seed, P, rows, cols, C, kind, fill=255, edges=()):
    """-> label uint8, confidence bits uint16, truth: blocks of classes on a background, about a third of the pixels lit, labels
    mostly right, values that are no class in truth and label, and the listed confidence patterns among random ones in [0, 1]"""
    rs = np.random.RandomState(seed)
    coarse = rs.randint(0, C, (P, -(-rows // 3), -(-cols // 5)))
    coarse[rs.uniform(size=coarse.shape) < 0.5] = 0
    truth = np.repeat(np.repeat(coarse, 3, axis=1), 5, axis=2)[:, :rows, :cols].astype(np.int64)
    bad = rs.uniform(size=truth.shape) < 0.04
    truth[bad] = rs.choice(bad_truths(kind, C), int(bad.sum()))
    truth = truth.astype(KIND_DTYPE[kind])
    cls = classes(truth, C)
    lit = rs.uniform(size=truth.shape) < 0.35
    label = np.where(cls >= 0, cls, 0)
    wrong = rs.uniform(size=truth.shape) < 0.2
    label = np.where(wrong, rs.randint(0, C, truth.shape), label)
    high = rs.uniform(size=truth.shape) < 0.03
    label = np.where(high, rs.choice([v for v in (C, 200, 254) if v != fill and v >= C], truth.shape), label)
    label = np.where(lit, label, fill).astype(np.uint8)
    conf = np.float16(rs.uniform(0.0, 1.0, truth.shape)).view(np.uint16).copy()
    pool = list(CONF_BITS) + [v for e in edges for v in (e - 1, e, e + 1)]
    special = rs.uniform(size=truth.shape) < 0.25
    conf[special] = rs.choice(pool, int(special.sum())).astype(np.uint16)
    return label, conf, truth


def prefill(seed, n):
    """a table that already holds counts above 2^32"""
    rs = np.random.RandomState(seed)
    return (rs.randint(1, 1 << 30, n).astype(np.uint64) << np.uint64(8)) + np.uint64(1 << 33)
