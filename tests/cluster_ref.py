"""The numpy reference of libubresnet_cluster.so (include/ubresnet_cluster.h): union-find over the lit pixels of a class map --
every adjacent pair hooks the larger root under the smaller, pointer jumping flattens, until no pair disagrees -- then the
numbering in ascending root order and the table from np.add.at / np.minimum.at / np.maximum.at.  Everything is integer: the GPU
tests compare bit for bit.  The views and patterns of tests/test_gpu_cluster_exact.py are built here, so that the CPU module can
hold them (and this reference) against a brute-force flood fill."""
import numpy as np

TILE_H, TILE_W = 32, 64                  # UBI_TILE_H, UBI_TILE_W (test_cpu_cluster.py holds them against the header)
PIXEL_BLOCK = 1024
TABLE_FIXED = 8
FILL = 255
T_H, T_W = TILE_H, TILE_W
VIEWS = {
    "1x1x1": (1, 1, 1),
    "row": (1, 1, T_W + 1),
    "col": (1, T_H + 1, 1),
    "four-tiles": (2, 2 * T_H + 3, 2 * T_W + 5),
    "one-short": (3, T_H - 1, T_W - 1),
}


def lit_mask(label, C, fill):
    return (label != fill) & (label < C)


def _edges(label, lit, connectivity, by_class):
    """the adjacent pairs (a, b), a < b, as two arrays of flat pixel indices"""
    P, rows, cols = label.shape
    idx = np.arange(label.size, dtype=np.int64).reshape(label.shape)
    shifts = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    ea, eb = [], []
    for dy, dx in shifts:
        ya, yb = slice(0, rows - dy), slice(dy, rows)
        if dx >= 0:
            xa, xb = slice(0, cols - dx), slice(dx, cols)
        else:
            xa, xb = slice(-dx, cols), slice(0, cols + dx)
        ok = lit[:, ya, xa] & lit[:, yb, xb]
        if by_class:
            ok &= label[:, ya, xa] == label[:, yb, xb]
        ea.append(idx[:, ya, xa][ok])
        eb.append(idx[:, yb, xb][ok])
    return np.concatenate(ea), np.concatenate(eb)


def roots(label, C, fill=FILL, connectivity=8, by_class=False):
    """-> (root int32 [P,rows,cols], foreign): the smallest pixel index of the pixel's cluster, -1 where it is not lit"""
    assert label.dtype == np.uint8 and label.ndim == 3 and connectivity in (4, 8)
    lit = lit_mask(label, C, fill)
    par = np.where(lit.reshape(-1), np.arange(label.size, dtype=np.int64), -1)
    ea, eb = _edges(label, lit, connectivity, by_class)
    while ea.size:
        ra, rb = par[ea], par[eb]
        differ = ra != rb
        ea, eb, ra, rb = ea[differ], eb[differ], ra[differ], rb[differ]
        if not ea.size:
            break
        np.minimum.at(par, np.maximum(ra, rb), np.minimum(ra, rb))       # hook the larger root under the smaller
        live = par >= 0
        while True:                                                      # pointer jumping until every pixel names a root
            nxt = par.copy()
            nxt[live] = par[par[live]]
            if (nxt == par).all():
                break
            par = nxt
    foreign = int(((label != fill) & (label >= C)).sum())
    return par.astype(np.int32).reshape(label.shape), foreign


def fix(h):
    """(fix(h) of include/ubresnet_score.h as int64, nonfinite) for uint16 half bits"""
    h = h.astype(np.int64)
    h = np.where(h == 0x8000, 0, h)
    bad = ((h & 0x8000) != 0) | ((h & 0x7C00) == 0x7C00)
    e, m = (h >> 10) & 31, h & 1023
    val = np.where(e == 0, m, (1024 + m) << np.maximum(e - 1, 0))
    return np.where(bad, 0, val), bad


def tabulate(label, conf_bits, root, C):
    """-> (ids int32 like root, table int64 [count, 8 + C], count)"""
    P, rows, cols = label.shape
    flat = root.reshape(-1).astype(np.int64)
    lit = flat >= 0
    heads = np.flatnonzero(flat == np.arange(flat.size))
    q = np.flatnonzero(lit)
    k = np.searchsorted(heads, flat[q])
    ids = np.full(flat.size, -1, np.int32)
    ids[q] = k
    table = np.zeros((heads.size, TABLE_FIXED + C), np.int64)
    table[:, 0] = heads
    table[:, 2], table[:, 4] = rows, cols
    y, x = q % (rows * cols) // cols, q % cols
    val, bad = fix(conf_bits.reshape(-1)[q])
    np.add.at(table[:, 1], k, 1)
    np.minimum.at(table[:, 2], k, y)
    np.maximum.at(table[:, 3], k, y)
    np.minimum.at(table[:, 4], k, x)
    np.maximum.at(table[:, 5], k, x)
    np.add.at(table[:, 6], k, val)
    np.add.at(table[:, 7], k, bad.astype(np.int64))
    np.add.at(table, (k, TABLE_FIXED + label.reshape(-1)[q].astype(np.int64)), 1)
    return ids.reshape(root.shape), table, int(heads.size)


def flood_fill(label, C, fill=FILL, connectivity=8, by_class=False):
    """brute force for tiny views: a stack-based fill from every unvisited lit pixel in index order -> root"""
    P, rows, cols = label.shape
    lit = lit_mask(label, C, fill)
    root = np.full(label.shape, -1, np.int32)
    steps = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and (connectivity == 8 or dy == 0 or dx == 0)]
    for p in range(P):
        for y in range(rows):
            for x in range(cols):
                if not lit[p, y, x] or root[p, y, x] >= 0:
                    continue
                head = (p * rows + y) * cols + x
                root[p, y, x] = head
                stack = [(y, x)]
                while stack:
                    cy, cx = stack.pop()
                    for dy, dx in steps:
                        ny, nx = cy + dy, cx + dx
                        if 0 <= ny < rows and 0 <= nx < cols and lit[p, ny, nx] and root[p, ny, nx] < 0 and \
                                (not by_class or label[p, ny, nx] == label[p, cy, cx]):
                            root[p, ny, nx] = head
                            stack.append((ny, nx))
    return root


# ------------------------------------------------------------------------------------------------------------------------
# patterns: name -> f(P, rows, cols) -> uint8 label; C = 4 classes, FILL elsewhere
# ------------------------------------------------------------------------------------------------------------------------
C4 = 4


def _blank(P, rows, cols):
    return np.full((P, rows, cols), FILL, np.uint8)


def _grid(P, rows, cols):
    return np.meshgrid(np.arange(P), np.arange(rows), np.arange(cols), indexing="ij")


def p_empty(P, rows, cols):
    return _blank(P, rows, cols)


def p_all(P, rows, cols):
    p, y, x = _grid(P, rows, cols)
    return ((p + y // 7 + x // 5) % C4).astype(np.uint8)


def p_checker(P, rows, cols):
    p, y, x = _grid(P, rows, cols)
    return np.where((y + x) % 2 == 0, 1, FILL).astype(np.uint8)


def p_diagonal(P, rows, cols):
    """a diagonal that wraps over the columns, so that it passes through every tile column in every tile row"""
    p, y, x = _grid(P, rows, cols)
    return np.where((x - y - 3 * p) % max(cols, 2) == 0, 2, FILL).astype(np.uint8)


def p_serpentine(P, rows, cols):
    """every other row lit, joined to the next lit row at alternating ends: one cluster per plane, whose root (0, 0) is reached
    from the last row only through every tile"""
    lab = _blank(P, rows, cols)
    lab[:, 0::2, :] = 1
    for y in range(1, rows, 2):
        lab[:, y, cols - 1 if (y // 2) % 2 == 0 else 0] = 3
    return lab


def p_u(P, rows, cols):
    """two arms from row 0 down columns 1 and 3 that share every tile they cross and join only in the last row"""
    lab = _blank(P, rows, cols)
    if cols >= 4 and rows >= 2:
        lab[:, :, 1] = 0
        lab[:, :, 3] = 0
        lab[:, rows - 1, 1:4] = 0
    else:
        lab[:, :, 0] = 0
    return lab


def p_corner(P, rows, cols):
    """two pixels that touch only diagonally across the corner of four tiles (or of the view's last pixels), both ways"""
    lab = _blank(P, rows, cols)
    y, x = min(T_H, rows - 1), min(T_W, cols - 1)
    lab[:, max(y - 1, 0), max(x - 1, 0)] = 1
    lab[:, y, x] = 1
    if P > 1 and y >= 1 and x >= 1:
        lab[1:] = FILL
        lab[1:, y - 1, x] = 2
        lab[1:, y, x - 1] = 2
    return lab


def p_row_wrap(P, rows, cols):
    """the last pixel of a row against the first of the next"""
    lab = _blank(P, rows, cols)
    for y in range(rows - 1):
        lab[:, y, cols - 1] = 1
        lab[:, y + 1, 0] = 1
    lab[:, 0, cols - 1] = 1
    if cols <= 2:                                                # the two columns would touch: keep every other row
        lab[:, 1::2, :] = FILL
    return lab


def p_plane_wrap(P, rows, cols):
    """the last pixel of a plane against the first of the next"""
    lab = _blank(P, rows, cols)
    lab[:, rows - 1, cols - 1] = 1
    lab[:, 0, 0] = 1
    return lab


def p_stripes(P, rows, cols):
    p, y, x = _grid(P, rows, cols)
    return ((x // 3 + p) % C4).astype(np.uint8)


def p_foreign(P, rows, cols):
    """lit blocks cut by lines of labels that are no class: 4 (= C), 200 and 254 -- and the fill"""
    p, y, x = _grid(P, rows, cols)
    lab = ((y // 4 + x // 4) % C4).astype(np.uint8)
    lab[(x % 9) == 4] = 4
    lab[(y % 11) == 5] = 200
    lab[(x + y) % 13 == 0] = 254
    lab[(x * 3 + y) % 17 == 0] = FILL
    return lab


def _random(percent):
    def make(P, rows, cols):
        rng = np.random.default_rng(1000 + percent + P * rows * cols)
        lab = rng.integers(0, C4, (P, rows, cols)).astype(np.uint8)
        lab[rng.random((P, rows, cols)) * 100 >= percent] = FILL
        return lab
    make.__doc__ = "a random field, %d %% lit" % percent
    return make


PATTERNS = {
    "empty": p_empty, "all-lit": p_all, "checker": p_checker, "diagonal": p_diagonal, "serpentine": p_serpentine, "u": p_u,
    "corner": p_corner, "row-wrap": p_row_wrap, "plane-wrap": p_plane_wrap, "stripes": p_stripes, "foreign": p_foreign,
    "random-1": _random(1), "random-41": _random(41), "random-59": _random(59), "random-90": _random(90),
}
MODES = ((8, False), (4, False), (8, True), (4, True))         # (connectivity, by_class)


def confidence_bits(shape, seed=7):
    """half bits: mostly finite values in 0..1, with a sprinkle of subnormals, 0x8000, negatives, inf and NaN"""
    rng = np.random.default_rng(seed + int(np.prod(shape)))
    bits = rng.random(shape).astype(np.float16).view(np.uint16).copy()
    edge = np.array([0x0001, 0x03FF, 0x8000, 0x8001, 0xBC00, 0x7C00, 0xFC00, 0x7E00, 0xFFFF, 0x7BFF, 0x0000, 0x3C00], np.uint16)
    pick = rng.random(shape) < 0.08
    bits[pick] = edge[rng.integers(0, len(edge), int(pick.sum()))]
    return bits


def reference(label, conf_bits, C=C4, fill=FILL, connectivity=8, by_class=False):
    """-> dict(root, ids, table, count, foreign)"""
    root, foreign = roots(label, C, fill, connectivity, by_class)
    ids, table, count = tabulate(label, conf_bits, root, C)
    return dict(root=root, ids=ids, table=table, count=count, foreign=foreign)
