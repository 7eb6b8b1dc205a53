"""ctypes binding of libubresnet_blend.so (the C ABI in include/ubresnet_blend.h): blended stitching of overlapping tiles in
whole-view inference on the device -- every tile is added, with a weight per tile row and per tile column, into a view-sized
buffer that ends as the log of the weighted mean of the covering tiles' probabilities -- and the float64 rule of those weights.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch or numpy, so the argument checks of the library and the weights can be
exercised on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C
import math

from ._binding import Binding

BLOCK = 256          # UBV_BLOCK
MAX_GRID = 2048      # UBV_MAX_GRID
MAX_TILES = 64       # UBV_MAX_TILES
MAX_CLASSES = 16     # UBV_MAX_CLASSES
KINDS = ("linear", "hann")

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
BINDING = Binding("UBV_LIB", "libubresnet_blend.so", "ubv", {
    "ubv_blend_begin": (C.c_int, [vp, i64, vp]),
    "ubv_blend_tiles": (C.c_int, [vp, i32, i32, i32, C.POINTER(i32), i32, vp, vp, vp, i32, i32, i32, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def check_kind(blend):
    """None (off) or one of KINDS; anything else is a ValueError"""
    if blend is not None and (not isinstance(blend, str) or blend not in KINDS):
        raise ValueError("blend must be None or one of %s (got %r)" % (list(KINDS), blend))
    return blend


def axis_gains(origins, t: int, n: int, margin: int, kind: str):
    """the unnormalised weights g of every tile along one axis of length n: [len(origins)][t] floats.  For tile coordinate u of a
    tile at origin o: d = the distance to the nearer tile edge that is not the view's own edge (infinite if both are), g = 0 where
    d < margin, else min(d - margin + 1, R) / R with R = ceil(t / 2) - margin; "hann" takes sin^2(pi / 2 * g)."""
    R = -(-t // 2) - margin
    if R < 1:
        raise ValueError("blend: margin=%d leaves no ramp in a tile side of %d" % (margin, t))
    out = []
    for o in origins:
        row = []
        for u in range(t):
            d = min(u if o > 0 else math.inf, t - 1 - u if o + t < n else math.inf)
            g = 0.0 if d < margin else min(d - margin + 1, R) / R
            row.append(math.sin(0.5 * math.pi * g) ** 2 if kind == "hann" else g)
        out.append(row)
    return out


def axis_log_weights(origins, t: int, n: int, margin: int, kind: str):
    """[len(origins)][t] float64: log(g_i / sum_j g_j) over the tiles j that cover the same view coordinate, -inf where g_i = 0,
    exactly +0 where one tile stands alone; 0 for tile coordinates beyond the view (never read).  A view coordinate that no tile
    weights is a ValueError: the tiling does not give the margin its overlaps."""
    check_kind(kind)
    g = axis_gains(origins, t, n, margin, kind)
    total = [0.0] * n
    for o, row in zip(origins, g):
        for u in range(min(t, n - o)):
            total[o + u] += row[u]
    if min(total) <= 0.0:
        raise ValueError("blend: view coordinate %d of %d has no weight with margin=%d" % (total.index(min(total)), n, margin))
    out = []
    for o, row in zip(origins, g):
        out.append([(math.log(row[u] / total[o + u]) if row[u] > 0.0 else -math.inf) if o + u < n else 0.0 for u in range(t)])
    return out


def desc3(tiles):
    """{plane, row0, col0} of every tile (the first three fields of deploy.view_tiles' descriptors) as the int32 array
    ubv_blend_tiles reads on the host"""
    flat = [int(v) for t in tiles for v in t[:3]]
    return (i32 * len(flat))(*flat)


def blend_begin(out: int, nelem: int, stream=None):
    """ubv_blend_begin on a raw device address: -inf in every element"""
    check(lib().ubv_blend_begin(out, int(nelem), stream), "blend_begin")


def blend_tiles(logp: int, Cn: int, th: int, tw: int, desc, n: int, lw_rows: int, lw_cols: int, out: int, P: int, rows: int,
                cols: int, stream=None):
    """ubv_blend_tiles on raw device addresses; `desc` is what desc3() returned"""
    check(lib().ubv_blend_tiles(logp, int(Cn), int(th), int(tw), desc, int(n), lw_rows, lw_cols, out, int(P), int(rows), int(cols),
                                stream), "blend_tiles")
