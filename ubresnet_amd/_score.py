"""ctypes binding of libubresnet_score.so (the C ABI in include/ubresnet_score.h): event products scored against a truth image
on the device -- lit-pixel confusion matrices split into clear and interface pixels, a reliability table of the float16
confidence and four tallies, added into an exact integer table.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C

from ._binding import Binding

MAX_CLASSES = 16     # UBQ_MAX_CLASSES
MAX_BINS = 32        # UBQ_MAX_BINS
MAX_RADIUS = 8       # UBQ_MAX_RADIUS
TRUTH_U8, TRUTH_I64 = 0, 1
TILE_H, TILE_W = 32, 128

vp, i32 = C.c_void_p, C.c_int32
BINDING = Binding("UBQ_LIB", "libubresnet_score.so", "ubq", {
    "ubq_table_words": (C.c_int, [i32, i32, i32]),
    "ubq_score_event": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, C.POINTER(C.c_uint16), i32, vp, i32, i32, i32, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def table_words(P: int, Cn: int, bins: int) -> int:
    """words of one table: P * (2*C*C + 6*bins + 4), as ubq_table_words counts them (which refuses what is out of range)"""
    n = lib().ubq_table_words(int(P), int(Cn), int(bins))
    if n < 0:
        check(n, "table_words")
    return n


def edges_array(edges):
    """the bins - 1 half bit patterns as the ctypes array ubq_score_event reads on the host; None for no edges"""
    return (C.c_uint16 * len(edges))(*edges) if len(edges) else None


def score_event(label: int, confidence: int, truth: int, truth_kind: int, Cn: int, fill_label: int, radius: int,
                interface_from: int, edges, bins: int, table: int, P: int, rows: int, cols: int, stream=None):
    """ubq_score_event on raw device addresses; `edges` is what edges_array() returned"""
    check(lib().ubq_score_event(label, confidence, truth, int(truth_kind), int(Cn), int(fill_label), int(radius),
                                int(interface_from), edges, int(bins), table, int(P), int(rows), int(cols), stream), "score_event")
