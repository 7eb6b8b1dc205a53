"""Reference of libubresnet_group.so (include/ubresnet_group.h) in Python / numpy fp64, written from the header: the tile planner,
the ordered fp64 sum of squares of the first launch of ubg_grad_norm (lane by lane, tile by tile, then the tree), the decision
rule of the second launch with the per-segment advance, and the table of cases that tests/test_gpu_group_exact.py runs -- one
entry per kernel compiled into the library, which tests/test_cpu_group.py holds against the library's symbol table.  No GPU and
no torch here.

Acceptance (as tests/opt_ref.py documents it for the ungrouped library): sumsq, norm, the counters and everything a step writes
are equal to the reference bit for bit; `scale` (one fp32 division on the device) is within one fp32 ulp of the numpy fp32
formula and exactly 1.0 where nothing is clipped."""
import math

import numpy as np

# geometry and sizes, as include/ubresnet_group.h states them (tests/test_cpu_group.py holds these against the header)
BLOCK, TILE_UNITS, MAX_GRID, STEP_GRID, CTL_HEAD_BYTES = 256, 1024, 1024, 2048, 80
CTL_BYTES = CTL_HEAD_BYTES + 8 * MAX_GRID
# byte offsets of struct ubg_ctl: those of ubo_ctl
OFFSETS = dict(sumsq=0, norm=8, scale=12, gscale=16, apply=20, clipped=24, bc1=28, sqrt_bc2=32, reserved=36, applied=40,
               skipped=48, clipped_total=56, row=64)

# kernel (normal form of tools/kernel_symbols.py) -> ids of the cases in test_gpu_group_exact.py that launch it
KERNEL_CASES = {
    "group_state_set_kernel": ["state-set", "adam-bits", "sgd-bits"],
    "group_sumsq_kernel": ["norm-exact", "norm-ordered", "inactive", "decide-sequence", "graph-replay"],
    "group_decide_kernel": ["norm-exact", "decide-sequence", "advance", "adam-bits", "sgd-bits"],
    "group_adam_kernel": ["adam-bits", "inactive", "skip", "graph-replay"],
    "group_sgd_kernel": ["sgd-bits", "inactive", "skip"],
}

# the layout of the exact tests: units of 9 segments (one lane, a tile less one, a tile's quarter on either side, one tile, one
# over, a few, two tiles and one, a few), in 3 groups that alternate at the segment boundaries
SEG_UNITS = [1, 255, 256, 257, 1024, 1025, 4, 2049, 3]
SEG_GROUP = [s % 3 for s in range(len(SEG_UNITS))]

# the segment lists of the planner tests: (name, seg_unit0, seg_units)
PLAN_LISTS = [
    ("edges", None, [1, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 1]),
    ("single", None, [5000]),
    ("single-unit", None, [1]),
    ("ones", None, [1] * 300),
    ("layout", None, SEG_UNITS),
    ("gaps", [3, 10, 5000, 9000], [2, 1030, 1024, 1]),
]


def starts(seg_units, first=0):
    """first units of segments laid end to end"""
    out, u = [], first
    for n in seg_units:
        out.append(u)
        u += n
    return out


def plan_tiles(seg_unit0, seg_units):
    """-> [(unit0, units, seg)]: every segment cut into tiles of TILE_UNITS units but for a shorter last one, in segment order"""
    tiles = []
    for s, (u0, n) in enumerate(zip(seg_unit0, seg_units)):
        assert n >= 1 and (s == 0 or u0 >= seg_unit0[s - 1] + seg_units[s - 1])
        k = 0
        while k < n:
            tiles.append((u0 + k, min(TILE_UNITS, n - k), s))
            k += TILE_UNITS
    return tiles


def grid(ntiles):
    return min(ntiles, MAX_GRID)


def ordered_sumsq(g, tiles, active):
    """the first launch of ubg_grad_norm and the sum of its partials.  g: float32 [n]; tiles: plan_tiles(); active: per segment.
    -> (sumsq as a Python float, partials float64 [grid]).  One accumulator per lane that lives across the workgroup's tiles;
    in a tile the lane's units l, l + 256, l + 512, l + 768 and x, y, z, w of each; the tree; the partials in index order."""
    g = np.asarray(g, dtype=np.float32)
    nw = grid(len(tiles))
    acc = np.zeros((nw, BLOCK), dtype=np.float64)
    with np.errstate(all="ignore"):
        for trip in range((len(tiles) + nw - 1) // nw):
            sq = np.zeros((nw, 4, BLOCK, 4), dtype=np.float64)              # [workgroup, unit of the lane, lane, float of the unit]
            for w in range(nw):
                t = trip * nw + w
                if t >= len(tiles) or not active[tiles[t][2]]:
                    continue                                                # + 0.0 leaves an accumulator as it is
                u0, n, _ = tiles[t]
                v = np.zeros(4 * TILE_UNITS, dtype=np.float64)
                v[:4 * n] = g[4 * u0:4 * (u0 + n)]
                sq[w] = (v * v).reshape(4, BLOCK, 4)
            for u in range(4):
                for e in range(4):
                    acc = acc + sq[:, u, :, e]
        s = acc.copy()
        h = BLOCK // 2
        while h > 0:
            s[:, :h] = s[:, :h] + s[:, h:2 * h]
            h //= 2
        partials = s[:, 0].copy()
        total = 0.0
        for v in partials.tolist():
            total += v
    return total, partials


def new_state(nseg, counts=None, table=None):
    """host model of the control block's counters and of state[]"""
    counts = [0] * nseg if counts is None else list(counts)
    segs = []
    for c in counts:
        row = table[min(c, len(table)) - 1] if c > 0 else (np.float32(0), np.float32(0))
        segs.append(dict(applied=int(c), bc1=np.float32(row[0]), sqrt_bc2=np.float32(row[1])))
    return dict(applied=0, skipped=0, clipped_total=0, segs=segs)


def decide(sumsq, grad_scale, max_norm, skip_nonfinite, state, active, table):
    """the second launch of ubg_grad_norm on the host, by the header's rule.  sumsq a Python float (fp64); max_norm < 0 or None:
    no clipping; state from new_state() (updated in place); active per segment; table float32 [len, 2].
    -> dict of the head fields the launch writes"""
    f = np.float32
    max_norm = -1.0 if max_norm is None else max_norm
    with np.errstate(all="ignore"):
        if math.isnan(sumsq):
            root = float("nan")
        elif math.isinf(sumsq):
            root = float("inf")
        else:
            root = math.sqrt(sumsq)
        norm = f(abs(float(f(grad_scale))) * root)
        if max_norm < 0:
            scale = f(1.0)
        else:
            scale = f(np.fmin(f(max_norm) / (norm + f(1e-6)), f(1.0)))        # fminf: a NaN quotient gives 1.0f
        gscale = f(f(grad_scale) * scale)
    apply = not (skip_nonfinite and not math.isfinite(sumsq))
    clipped = bool(apply and scale < 1.0)
    if apply:
        state["applied"] += 1
        state["clipped_total"] += int(clipped)
        for s, on in enumerate(active):
            if on:
                seg = state["segs"][s]
                seg["applied"] += 1
                row = table[min(seg["applied"], len(table)) - 1]
                seg["bc1"], seg["sqrt_bc2"] = f(row[0]), f(row[1])
    else:
        state["skipped"] += 1
    return dict(sumsq=sumsq, norm=norm, scale=scale, gscale=gscale, apply=int(apply), clipped=int(clipped), applied=state["applied"],
                skipped=state["skipped"], clipped_total=state["clipped_total"])


def advance(grad_scale, state, active, table):
    """ubg_advance: the decision with nothing to decide"""
    return decide(0.0, grad_scale, -1.0, False, state, active, table)
