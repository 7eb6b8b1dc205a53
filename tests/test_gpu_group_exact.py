"""libubresnet_group.so on the device, exactly: the grouped Adam / SGD steps against libubresnet_opt.so's guarded steps run on
each segment's slice, bit for bit; inactive segments untouched and outside the norm; the norm against math.fsum and against
group_ref's ordered emulation; the decision and every segment's counter against group_ref; ubg_advance; graph replay.

The layout used throughout (group_ref.SEG_UNITS): 9 segments of 1, 255, 256, 257, 1024, 1025, 4, 2049 and 3 float4 units, with
a gap of two units that belongs to no segment after the fourth, in 3 groups that alternate at the segment boundaries.

Every case id of group_ref.KERNEL_CASES is claimed by a _case("...") call below; tests/test_cpu_group.py holds the table against
the kernels compiled into the library."""
import math

import numpy as np
import pytest
import torch

import group_ref as R
import kref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _group as G
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _opt as O

CASES = R.KERNEL_CASES
DEV = "cuda"
F32 = torch.float32
f32 = np.float32

GAP_AFTER, GAP = 3, 2
SEG_UNIT0 = R.starts(R.SEG_UNITS[:GAP_AFTER + 1]) + R.starts(R.SEG_UNITS[GAP_AFTER + 1:], sum(R.SEG_UNITS[:GAP_AFTER + 1]) + GAP)
NSEG = len(R.SEG_UNITS)
N = 4 * (SEG_UNIT0[-1] + R.SEG_UNITS[-1])
GROUP_HYPER = [(1e-3, 1e-4), (1e-5, 0.0), (3e-4, 1e-2)]               # (lr, weight_decay) of the 3 groups
COUNTS = [0, 1, 7, 100000, 0, 1, 7, 100000, 2]                        # steps each segment has behind it; 100000 is past the table
ALL = [True] * NSEG


def _case(cid):
    """names the row(s) of group_ref.KERNEL_CASES a test stands for (tests/test_cpu_group.py reads these calls from the syntax tree)"""
    assert any(cid in ids for ids in CASES.values()), "case %r is in no row of group_ref.KERNEL_CASES" % cid


def _seg(s):
    return slice(4 * SEG_UNIT0[s], 4 * (SEG_UNIT0[s] + R.SEG_UNITS[s]))


_tables = {}


def _table(b1=0.9, b2=0.999):
    if (b1, b2) not in _tables:
        host = O.bias_table(b1, b2)
        _tables[(b1, b2)] = (torch.from_numpy(host).to(DEV), host)
    return _tables[(b1, b2)]


class Plan(object):
    """tile table, hyper and state of a segment list on the device, each between two 256-byte margins of 0xA5, and a control
    block likewise"""

    def __init__(self, unit0=None, units=None, hyper=None, active=None, counts=None, table=None):
        self.unit0, self.units = list(SEG_UNIT0 if unit0 is None else unit0), list(R.SEG_UNITS if units is None else units)
        self.nseg = len(self.units)
        self.host_tiles = R.plan_tiles(self.unit0, self.units)
        tiles = G.plan_tiles(self.unit0, self.units)
        assert [(int(t["unit0"]), int(t["units"]), int(t["seg"])) for t in tiles] == self.host_tiles
        self.ntiles = len(tiles)
        self.n = 4 * (self.unit0[-1] + self.units[-1])
        self._full = {}
        self.tiles = self._margined("tiles", torch.from_numpy(tiles.view(np.uint8).copy()))
        self.hyper = self._margined("hyper", torch.zeros(16 * self.nseg, dtype=torch.uint8))
        self.state = self._margined("state", torch.zeros(16 * self.nseg, dtype=torch.uint8))
        self.ctl = self._margined("ctl", torch.zeros(R.CTL_BYTES, dtype=torch.uint8))
        self.table = table or _table()
        self.set_hyper(hyper or [GROUP_HYPER[s % 3] for s in range(self.nseg)], ALL[:1] * self.nseg if active is None else active)
        if counts is not None:
            self.set_counts(counts)

    def _margined(self, name, body):
        full = torch.full((body.numel() + 512,), 0xA5, dtype=torch.uint8, device=DEV)
        full[256:256 + body.numel()].copy_(body)
        self._full[name] = full
        return full[256:256 + body.numel()]

    def set_hyper(self, hyper, active):
        h = np.zeros(self.nseg, dtype=G.HYPER)
        h["lr"], h["weight_decay"], h["active"] = [a for a, _ in hyper], [b for _, b in hyper], [1 if a else 0 for a in active]
        self.hyper.copy_(torch.from_numpy(h.view(np.uint8).copy()))
        self.hyper_host, self.active = h, list(active)

    def set_counts(self, counts):
        dev = torch.tensor(list(counts), dtype=torch.int64, device=DEV)
        G.state_set(self.state.data_ptr(), self.nseg, 0, self.nseg, dev.data_ptr(), self.table[0].data_ptr(), self.table[0].shape[0], L.stream_ptr())
        torch.cuda.synchronize()

    def get_state(self):
        return G.state_get(self.state.data_ptr(), self.nseg, L.stream_ptr())

    def head(self):
        return G.read_ctl(self.ctl[:R.CTL_HEAD_BYTES].cpu().numpy().tobytes())

    def norm(self, g, grad_scale=1.0, max_norm=None, skip=True):
        G.grad_norm(g.data_ptr(), g.numel(), self.tiles.data_ptr(), self.ntiles, self.hyper.data_ptr(), self.state.data_ptr(), self.nseg,
                    grad_scale, max_norm, skip, self.table[0].data_ptr(), self.table[0].shape[0], self.ctl.data_ptr(), L.stream_ptr())

    def advance(self, grad_scale=1.0):
        G.advance(self.hyper.data_ptr(), self.state.data_ptr(), self.nseg, grad_scale, self.table[0].data_ptr(), self.table[0].shape[0],
                  self.ctl.data_ptr(), L.stream_ptr())

    def adam(self, p, g, m, v, b1=0.9, b2=0.999, eps=1e-8):
        G.adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), self.tiles.data_ptr(), self.ntiles,
                    self.hyper.data_ptr(), self.state.data_ptr(), self.nseg, b1, b2, eps, self.ctl.data_ptr(), L.stream_ptr())

    def sgd(self, p, g, buf, momentum, dampening, nesterov):
        G.sgd_step(p.data_ptr(), g.data_ptr(), None if buf is None else buf.data_ptr(), p.numel(), self.tiles.data_ptr(), self.ntiles,
                   self.hyper.data_ptr(), self.state.data_ptr(), self.nseg, momentum, dampening, nesterov, self.ctl.data_ptr(), L.stream_ptr())

    def margins_intact(self):
        for name, full in self._full.items():
            assert bool((full[:256] == 0xA5).all()) and bool((full[-256:] == 0xA5).all()), "wrote outside %s" % name
        assert torch.equal(self.tiles.cpu(), torch.from_numpy(G.plan_tiles(self.unit0, self.units).view(np.uint8).copy())), "the tile table changed"
        assert self.hyper.cpu().numpy().tobytes() == self.hyper_host.tobytes(), "a kernel wrote hyper"


def _margined(t, fill=float("nan")):
    """a copy of t between two 64-element margins -> (full, view)"""
    full = torch.full((t.numel() + 128,), fill, dtype=t.dtype, device=DEV)
    full[64:64 + t.numel()].copy_(t)
    return full, full[64:64 + t.numel()]


def _margins_ok(full, what):
    assert bool(torch.isnan(full[:64]).all()) and bool(torch.isnan(full[-64:]).all()), "%s: wrote outside the buffer" % what


def _edges():
    """signed zeros and subnormals (kref.edge_table's fp32 rows of those classes)"""
    return kref.edge_values(F32, classes=("zero", "f32_subnormal_min", "f32_subnormal", "f32_subnormal_max"))


def _operands(seed, n=None):
    """param, grad, exp_avg, exp_avg_sq from a seeded generator; signed zeros and subnormals at the head of every segment that has
    room and spread over the largest"""
    n = N if n is None else n
    gen = torch.Generator(device="cpu").manual_seed(seed)
    p = torch.randn(n, generator=gen) * 0.1
    g = torch.randn(n, generator=gen) * 1e-2
    m = torch.randn(n, generator=gen) * 1e-3
    v = (torch.randn(n, generator=gen) * 1e-2).square()
    if n == N:
        e = _edges()
        for k, t in enumerate((p, g, m)):
            for s in range(NSEG):
                lo, room = _seg(s).start, 4 * R.SEG_UNITS[s]
                cnt = min(len(e), room)
                t[lo:lo + cnt] = e.roll(k + s)[:cnt]
            lo = _seg(7).start
            t[lo + 1000 + 97 * torch.arange(len(e))] = e.roll(3 * k)
        lo = _seg(7).start
        v[lo + 2000 + 89 * torch.arange(len(e))] = e.abs()                   # exp_avg_sq is never negative
        gap = slice(_seg(GAP_AFTER).stop, _seg(GAP_AFTER + 1).start)
        for t in (p, g, m, v):
            t[gap] = float("nan")                                            # the gap belongs to no segment: never read, never written
    return [t.to(DEV) for t in (p, g, m, v)]


def _write_ubo_head(ctl, **fields):
    h = O.Ctl()
    for k, val in fields.items():
        setattr(h, k, val)
    ctl.zero_()
    ctl[:O.CTL_HEAD_BYTES].copy_(torch.frombuffer(bytearray(bytes(h)), dtype=torch.uint8))


def _row(host_table, count):
    r = host_table[min(count, len(host_table)) - 1]
    return float(r[0]), float(r[1])


def _unchanged(got, before, what):
    assert torch.equal(got.view(torch.int32), before.view(torch.int32)), "%s: bytes changed" % what


# ------------------------------------------------------------------------------------------------------------------------
# counters from a checkpoint
# ------------------------------------------------------------------------------------------------------------------------
def test_state_set_seeds_counts_and_corrections_and_state_get_reads_them():
    _case("state-set")
    pl = Plan(counts=COUNTS)
    _, host = pl.table
    st = pl.get_state()
    assert st["applied"].tolist() == COUNTS
    for s, c in enumerate(COUNTS):
        want = (0.0, 0.0) if c == 0 else _row(host, c)
        assert (float(st["bc1"][s]), float(st["sqrt_bc2"][s])) == want, s
    assert len(host) < 100000 and _row(host, 100000) == (1.0, 1.0)
    # a range in the middle, a negative count stored as zero; the others stay
    dev = torch.tensor([5, -3], dtype=torch.int64, device=DEV)
    G.state_set(pl.state.data_ptr(), NSEG, 3, 2, dev.data_ptr(), pl.table[0].data_ptr(), len(host), L.stream_ptr())
    st = pl.get_state()
    assert st["applied"].tolist() == COUNTS[:3] + [5, 0] + COUNTS[5:]
    assert (float(st["bc1"][3]), float(st["sqrt_bc2"][3])) == _row(host, 5) and (float(st["bc1"][4]), float(st["sqrt_bc2"][4])) == (0.0, 0.0)
    pl.margins_intact()


# ------------------------------------------------------------------------------------------------------------------------
# step bits: the grouped launch against the ungrouped library on each segment's slice
# ------------------------------------------------------------------------------------------------------------------------
def _ubo_ctl():
    return torch.zeros(O.CTL_BYTES, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("grad_scale", [1.0, 0.375])
def test_adam_step_equals_ubo_adam_step_on_every_segment(grad_scale):
    _case("adam-bits")
    pl = Plan(counts=COUNTS)
    _, host = pl.table
    ops = _operands(100)
    mine = [_margined(t) for t in ops]
    ref = [t.clone() for t in ops]
    pl.advance(grad_scale)
    pl.adam(*[v for _, v in mine])
    ctl = _ubo_ctl()
    for s in range(NSEG):
        lr, wd = GROUP_HYPER[s % 3]
        bc1, sbc2 = _row(host, COUNTS[s] + 1)
        _write_ubo_head(ctl, apply=1, scale=1.0, gscale=grad_scale, bc1=bc1, sqrt_bc2=sbc2, applied=COUNTS[s] + 1)
        sl = [t[_seg(s)] for t in ref]
        assert all(x.data_ptr() % 16 == 0 for x in sl)
        O.adam_step(sl[0].data_ptr(), sl[1].data_ptr(), sl[2].data_ptr(), sl[3].data_ptr(), sl[0].numel(), lr, 0.9, 0.999, 1e-8, wd,
                    ctl.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    for (full, got), want, was, nm in zip(mine, ref, ops, ("param", "grad", "exp_avg", "exp_avg_sq")):
        kref.assert_bits(got, want, what="grouped adam, grad_scale %g: %s" % (grad_scale, nm))
        _margins_ok(full, nm)
        if nm != "grad":
            for s in range(NSEG):
                if R.SEG_UNITS[s] >= 4:                                      # (the smallest hold signed zeros and subnormals only)
                    assert not torch.equal(got[_seg(s)], was[_seg(s)]), "segment %d of %s did not move" % (s, nm)
    _unchanged(mine[1][1], ops[1], "grad")
    st = pl.get_state()
    assert st["applied"].tolist() == [c + 1 for c in COUNTS]
    h = pl.head()
    assert (h.apply, h.applied, h.skipped, h.gscale, h.scale, h.norm, h.sumsq) == (1, 1, 0, grad_scale, 1.0, 0.0, 0.0)
    pl.margins_intact()


SGD_SETTINGS = [(0.0, 0.0, 0), (0.9, 0.0, 0), (0.9, 0.0, 1), (0.9, 0.5, 0)]          # plain, momentum, nesterov, dampening


@pytest.mark.parametrize("momentum,dampening,nesterov", SGD_SETTINGS)
def test_sgd_step_equals_ubo_sgd_step_on_every_segment(momentum, dampening, nesterov):
    _case("sgd-bits")
    pl = Plan(counts=COUNTS, table=_table(0.0, 0.0))
    p, g, m, _ = _operands(200 + int(10 * momentum) + nesterov + int(10 * dampening))
    for s in range(NSEG):
        if COUNTS[s] == 0:
            m[_seg(s)] = float("nan")                                       # a segment's first step must not read its buffer
    ops = (p, g, m)
    mine = [_margined(t) for t in ops]
    ref = [t.clone() for t in ops]
    pl.advance(0.5)
    pl.sgd(mine[0][1], mine[1][1], mine[2][1] if momentum else None, momentum, dampening, nesterov)
    ctl = _ubo_ctl()
    for s in range(NSEG):
        lr, wd = GROUP_HYPER[s % 3]
        _write_ubo_head(ctl, apply=1, scale=1.0, gscale=0.5, applied=COUNTS[s] + 1)
        sl = [t[_seg(s)] for t in ref]
        O.sgd_step(sl[0].data_ptr(), sl[1].data_ptr(), sl[2].data_ptr() if momentum else None, sl[0].numel(), lr, momentum, dampening, wd,
                   nesterov, ctl.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    what = "grouped sgd momentum=%g dampening=%g nesterov=%d" % (momentum, dampening, nesterov)
    for (full, got), want, nm in zip(mine, ref, ("param", "grad", "momentum buffer")):
        kref.assert_bits(got, want, what="%s: %s" % (what, nm))
        _margins_ok(full, nm)
    _unchanged(mine[1][1], g, "grad")
    if momentum:
        for s in range(NSEG):
            assert bool(torch.isfinite(mine[2][1][_seg(s)]).all()) and bool(torch.isfinite(mine[0][1][_seg(s)]).all()), s
            assert R.SEG_UNITS[s] < 4 or not torch.equal(mine[2][1][_seg(s)], m[_seg(s)])
    else:
        _unchanged(mine[2][1], m, "momentum buffer without momentum")
    assert not torch.equal(mine[0][1][_seg(7)], p[_seg(7)])
    assert pl.get_state()["applied"].tolist() == [c + 1 for c in COUNTS]
    pl.margins_intact()


# ------------------------------------------------------------------------------------------------------------------------
# inactive segments and skipped steps
# ------------------------------------------------------------------------------------------------------------------------
OFF = (0, 4, 8)                                                               # the first, a middle and the last segment
ACTIVE = [s not in OFF for s in range(NSEG)]


def _sentinel(t, k):
    """a pattern with NaNs of distinct payloads in the inactive segments of t"""
    for s in OFF:
        n = 4 * R.SEG_UNITS[s]
        pat = (torch.arange(n, dtype=torch.int64) * 2654435761 + 12345 * k) % (1 << 22)
        bits = torch.where(torch.arange(n) % 3 == 0, 0x7fc00000 + pat, 0x3f800000 + pat).to(torch.int32)
        t[_seg(s)] = bits.view(F32).to(DEV)


def test_inactive_segments_are_untouched_and_outside_the_norm():
    _case("inactive")
    for kind in ("adam", "sgd"):
        pl = Plan(counts=COUNTS, active=ACTIVE)
        ops = _operands(300)
        ops[1] = kref.exact_operands((N,), F32, density=0.6, seed=31, exp=-3, maxmag=7, device=DEV)      # dyadic: the sum is exact
        for k, t in enumerate(ops):
            _sentinel(t, k)
        for s in OFF:
            ops[1][_seg(s)] = float("nan")                                   # stale gradient bytes of frozen parameters
        ops[1][_seg(GAP_AFTER).stop:_seg(GAP_AFTER + 1).start] = float("inf")
        mine = [_margined(t) for t in ops]
        before_state = pl.get_state()
        pl.norm(mine[1][1], max_norm=None, skip=True)
        if kind == "adam":
            pl.adam(*[v for _, v in mine])
        else:
            pl.sgd(mine[0][1], mine[1][1], mine[2][1], 0.9, 0.0, 0)
        torch.cuda.synchronize()
        h = pl.head()
        want = math.fsum(float(x) * float(x) for s in range(NSEG) if ACTIVE[s] for x in ops[1][_seg(s)].cpu().tolist())
        assert h.apply == 1 and h.skipped == 0 and h.sumsq == want and h.norm == float(f32(math.sqrt(want))), (h.apply, h.sumsq, want)
        st = pl.get_state()
        for s in range(NSEG):
            if ACTIVE[s]:
                assert st["applied"][s] == COUNTS[s] + 1
                assert not torch.equal(mine[0][1][_seg(s)], ops[0][_seg(s)]), "%s: active segment %d did not move" % (kind, s)
            else:
                assert st[s].tobytes() == before_state[s].tobytes(), "the state of inactive segment %d changed" % s
                for (_, got), was, nm in zip(mine, ops, ("param", "grad", "state 1", "state 2")):
                    _unchanged(got[_seg(s)], was[_seg(s)], "%s: %s of inactive segment %d" % (kind, nm, s))
        gap = slice(_seg(GAP_AFTER).stop, _seg(GAP_AFTER + 1).start)
        for (full, got), was, nm in zip(mine, ops, ("param", "grad", "state 1", "state 2")):
            _unchanged(got[gap], was[gap], "%s: %s in the gap" % (kind, nm))
            _margins_ok(full, nm)
        _unchanged(mine[1][1], ops[1], "grad")
        if kind == "sgd":
            _unchanged(mine[3][1], ops[3], "a buffer the sgd step does not take")
        pl.margins_intact()


def test_a_skipped_step_touches_nothing_at_all():
    _case("skip")
    for kind, poison in (("adam", float("inf")), ("sgd", float("nan"))):
        pl = Plan(counts=COUNTS, active=ACTIVE)
        ops = _operands(400)
        ops[1][_seg(5).start + 77] = poison                                  # in an ACTIVE segment
        mine = [_margined(t) for t in ops]
        before_state = pl.get_state()
        pl.norm(mine[1][1], max_norm=1.0, skip=True)
        ctl_before = pl.ctl.clone()
        if kind == "adam":
            pl.adam(*[v for _, v in mine])
        else:
            pl.sgd(mine[0][1], mine[1][1], mine[2][1], 0.9, 0.0, 1)
        torch.cuda.synchronize()
        h = pl.head()
        assert (h.apply, h.applied, h.skipped, h.clipped, h.row[2]) == (0, 0, 1, 0, 0.0) and not math.isfinite(h.sumsq)
        assert pl.get_state().tobytes() == before_state.tobytes(), "a skipped step advanced a counter"
        assert torch.equal(pl.ctl, ctl_before), "a step kernel wrote the control block"
        for (full, got), was, nm in zip(mine, ops, ("param", "grad", "state 1", "state 2")):
            _unchanged(got, was, "%s skipped: %s" % (kind, nm))
            _margins_ok(full, nm)
        pl.margins_intact()


# ------------------------------------------------------------------------------------------------------------------------
# norm
# ------------------------------------------------------------------------------------------------------------------------
_TRIPS_UNITS = [(1, 3, 256, 2, 7)[k % 5] for k in range(2 * R.MAX_GRID + 5)]
# name -> (units of the segments, laid end to end; which are active).  "past-the-grid" is the size the layout of the network's
# gradients resembles (a few workgroups take a second tile); in "three-trips", 2053 small one-tile segments with every seventh
# off, EVERY workgroup takes a second tile and five a third, so a lane's accumulator lives across three tiles
NORM_SIZES = {
    "one-tile": ([1000], [True]),
    "grid-tiles": ([R.MAX_GRID * R.TILE_UNITS], [True]),
    "past-the-grid": ([1025 * R.TILE_UNITS + 37], [True]),
    "three-trips": (_TRIPS_UNITS, [k % 7 != 3 for k in range(len(_TRIPS_UNITS))]),
}


def _norm_plan(size):
    units, active = NORM_SIZES[size]
    return Plan(unit0=R.starts(units), units=units, hyper=[(1e-3, 0.0)] * len(units), active=active)


def test_norm_sizes_are_what_they_claim():
    assert [len(R.plan_tiles(R.starts(u), u)) for u, _ in NORM_SIZES.values()] == [1, R.MAX_GRID, 1026, 2 * R.MAX_GRID + 5]
    assert 4.1e6 < 4 * NORM_SIZES["past-the-grid"][0][0] < 4.3e6
    units, active = NORM_SIZES["three-trips"]
    assert max(units) <= R.TILE_UNITS and len(units) == 2053 and not all(active) and active[0] and active[R.MAX_GRID] and active[2 * R.MAX_GRID]
    assert all(any(active[w + k * R.MAX_GRID] for k in range(2)) for w in range(R.MAX_GRID)), "every workgroup has work"


@pytest.mark.parametrize("size", sorted(NORM_SIZES))
def test_norm_of_dyadic_values_is_the_exact_sum(size):
    _case("norm-exact")
    pl = _norm_plan(size)
    # m * 2^-3, |m| <= 7: every square is a multiple of 2^-6 below 1, any sum of < 2^23 of them is exact in fp64 in any order
    g = kref.exact_operands((pl.n,), F32, density=0.5, seed=len(size), exp=-3, maxmag=7, device=DEV)
    g[-1] = 0.875                                                           # the last element counts
    keep = torch.zeros(pl.n, dtype=torch.bool, device=DEV)
    for u0, n, a in zip(pl.unit0, pl.units, pl.active):
        if a:
            keep[4 * u0:4 * (u0 + n)] = True
    g = torch.where(keep, g, torch.full_like(g, float("nan")))              # stale bytes of inactive segments
    full, gv = _margined(g)
    pl.norm(gv, max_norm=None)
    torch.cuda.synchronize()
    h = pl.head()
    want = math.fsum((g[keep].double().cpu().numpy() ** 2))
    assert want > 0 and h.sumsq == want, (size, h.sumsq, want)
    assert h.norm == float(f32(math.sqrt(want))) and (h.scale, h.gscale, h.apply, h.clipped, h.applied, h.skipped) == (1.0, 1.0, 1, 0, 1, 0)
    assert list(h.row) == [h.norm, 1.0, 1.0, 1.0]
    part = pl.ctl[R.CTL_HEAD_BYTES:].view(torch.float64).cpu()
    grid = R.grid(pl.ntiles)
    assert not bool(part[grid:].any()), "partials past the grid were written"
    s = 0.0
    for v in part[:grid].tolist():
        s += v
    assert s == h.sumsq
    _unchanged(gv, g, "grad")
    _margins_ok(full, "grad")
    assert pl.get_state()["applied"].tolist() == [int(a) for a in pl.active]
    pl.margins_intact()


@pytest.fixture(scope="module")
def general_runs():
    """general (not dyadic) values: the 9-segment layout with three segments off, and every size of NORM_SIZES; two runs each"""
    out = {}
    for name in ["layout"] + sorted(NORM_SIZES):
        blocks = []
        for _ in range(2):
            pl = Plan(active=ACTIVE) if name == "layout" else _norm_plan(name)
            gen = torch.Generator(device="cpu").manual_seed(77)
            g = torch.randn(pl.n, generator=gen) * torch.exp(4 * torch.randn(pl.n, generator=gen))     # magnitudes over many binades
            for u0, n, a in zip(pl.unit0, pl.units, pl.active):
                if not a:
                    g[4 * u0:4 * (u0 + n)] = float("nan")
            gd = g.to(DEV)
            pl.norm(gd, max_norm=None)
            torch.cuda.synchronize()
            blocks.append(pl)
        out[name] = dict(g=g.numpy(), plans=blocks, active=pl.active)
    return out


def test_norm_of_general_values_is_the_ordered_sum_bit_for_bit(general_runs):
    _case("norm-ordered")
    for name, r in general_runs.items():
        pl = r["plans"][0]
        want, partials = R.ordered_sumsq(r["g"], pl.host_tiles, r["active"])
        h = pl.head()
        assert math.isfinite(want) and want > 0
        got = pl.ctl[R.CTL_HEAD_BYTES:].view(torch.float64).cpu().numpy()[:len(partials)]
        assert got.tobytes() == partials.tobytes(), "%s: %d partials differ from the ordered emulation" % (name, int((got != partials).sum()))
        assert np.float64(h.sumsq).tobytes() == np.float64(want).tobytes(), (name, h.sumsq, want)
        assert h.norm == float(f32(math.sqrt(want)))
        a, b = r["plans"]
        assert torch.equal(a.ctl, b.ctl), "%s: two runs differ in the control block" % name
        assert a.get_state().tobytes() == b.get_state().tobytes()
        pl.margins_intact()
    three = R.ordered_sumsq(general_runs["three-trips"]["g"], general_runs["three-trips"]["plans"][0].host_tiles, general_runs["three-trips"]["active"])[1]
    assert len(three) == R.MAX_GRID and len(general_runs["three-trips"]["plans"][0].host_tiles) > 2 * R.MAX_GRID


# ------------------------------------------------------------------------------------------------------------------------
# decision and counters
# ------------------------------------------------------------------------------------------------------------------------
def _ulps32(a, b):
    a, b = f32(a), f32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def _compare(pl, d, model, gs, what):
    h = pl.head()
    if math.isnan(d["sumsq"]):
        assert math.isnan(h.sumsq), what
    else:
        assert h.sumsq == d["sumsq"], "%s: sumsq %r, expected %r" % (what, h.sumsq, d["sumsq"])
    kref.assert_bits(torch.tensor([h.norm], dtype=F32), torch.tensor([float(d["norm"])], dtype=F32), what=what + " norm")
    if math.isnan(float(d["scale"])):
        assert math.isnan(h.scale), what
    else:
        assert _ulps32(h.scale, d["scale"]) <= 1, "%s: scale %r, formula %r" % (what, h.scale, float(d["scale"]))
    if d["scale"] == 1.0:
        assert h.scale == 1.0, what
    kref.assert_bits(torch.tensor([h.gscale], dtype=F32), torch.tensor([float(f32(gs) * f32(h.scale))], dtype=F32), what=what + " gscale")
    for k in ("apply", "clipped", "applied", "skipped", "clipped_total"):
        assert getattr(h, k) == d[k], "%s: %s is %r, expected %r" % (what, k, getattr(h, k), d[k])
    kref.assert_bits(torch.tensor(list(h.row), dtype=F32), torch.tensor([h.norm, h.scale, float(h.apply), h.gscale], dtype=F32), what=what + " row")
    st = pl.get_state()
    for s, seg in enumerate(model["segs"]):
        got = (int(st["applied"][s]), float(st["bc1"][s]), float(st["sqrt_bc2"][s]))
        assert got == (seg["applied"], float(seg["bc1"]), float(seg["sqrt_bc2"])), "%s: segment %d is %r, expected %r" % (what, s, got, seg)


def test_decision_and_counters_follow_the_scripted_sequence():
    """fine, clipped, NaN, inf, fine, with the active set changing from step to step (gradual unfreezing)"""
    _case("decide-sequence")
    pl = Plan(counts=COUNTS)
    _, host = pl.table
    model = R.new_state(NSEG, COUNTS, host)
    base = kref.exact_operands((N,), F32, density=0.5, seed=11, exp=-3, maxmag=7, device=DEV)
    base[_seg(1).start] = 1.0
    sets = [[s >= 6 for s in range(NSEG)], [s >= 3 for s in range(NSEG)], ALL, ALL, [s != 4 for s in range(NSEG)]]
    script = [("fine", None, 1e4), ("clipped", None, 0.5), ("nan", float("nan"), 1e4), ("inf", float("inf"), 1e4), ("fine again", None, 1e4)]
    seen = []
    for (name, poison, max_norm), active in zip(script, sets):
        g = base.clone()
        if poison is not None:
            g[_seg(7).start + 1234] = poison
        for s in range(NSEG):
            if not active[s]:
                g[_seg(s)] = float("nan")
        pl.set_hyper([GROUP_HYPER[s % 3] for s in range(NSEG)], active)
        pl.norm(g, grad_scale=0.5, max_norm=max_norm, skip=True)
        torch.cuda.synchronize()
        sumsq, _ = R.ordered_sumsq(g.cpu().numpy(), pl.host_tiles, active)
        d = R.decide(sumsq, 0.5, max_norm, True, model, active, host)
        _compare(pl, d, model, 0.5, "sequence step %r" % name)
        h = pl.head()
        seen.append((h.apply, h.clipped, h.applied, h.skipped, h.clipped_total))
    assert seen == [(1, 0, 1, 0, 0), (1, 1, 2, 0, 1), (0, 0, 2, 1, 1), (0, 0, 2, 2, 1), (1, 0, 3, 2, 1)]
    assert pl.get_state()["applied"].tolist() == [c + k for c, k in zip(COUNTS, [1, 1, 1, 2, 1, 2, 3, 3, 3])]
    pl.margins_intact()


def test_advance_is_the_decision_without_a_gradient():
    _case("advance")
    pl = Plan(counts=COUNTS, active=ACTIVE)
    _, host = pl.table
    model = R.new_state(NSEG, COUNTS, host)
    pl.ctl[R.CTL_HEAD_BYTES:].view(torch.float64).fill_(float("nan"))       # partials of some earlier norm: not read
    for k, gs in enumerate((1.0, -0.25, 3.0)):
        pl.advance(gs)
        torch.cuda.synchronize()
        d = R.advance(gs, model, ACTIVE, host)
        _compare(pl, d, model, gs, "advance %d" % k)
        h = pl.head()
        assert (h.sumsq, h.norm, h.scale, h.gscale, h.apply, h.clipped, h.applied, h.skipped) == (0.0, 0.0, 1.0, gs, 1, 0, k + 1, 0)
    assert pl.get_state()["applied"].tolist() == [c + 3 * int(a) for c, a in zip(COUNTS, ACTIVE)]
    assert bool(torch.isnan(pl.ctl[R.CTL_HEAD_BYTES:].view(torch.float64)).all()), "ubg_advance wrote a partial"
    pl.margins_intact()


# ------------------------------------------------------------------------------------------------------------------------
# graph replay
# ------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_steps():
    """ubg_grad_norm + ubg_adam_step captured once on one stream, replayed three times, against three eager pairs"""
    _case("graph-replay")
    ops = _operands(500)
    for t in ops:
        t[_seg(GAP_AFTER).stop:_seg(GAP_AFTER + 1).start] = 0.0
    active = [s != 2 for s in range(NSEG)]
    max_norm = math.sqrt(float(sum(ops[1][_seg(s)].double().square().sum() for s in range(NSEG) if active[s]))) / 2

    def pair(pl, bufs):
        pl.norm(bufs[1], max_norm=max_norm, skip=True)
        pl.adam(*bufs)
    eager, epl = [t.clone() for t in ops], Plan(counts=COUNTS, active=active)
    for _ in range(3):
        pair(epl, eager)
    replay, rpl = [t.clone() for t in ops], Plan(counts=COUNTS, active=active)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair(rpl, replay)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for x, y, nm in zip(replay, eager, ("param", "grad", "exp_avg", "exp_avg_sq")):
        kref.assert_bits(x, y, what="graph replay against eager: " + nm)
    assert torch.equal(rpl.ctl, epl.ctl) and rpl.get_state().tobytes() == epl.get_state().tobytes()
    h = rpl.head()
    assert h.applied == 3 and h.clipped_total == 3
    assert rpl.get_state()["applied"].tolist() == [c + 3 * int(a) for c, a in zip(COUNTS, active)]
    assert not torch.equal(replay[0][_seg(7)], ops[0][_seg(7)]) and torch.equal(replay[0][_seg(2)], ops[0][_seg(2)])
    rpl.margins_intact()
