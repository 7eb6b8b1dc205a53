"""libubresnet_stats.so on the device, exactly: ubs_scan's per-row counts, ubs_note, the decision of ubs_decide field for field
and ubs_resolve's moves against tests/stats_ref.py, as whole-buffer bit comparisons.  The live and the shadow arena are filled
with a recognisable pattern around every run, so a write outside a run is seen; the control block lies between checked margins.
Row counts come from the header's geometry; the values are NaNs with payloads (quiet and signalling), both infinities, both zeros,
the largest finite value and subnormals of either sign in the fp32 rows, and int64 values whose halves look like NaN or Inf in the
raw rows.  One captured graph of the four calls is replayed over keep, restore, keep."""
import itertools

import numpy as np
import pytest
import torch

import stats_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _stats as S

DEV = "cuda"
FILL_LIVE, FILL_SHADOW = 0xA5A5A5A5, 0x5A5A5A5A         # (as fp32: a small negative value and a large positive one: both finite)
MARGIN, GAP = 64, 3
B_ = R.BLOCK
# fp32 bit patterns that must NOT count: both zeros, the largest finite value of either sign, subnormals of either sign
FINITE_EDGES = [0x00000000, 0x80000000, 0x7f7fffff, 0xff7fffff, 0x00000001, 0x807fffff, 0x007fffff, 0x80000001]
# and those that must: quiet and signalling NaNs with payloads, both infinities
QNAN, QNAN_NEG, SNAN, SNAN_NEG, PINF, NINF = 0x7fc00001, 0xffc12345, 0x7f800001, 0xffbfffff, 0x7f800000, 0xff800000
# int64 values whose 32-bit halves look like NaN or Inf as floats (low half first in memory)
RAW_NANLIKE = [(0x7f800000, 0x7fc00001), (0xffc12345, 0xff800000), (0x7f800001, 0xffffffff)]

# the rows of the general layout: (count, kind); an empty row in the middle, two raw rows (an int64 scalar is 2 units)
ROWS = [(1, 0), (2, 0), (3, 0), (B_ - 1, 0), (0, 0), (B_, 0), (B_ + 1, 0), (2, 1), (4 * B_ + 1, 0), (6, 1)]
BAD_ONE = {3: [(B_ - 2, QNAN)]}                                                       # row -> [(index in the row, bits)]
BAD_THREE = {0: [(0, QNAN_NEG)], 6: [(0, SNAN), (B_, NINF), (17, SNAN_NEG)], 8: [(4 * B_, PINF), (B_ + 5, QNAN), (2 * B_, PINF), (3, NINF)]}
CONTENTS = {"clean": ({}, False), "one-bad-row": (BAD_ONE, False), "three-bad-rows": (BAD_THREE, False), "raw-only": ({}, True)}


class Arena(object):
    """the rows' runs in one shadow and one live buffer of 32-bit units, GAP watched units between neighbours and a margin at
    either end; a numpy mirror of both; the device table"""

    def __init__(self, rows):
        self.rows, at = [], MARGIN
        for count, kind in rows:
            self.rows.append((at, at + 1, count, kind))              # the live run starts one unit later than the shadow run
            at += count + GAP + 1
        self.total = at + MARGIN
        self.h_shadow = np.full(self.total, FILL_SHADOW, dtype=np.uint32)
        self.h_live = np.full(self.total, FILL_LIVE, dtype=np.uint32)
        self.shadow = torch.from_numpy(self.h_shadow.view(np.int32).copy()).to(DEV)
        self.live = torch.from_numpy(self.h_live.view(np.int32).copy()).to(DEV)
        t = S.seg_table([self.shadow.data_ptr() + 4 * so for so, _, _, _ in self.rows], [self.live.data_ptr() + 4 * lo for _, lo, _, _ in self.rows],
                        [c for _, _, c, _ in self.rows], [k for _, _, _, k in self.rows])
        self.table = torch.from_numpy(t.view(np.int64).reshape(-1, 4).copy()).to(DEV)
        self.nseg = len(rows)
        self.bad = torch.full((self.nseg + 2 * MARGIN,), 0x77, dtype=torch.int32, device=DEV)
        self.seen = torch.zeros(self.nseg, dtype=torch.int32, device=DEV)
        self.ctl_full = torch.full((R.CTL_BYTES + 512,), 0xA5, dtype=torch.uint8, device=DEV)
        self.ctl = self.ctl_full[256:256 + R.CTL_BYTES]
        S.ctl_init(self.ctl.data_ptr(), L.stream_ptr())
        self.h_seen = np.zeros(self.nseg, dtype=np.int32)
        self.ref = R.Ctl()

    def bad_view(self):
        return self.bad[MARGIN:MARGIN + self.nseg]

    def set_live(self, rs, bad=None, raw_nanlike=False):
        """fresh live values in every run (finite fp32 with the finite edge values among them; raw rows: arbitrary int64 that do
        not look like NaN, or the NaN-like ones), then the bad values of `bad`; host mirror and device"""
        for r, (_, lo, count, kind) in enumerate(self.rows):
            if count <= 0:
                continue
            if kind == R.KIND_F32:
                v = rs.standard_normal(count).astype(np.float32).view(np.uint32)
                k = min(count, len(FINITE_EDGES))
                at = rs.permutation(count)[:k]
                v[at] = np.array(FINITE_EDGES[:k], dtype=np.uint32)
            else:
                v = rs.randint(0, 1 << 30, size=count, dtype=np.int64).astype(np.uint32)          # exponent fields below all-ones
                if raw_nanlike:
                    flat = np.array([h for pair in RAW_NANLIKE for h in pair], dtype=np.uint32)
                    v[:min(count, len(flat))] = flat[:count]
            self.h_live[lo:lo + count] = v
        for r, items in (bad or {}).items():
            _, lo, count, kind = self.rows[r]
            assert kind == R.KIND_F32
            for i, bits in items:
                assert i < count
                self.h_live[lo + i] = bits
        self.live.copy_(torch.from_numpy(self.h_live.view(np.int32)))

    def call(self, flag_addr, flag_value, check, note=True):
        """the four launches, then the reference's replay on the mirror"""
        st = L.stream_ptr()
        S.scan(self.table.data_ptr(), self.nseg, self.bad_view().data_ptr(), st)
        if note:
            S.note(self.seen.data_ptr(), self.bad_view().data_ptr(), self.nseg, st)
        S.decide(self.ctl.data_ptr(), self.bad_view().data_ptr(), self.nseg, flag_addr, check, st)
        S.resolve(self.table.data_ptr(), self.nseg, self.ctl.data_ptr(), st)
        self.replay(flag_value, check, note)

    def replay(self, flag_value, check, note=True):
        self.h_bad = R.scan(self.h_live, self.rows)
        if note:
            self.h_seen = R.note(self.h_seen, self.h_bad)
        self.ref.decide(self.h_bad, flag_value, check)
        R.resolve(self.h_shadow, self.h_live, self.rows, self.ref.keep)

    def compare(self, what):
        torch.cuda.synchronize()
        h = S.read_ctl(self.ctl.cpu().numpy().tobytes())
        got = (h.keep, h.bad_rows, h.kept, h.restored, h.restored_for_stats)
        assert got == self.ref.fields(), "%s: control block %r, reference %r" % (what, got, self.ref.fields())
        assert self.bad_view().cpu().numpy().tolist() == self.h_bad.tolist(), "%s: bad[]" % what
        assert self.seen.cpu().numpy().tolist() == self.h_seen.tolist(), "%s: seen[]" % what
        for name, dev, host in (("live", self.live, self.h_live), ("shadow", self.shadow, self.h_shadow)):
            diff = dev.cpu().numpy().view(np.uint32) != host
            assert not diff.any(), "%s: %s differs from the reference in %d units, first at %d" % (what, name, int(diff.sum()), int(diff.argmax()))
        assert bool((self.bad[:MARGIN] == 0x77).all()) and bool((self.bad[-MARGIN:] == 0x77).all()), "%s: wrote outside bad[]" % what
        assert bool((self.ctl_full[:256] == 0xA5).all()) and bool((self.ctl_full[-256:] == 0xA5).all()), "%s: wrote outside the control block" % what


def _flag(value):
    """an optimizer's control block as far as ubs_decide looks: an int32 at byte 20 of a 16-byte aligned block -> (block, address)"""
    if value is None:
        return None, None
    blk = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    blk[R.APPLY_OFFSET // 4] = value
    return blk, blk.data_ptr() + R.APPLY_OFFSET


def test_the_rows_cover_the_paths_of_the_launch():
    counts = [c for c, _ in ROWS]
    assert all(c in counts for c in (1, 2, 3, B_ - 1, B_, B_ + 1, 4 * B_ + 1)) and 0 in counts[1:-1]
    assert sorted(k for _, k in ROWS) == [0] * 8 + [1] * 2
    a = Arena(ROWS)
    # the patterns around the runs are finite as fp32, the bad values are not, the finite edge values are
    for bits, bad in [(FILL_LIVE, 0), (FILL_SHADOW, 0)] + [(b, 0) for b in FINITE_EDGES] + [(b, 1) for b in (QNAN, QNAN_NEG, SNAN, SNAN_NEG, PINF, NINF)]:
        assert int(R.scan(np.array([bits], dtype=np.uint32), [(0, 0, 1, 0)])[0]) == bad
        assert bool(np.isfinite(np.array([bits], dtype=np.uint32).view(np.float32))[0]) == (not bad)
    assert all(lo == so + 1 for so, lo, _, _ in a.rows) and a.total == sum(counts) + len(ROWS) * (GAP + 1) + 2 * MARGIN


def test_ctl_init_zeroes_the_block():
    a = Arena([(1, 0)])
    torch.cuda.synchronize()
    assert not a.ctl.cpu().numpy().any(), "ubs_ctl_init left a nonzero byte"
    a.ctl.fill_(0xEE)
    S.ctl_init(a.ctl.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    assert not a.ctl.cpu().numpy().any()
    assert bool((a.ctl_full[:256] == 0xA5).all()) and bool((a.ctl_full[-256:] == 0xA5).all())


@pytest.mark.parametrize(("flag", "check", "content"), list(itertools.product((None, 0, 1), (1, 0), sorted(CONTENTS))),
                         ids=lambda v: str(v))
def test_six_calls_follow_the_reference_bit_for_bit(flag, check, content):
    """calls 1, 3, 4 and 6 see the content, calls 2 and 5 clean values; fresh live values before every call"""
    bad, raw = CONTENTS[content]
    a = Arena(ROWS)
    rs = np.random.RandomState(7)
    a.set_live(rs)
    for so, lo, count, _ in a.rows:                            # the shadow starts as a copy of a first, clean set of live values
        a.h_shadow[so:so + count] = a.h_live[lo:lo + count]
    a.shadow.copy_(torch.from_numpy(a.h_shadow.view(np.int32)))
    blk, addr = _flag(flag)
    keeps = []
    for k in range(6):
        dirty = k in (0, 2, 3, 5)
        a.set_live(rs, bad if dirty else None, raw and dirty)
        before = None if blk is None else blk.clone()
        a.call(addr, flag, check)
        a.compare("call %d (flag %r, check %d, %s)" % (k + 1, flag, check, content))
        keeps.append(a.ref.keep)
        if blk is not None:
            assert torch.equal(blk, before), "ubs_decide wrote to the optimizer's block"
    # what the rule says for this combination, spelled out
    poisons = bool(bad) and bool(check)
    want = [int(flag != 0 and not (poisons and k in (0, 2, 3, 5))) for k in range(6)]
    assert keeps == want
    rows_bad = len(bad)
    assert a.ref.bad_rows == rows_bad and a.h_bad.tolist() == [len(bad.get(r, [])) for r in range(len(ROWS))]
    assert a.ref.fields()[2:] == (sum(want), 6 - sum(want), 4 if (poisons and flag != 0) else 0)
    assert a.h_seen.tolist() == [4 * len(bad.get(r, [])) for r in range(len(ROWS))]


@pytest.mark.parametrize("nseg", [1, R.SEG_GRID + 1], ids=["one-row", "one-workgroup-takes-two-rows"])
def test_the_number_of_rows(nseg):
    """a table of one row; a table of UBS_SEG_GRID + 1 rows: workgroup 0 takes rows 0 and UBS_SEG_GRID, bad values in both"""
    rows = [(5, 0)] if nseg == 1 else [((2, 1) if r % 3 == 1 else (2 + r % 4, 0)) for r in range(nseg - 1)] + [(B_ + 1, 0)]
    bad = {0: [(1, SNAN)]} if nseg == 1 else {0: [(1, SNAN)], 8: [(0, PINF), (1, NINF)], nseg - 1: [(B_, QNAN)]}
    a = Arena(rows)
    rs = np.random.RandomState(nseg)
    blk, addr = _flag(1)
    for k, (dirty, flag) in enumerate([(False, 1), (True, 1), (False, 0), (False, 1)]):
        a.set_live(rs, bad if dirty else None, raw_nanlike=True)
        blk[R.APPLY_OFFSET // 4] = flag
        a.call(addr, flag, 1)
        a.compare("nseg %d call %d" % (nseg, k + 1))
        if dirty:
            assert a.h_bad[0] == 1 and a.h_bad[nseg - 1] == 1 and a.ref.bad_rows == len(bad)
    assert a.ref.fields() == (1, 0, 2, 2, 1)
    assert (a.h_seen != 0).sum() == len(bad)


def test_a_captured_graph_replays_keep_restore_keep():
    """the four calls captured once; between replays only the flag's value and the live bytes change; a twin arena takes the same
    three steps as direct calls"""
    g, d = Arena(ROWS), Arena(ROWS)
    rs_g, rs_d = np.random.RandomState(11), np.random.RandomState(11)
    blk_g, addr_g = _flag(1)
    blk_d, addr_d = _flag(1)
    g.set_live(rs_g)
    d.set_live(rs_d)
    torch.cuda.synchronize()
    st = g.shadow.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stp = L.stream_ptr()
        S.scan(g.table.data_ptr(), g.nseg, g.bad_view().data_ptr(), stp)
        S.note(g.seen.data_ptr(), g.bad_view().data_ptr(), g.nseg, stp)
        S.decide(g.ctl.data_ptr(), g.bad_view().data_ptr(), g.nseg, addr_g, 1, stp)
        S.resolve(g.table.data_ptr(), g.nseg, g.ctl.data_ptr(), stp)
    torch.cuda.synchronize()
    assert torch.equal(g.shadow, st) and S.read_ctl(g.ctl.cpu().numpy().tobytes()).kept == 0             # the capture ran nothing
    for k, (flag, bad) in enumerate([(1, None), (0, None), (1, None)]):
        if k:
            g.set_live(rs_g, bad)
            d.set_live(rs_d, bad)
        blk_g[R.APPLY_OFFSET // 4] = flag
        blk_d[R.APPLY_OFFSET // 4] = flag
        graph.replay()
        g.replay(flag, 1)
        d.call(addr_d, flag, 1)
        g.compare("replay %d" % (k + 1))
        d.compare("direct call %d" % (k + 1))
        assert torch.equal(g.live, d.live) and torch.equal(g.shadow, d.shadow) and torch.equal(g.ctl, d.ctl)
    assert g.ref.fields() == (1, 0, 2, 1, 0)
    # and a fourth replay in which only the scan objects: same graph, live bytes with a NaN
    g.set_live(rs_g, BAD_ONE)
    graph.replay()
    g.replay(1, 1)
    g.compare("replay 4")
    assert g.ref.fields() == (0, 1, 2, 2, 1)
