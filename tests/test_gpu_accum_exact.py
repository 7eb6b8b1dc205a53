"""libubresnet_accum.so on the device, exactly: ubc_set on arbitrary bit patterns, ubc_add and ubc_finish against the numpy replay
of tests/accum_ref.py over whole buffers bit for bit (sizes from the header's geometry, edge values in both operands), what each
call must leave alone, a whole cycle, and the same cycle captured in a graph.  Every buffer lies between guard margins that are
checked."""
import numpy as np
import pytest
import torch

import accum_ref as R
import kref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _accum as A
    from ubresnet_amd import _lib as L

DEV = "cuda"
F32 = torch.float32
f32 = np.float32
SIZES = R.flat_sizes()
FLT_MIN = f32(1.1754944e-38)


class Guard:
    """n elements between two 64-element margins; begin() snapshots, check() asserts that nothing outside the n elements
    (written=False: nothing at all) changed"""

    def __init__(self, n, fill=float("nan")):
        self.full = torch.full((n + 128,), fill, dtype=F32, device=DEV)
        self.t = self.full[64:64 + n]
        self.n = n

    def set(self, v):
        self.t.copy_(torch.from_numpy(v) if isinstance(v, np.ndarray) else v)
        return self

    def begin(self):
        self.before = self.full.clone()
        return self

    def check(self, what, written=True):
        w = torch.zeros(self.n + 128, dtype=torch.bool, device=DEV)
        if written:
            w[64:64 + self.n] = True
        kref.assert_untouched(self.full, self.before, w, what)


def _bits(t):
    return t.view(torch.int32)


def _rand_bits(rs, n):
    """n arbitrary 32-bit patterns as fp32 (NaNs with payloads, infinities, subnormals and both zeros among them)"""
    v = rs.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    v[:8] = [0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000000, 0x7f800000, 0x00000001, 0x807fffff][:min(n, 8)]
    return torch.from_numpy(v.view(np.int32).copy()).view(F32)


def _operands(rs, n, k=0):
    """ordinary values with some subnormal and near-subnormal ones among them"""
    v = (rs.standard_normal(n) * (1.0 + k)).astype(f32)
    v[k % 7::7] *= f32(1e-38)
    return v


def _edge_pairs():
    """every pair of kref.edge_table(float32) values (subnormals, both zeros, both infinities, NaN, the largest finite value)
    and pairs whose sum is normal while the sum times a scale of 1/4 or 1/3 is subnormal; padded with ones to a multiple of 4"""
    edge = kref.edge_values(F32).numpy()
    k = len(edge)
    a, g = np.repeat(edge, k), np.tile(edge, k)
    a = np.concatenate([a, f32([1.5e-38, -1.5e-38, 1.2e-38, 3e-38])])
    g = np.concatenate([g, f32([1.0e-38, -1.0e-38, 2e-45, -1.7e-38])])
    n = (len(a) + 3) // 4 * 4
    return np.concatenate([a, np.ones(n - len(a), f32)]), np.concatenate([g, np.ones(n - len(g), f32)]), n


def test_the_sizes_come_from_the_geometry():
    t = A.BLOCK * A.UNROLL
    assert (A.BLOCK, A.UNROLL, A.MAX_GRID) == (R.BLOCK, R.UNROLL, R.MAX_GRID)
    assert SIZES == [4, 4 * (t - 1), 4 * t, 4 * (t + 1), 4 * (A.MAX_GRID * t + 1)] and [R.grid(n) for n in SIZES] == [1, 1, 1, 2, A.MAX_GRID]


@pytest.mark.parametrize("n", SIZES)
def test_set_copies_bit_patterns_and_leaves_the_gradient(n):
    rs = np.random.RandomState(n % 65521)
    acc, g = Guard(n), Guard(n)
    g.t.copy_(_rand_bits(rs, n))
    acc.t.copy_(_rand_bits(rs, n))
    acc.begin()
    g.begin()
    A.set_(acc.t.data_ptr(), g.t.data_ptr(), n, L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(acc.t), _bits(g.t)), "n=%d: not copied bit for bit" % n
    assert int(_bits(acc.t)[0]) == 0x7fc00001                                          # a NaN payload went across
    acc.check("n=%d set: acc" % n)
    g.check("n=%d set: grad" % n, written=False)


@pytest.mark.parametrize("n", SIZES)
def test_add_then_finish_are_the_numpy_replay(n):
    rs = np.random.RandomState(n % 65519)
    ha, hg = _operands(rs, n, 0), _operands(rs, n, 1)
    acc, g = Guard(n).set(ha).begin(), Guard(n).set(hg).begin()
    A.add(acc.t.data_ptr(), g.t.data_ptr(), n, L.stream_ptr())
    torch.cuda.synchronize()
    ha = R.add(ha, hg)
    kref.assert_bits(acc.t, torch.from_numpy(ha), what="n=%d add: acc" % n)
    acc.check("n=%d add: acc" % n)
    g.check("n=%d add: grad" % n, written=False)
    hg = _operands(rs, n, 2)
    g.set(hg).begin()
    acc.begin()
    scale = R.scale_of(3)
    A.finish(g.t.data_ptr(), acc.t.data_ptr(), n, scale, L.stream_ptr())
    torch.cuda.synchronize()
    kref.assert_bits(g.t, torch.from_numpy(R.finish(ha, hg, scale)), what="n=%d finish: grad" % n)
    g.check("n=%d finish: grad" % n)
    acc.check("n=%d finish: acc" % n, written=False)


def test_add_on_edge_values_in_both_operands():
    ha, hg, n = _edge_pairs()
    acc, g = Guard(n, fill=1.0).set(ha).begin(), Guard(n, fill=1.0).set(hg).begin()
    A.add(acc.t.data_ptr(), g.t.data_ptr(), n, L.stream_ptr())
    torch.cuda.synchronize()
    want = R.add(ha, hg)
    with np.errstate(all="ignore"):
        fin_in = np.isfinite(ha) & np.isfinite(hg)
        assert (np.isnan(want) & np.isinf(ha) & np.isinf(hg)).any()                                    # inf + -inf
        assert (np.isinf(want) & fin_in).any()                                                         # a sum that overflows
        assert ((want != 0) & (np.abs(want) < FLT_MIN) & (ha != 0) & (hg != 0)).any()                  # subnormal + subnormal = subnormal
        assert ((want == 0) & np.signbit(want)).any() and ((want == 0) & ~np.signbit(want)).any()     # both zeros come out
    kref.assert_bits(acc.t, torch.from_numpy(want), what="edge values: add")                           # finite: the bits; NaN: NaN
    acc.check("edge values add: acc")
    g.check("edge values add: grad", written=False)


@pytest.mark.parametrize("scale", [f32(0.25), f32(1.0 / 3.0), f32(1.0)], ids=["1/4", "1/3", "1"])
def test_finish_on_edge_values_in_both_operands(scale):
    ha, hg, n = _edge_pairs()
    acc, g = Guard(n, fill=1.0).set(ha).begin(), Guard(n, fill=1.0).set(hg).begin()
    A.finish(g.t.data_ptr(), acc.t.data_ptr(), n, scale, L.stream_ptr())
    torch.cuda.synchronize()
    want = R.finish(ha, hg, scale)
    with np.errstate(all="ignore"):
        s = R.add(ha, hg)
        assert np.isnan(want).any() and np.isinf(want).any() and ((want != 0) & (np.abs(want) < FLT_MIN)).any()
        if scale != f32(1.0):
            assert ((np.abs(s) >= FLT_MIN) & np.isfinite(s) & (want != 0) & (np.abs(want) < FLT_MIN)).any()   # a normal sum scaled into the subnormals
    kref.assert_bits(g.t, torch.from_numpy(want), what="edge values: finish, scale %r" % float(scale))
    g.check("edge values finish: grad")
    acc.check("edge values finish: acc", written=False)


def _cycle_operands(rs, n, k0=0):
    hs = [_operands(rs, n, k0 + k) for k in range(3)]
    hs[1][5::13] = -hs[0][5::13]                                # cancellation to zero here and there
    hs[2][1::17] = f32(3e38)
    hs[0][1::34] = f32(3e38)                                    # overflow at some of those
    hs[2][5::26] = f32(0.0)                                     # and the zero stays a zero at some
    return hs


@pytest.mark.parametrize("n", [SIZES[3], SIZES[4]])
def test_a_cycle_of_three_is_the_replay(n):
    """what GradAccumulator(every=3) launches: set, add, finish with float32(1/3), the gradient buffer rewritten in between as a
    replayed backward rewrites it"""
    rs = np.random.RandomState(3)
    hs = _cycle_operands(rs, n)
    scale = R.scale_of(3)
    acc, g = Guard(n), Guard(n)
    acc.begin()
    g.begin()
    s = L.stream_ptr()
    g.set(hs[0])
    A.set_(acc.t.data_ptr(), g.t.data_ptr(), n, s)
    g.set(hs[1])
    A.add(acc.t.data_ptr(), g.t.data_ptr(), n, s)
    g.set(hs[2])
    A.finish(g.t.data_ptr(), acc.t.data_ptr(), n, scale, s)
    torch.cuda.synchronize()
    want = R.cycle(hs, scale)
    assert np.isinf(want).any() and (want == 0).any()
    kref.assert_bits(g.t, torch.from_numpy(want), what="n=%d cycle: grad" % n)
    kref.assert_bits(acc.t, torch.from_numpy(R.add(R.set_(hs[0]), hs[1])), what="n=%d cycle: acc" % n)
    g.check("n=%d cycle: grad" % n)
    acc.check("n=%d cycle: acc" % n)


def test_a_captured_cycle_replays_on_fresh_operands():
    """no launch argument depends on anything the device decides: the three launches capture as they are"""
    n = SIZES[3]
    scale = R.scale_of(3)
    acc, gs = Guard(n), [Guard(n) for _ in range(3)]
    for b in gs:
        b.set(np.ones(n, f32))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        A.set_(acc.t.data_ptr(), gs[0].t.data_ptr(), n, L.stream_ptr())
        A.add(acc.t.data_ptr(), gs[1].t.data_ptr(), n, L.stream_ptr())
        A.finish(gs[2].t.data_ptr(), acc.t.data_ptr(), n, scale, L.stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(acc.t).all()) and bool((gs[2].t == 1).all())               # the capture ran nothing
    for rep in range(2):
        rs = np.random.RandomState(40 + rep)
        hs = _cycle_operands(rs, n, rep)
        for b, h in zip(gs, hs):
            b.set(h).begin()
        acc.begin()
        graph.replay()
        torch.cuda.synchronize()
        kref.assert_bits(gs[2].t, torch.from_numpy(R.cycle(hs, scale)), what="replay %d: grad" % (rep + 1))
        kref.assert_bits(acc.t, torch.from_numpy(R.add(R.set_(hs[0]), hs[1])), what="replay %d: acc" % (rep + 1))
        gs[0].check("replay %d: first gradient" % (rep + 1), written=False)
        gs[1].check("replay %d: second gradient" % (rep + 1), written=False)
        gs[2].check("replay %d: last gradient" % (rep + 1))
        acc.check("replay %d: acc" % (rep + 1))
