"""libubresnet_blend.so on the device, exactly: ubv_blend_begin and ubv_blend_tiles on the cases of tests/blend_ref.py -- tiles 5 x 7
(scalar path) and 8 x 12 (vector path) in views of 11 x 17 and 16 x 24, a buffer offset by one float, a column origin that is no
multiple of 4, C in {1, 3, 16}, pixels under 0, 1, 2 and 4 tiles inside one call and across two, a tile hanging over the view's
edge, and one case sized from the header geometry to reach a second, partial grid-stride trip.  Uncovered pixels keep a sentinel;
a pixel that one tile reaches holds fl(x + w) bit for bit (the tile's own bits where the weight is +0); every other element is
within the derived bound of the fp64 reference; -inf weights leave the buffer untouched; the edge rules of lae bit for bit; two
runs are bit-equal; the calls replay from a captured graph to the same bits.  Every buffer lies between guard margins that are
checked.  tests/test_cpu_blend.py holds the case ids against the compiled kernels."""
import numpy as np
import pytest
import torch

import blend_ref as R
import kref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _blend as V
    from ubresnet_amd import _lib as L

CASES = R.KERNEL_CASES
DEV = "cuda"
F32 = torch.float32
f32 = np.float32
MARGIN = 64                                                     # floats: 256 bytes, so the payload keeps the allocation's alignment
WORST = {}
T_LN2 = R.T.LN2_F32


class Guard:
    """an array's floats, `offset` floats past a 16-byte boundary, between two margins; begin() snapshots, check() asserts that
    nothing outside the payload (written=False: nothing at all) changed"""

    def __init__(self, shape, offset=0, fill=float("nan")):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.full = torch.full((self.n + 2 * MARGIN + offset,), fill, dtype=F32, device=DEV)
        self.lo = MARGIN + offset
        self.t = self.full[self.lo:self.lo + self.n].view(self.shape)
        assert self.t.data_ptr() % 16 == 4 * offset

    def set(self, v):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(v)).view(F32).view(self.shape))
        return self

    def begin(self):
        self.before = self.full.clone()
        return self

    def check(self, what, written=True):
        w = torch.zeros(self.full.numel(), dtype=torch.bool, device=DEV)
        if written:
            w[self.lo:self.lo + self.n] = True
        kref.assert_untouched(self.full, self.before, w, what)

    def bits(self):
        return self.t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _upload(name):
    """the case's operands on the device: [(logp, desc3, n, lw_rows, lw_cols)] as Guards, and the host inputs"""
    c = R.CASES[name]
    host = R.case_inputs(name)
    dev = []
    for logp, desc, lwr, lwc in host:
        dev.append((Guard(logp.shape, c["offset"]).set(logp).begin(), V.desc3(desc), len(desc),
                    Guard(lwr.shape, c["offset"]).set(lwr).begin(), Guard(lwc.shape, c["offset"]).set(lwc).begin()))
    return c, host, dev


def _calls(c, dev, out):
    th, tw = c["tile"]
    P, rows, cols = c["view"]
    for logp, desc, n, lwr, lwc in dev:
        V.blend_tiles(logp.t.data_ptr(), c["C"], th, tw, desc, n, lwr.t.data_ptr(), lwc.t.data_ptr(), out.t.data_ptr(), P, rows, cols,
                      L.stream_ptr())


def _run(name):
    """begin, the sentinel into the uncovered pixels, the case's calls -> (case, host inputs, device operands, out Guard, fp64
    reference, bound, cover count); checks everything that holds for every case"""
    c, host, dev = _upload(name)
    P, rows, cols = c["view"]
    Cn = c["C"]
    out = Guard((P, Cn, rows, cols), c["offset"], fill=7.0).begin()
    V.blend_begin(out.t.data_ptr(), out.n, L.stream_ptr())
    torch.cuda.synchronize()
    out.check(name + ": begin")
    assert (out.bits() == 0xFF800000).all(), name + ": begin did not store -inf everywhere"
    ref, lim, count = R.blend(np.full((P, Cn, rows, cols), -np.inf, f32), host)
    covered = np.broadcast_to(count[:, None] > 0, ref.shape)
    assert (~covered).any() and covered.any()
    out.t[torch.from_numpy(~covered).to(DEV)] = float(R.SENTINEL)
    out.begin()
    _calls(c, dev, out)
    torch.cuda.synchronize()
    out.check(name + ": out")
    for logp, _, _, lwr, lwc in dev:
        for g, nm in ((logp, "logp"), (lwr, "lw_rows"), (lwc, "lw_cols")):
            g.check("%s: %s" % (name, nm), written=False)
    bits = out.bits()
    assert (bits[~covered] == R.SENTINEL.view(np.uint32)).all(), name + ": a pixel no tile covers was written"
    # reached by one tile: fl(x + fl(lwr + lwc)) bit for bit
    once = np.zeros(ref.shape, np.uint32)
    for logp, desc, lwr, lwc in host:
        th, tw = logp.shape[2:]
        for t, (p, r0, c0) in enumerate(desc):
            hh, ww = min(th, rows - r0), min(tw, cols - c0)
            once[p, :, r0:r0 + hh, c0:c0 + ww] = R.operand32(logp[t], lwr[t], lwc[t])[:, :hh, :ww].view(np.uint32)
    single = np.broadcast_to(count[:, None] == 1, ref.shape)
    assert single.any() and np.array_equal(bits[single], once[single]), name + ": a pixel under one tile is not fl(x + w)"
    got = bits.view(f32).astype(np.float64)
    multi = covered & ~single
    assert not np.isnan(got[covered]).any() and np.array_equal(np.isneginf(got[covered]), np.isneginf(ref[covered])), name
    fin = multi & np.isfinite(ref)
    assert fin.any()
    err = np.abs(got[fin] - ref[fin])                             # a bound of zero (x = +0 with weight +0 and nothing else) admits no error
    ratio = np.where(lim[fin] > 0, err / np.where(lim[fin] > 0, lim[fin], 1.0), np.where(err == 0, 0.0, np.inf))
    WORST[name] = float(ratio.max())
    print("%s: worst error / bound %.3f (max |err| %.3e) over %d elements" % (name, WORST[name], float(err.max()), int(fin.sum())))
    assert WORST[name] <= 1.0, "%s: worst error / bound %.3f" % (name, WORST[name])
    return c, host, dev, out, ref, count


def test_the_geometry_is_the_header_s():
    assert (V.BLOCK, V.MAX_GRID, V.MAX_TILES, V.MAX_CLASSES) == (R.BLOCK, R.MAX_GRID, R.MAX_TILES, R.MAX_CLASSES)
    assert R.grid(R.units("second-trip", 0)) == V.MAX_GRID < -(-R.units("second-trip", 0) // R.BLOCK)
    assert R.grid(R.begin_units("second-trip")) == V.MAX_GRID < -(-R.begin_units("second-trip") // R.BLOCK)


@pytest.mark.parametrize("name", ["scalar-C1", "scalar-C3-two-calls", "scalar-C16", "vector-C1", "vector-C3-two-calls", "vector-C16",
                                  "offset-C3", "odd-origin-C3", "second-trip"])
def test_blend(name):
    c, host, dev, out, ref, count = _run(name)
    assert set(count.ravel().tolist()) >= ({0, 1, 2} if name == "second-trip" else {0, 1, 2, 4})
    first = out.bits().copy()
    # weight +0 on the first tile of the first call: where it stands alone the tile's own bits arrive
    logp, desc, lwr, lwc = host[0]
    assert not lwr[0].any() and not lwc[0].any() and not np.signbit(lwr[0]).any()
    p, r0, c0 = desc[0]
    th, tw = c["tile"]
    alone = count[p, r0:r0 + th, c0:c0 + tw] == 1
    assert alone.any() and np.array_equal(first[p, :, r0:r0 + th, c0:c0 + tw][:, alone], logp[0].view(np.uint32)[:, alone])
    # the same calls on the same buffer state: the same bits
    V.blend_begin(out.t.data_ptr(), out.n, L.stream_ptr())
    out.t[torch.from_numpy(np.broadcast_to(count[:, None] == 0, ref.shape).copy()).to(DEV)] = float(R.SENTINEL)
    _calls(c, dev, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.bits(), first), name + ": two runs differ"
    if name == "second-trip":
        return
    # a call whose every row weight is -inf leaves the buffer as it is, bit for bit
    lg, d3, n, gr, gc = dev[-1]
    dead = Guard(gr.shape, c["offset"]).set(np.full(gr.shape, -np.inf, f32))
    out.begin()
    P, rows, cols = c["view"]
    V.blend_tiles(lg.t.data_ptr(), c["C"], th, tw, d3, n, dead.t.data_ptr(), gc.t.data_ptr(), out.t.data_ptr(), P, rows, cols, L.stream_ptr())
    torch.cuda.synchronize()
    out.check(name + ": -inf weights", written=False)


def _edge_pairs():
    """every ordered pair of these values that lae settles without a library call: (-inf, -inf), (-inf, x), (x, x), (+inf, x), NaN"""
    vals = np.array([-np.inf, np.inf, np.nan, -0.0, 0.0, -1.25, -100.0, -1e-38, -3e38, 1e-45, 2.5], dtype=f32)
    a, b = np.repeat(vals, len(vals)), np.tile(vals, len(vals))
    with np.errstate(all="ignore"):
        b0 = (b + f32(0)).astype(f32)                           # the weight +0 is added: -0.0 arrives as +0.0
        out, general = R.lae32(a, b0)
    keep = ~general
    return a[keep], b[keep], out[keep]


@pytest.mark.parametrize("width", [1, 4])
def test_edge_rules_bit_for_bit(width):
    """the running values a in the view, one tile of one row over it with the values b and weight +0: out = lae(a, b + 0).
    width 1: an odd number of columns, scalar path; width 4: a multiple of 4, vector path"""
    a, b, want = _edge_pairs()
    n = len(a) // 4 * 4 if width == 4 else len(a) // 2 * 2 + 1
    a, b, want = a[:n], b[:n], want[:n]
    assert n >= 60 and np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    out = Guard((1, 1, 1, n)).set(a.reshape(1, 1, 1, n)).begin()
    tile = Guard((1, 1, 1, n)).set(b.reshape(1, 1, 1, n)).begin()
    zr, zc = Guard((1, 1)).set(np.zeros((1, 1), f32)), Guard((1, n)).set(np.zeros((1, n), f32))
    V.blend_tiles(tile.t.data_ptr(), 1, 1, n, V.desc3([(0, 0, 0)]), 1, zr.t.data_ptr(), zc.t.data_ptr(), out.t.data_ptr(), 1, 1, n, L.stream_ptr())
    torch.cuda.synchronize()
    kref.assert_bits(out.t.reshape(-1), torch.from_numpy(want), what="edge rules, width %d" % width)
    out.check("edge rules: out")
    tile.check("edge rules: logp", written=False)
    same = (a == b) & np.isfinite(a)
    assert same.any() and np.array_equal(want[same].view(np.uint32), (np.maximum(a[same], b[same]) + T_LN2).astype(f32).view(np.uint32))
    # a weight of -inf: out stays a bit for bit, except that a +inf or NaN log-probability meets it as NaN
    out.set(a.reshape(1, 1, 1, n)).begin()
    zr.set(np.full((1, 1), -np.inf, f32))
    V.blend_tiles(tile.t.data_ptr(), 1, 1, n, V.desc3([(0, 0, 0)]), 1, zr.t.data_ptr(), zc.t.data_ptr(), out.t.data_ptr(), 1, 1, n, L.stream_ptr())
    torch.cuda.synchronize()
    poisoned = np.isnan(b) | (np.isinf(b) & (b > 0)) | np.isnan(a)
    got = out.bits().reshape(-1)
    assert np.array_equal(got[~poisoned], a[~poisoned].view(np.uint32)) and np.isnan(got.view(f32)[poisoned]).all()


def test_a_captured_graph_replays_begin_and_two_calls():
    """no launch argument depends on anything the device decides: begin and the two calls of a case capture as they are"""
    name = "vector-C3-two-calls"
    c, host, dev = _upload(name)
    P, rows, cols = c["view"]
    out = Guard((P, c["C"], rows, cols), fill=7.0)
    torch.cuda.synchronize()

    def calls():
        V.blend_begin(out.t.data_ptr(), out.n, L.stream_ptr())
        _calls(c, dev, out)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls()
    torch.cuda.synchronize()
    assert bool((out.t == 7.0).all()), "the capture ran something"
    out.begin()
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.bits().copy()
    out.check("replay")
    out.t.fill_(7.0)
    calls()
    torch.cuda.synchronize()
    assert np.array_equal(replayed, out.bits()), "the replay differs from the eager calls"
    ref, lim, count = R.blend(np.full((P, c["C"], rows, cols), -np.inf, f32), host)
    covered = np.broadcast_to(count[:, None] > 0, ref.shape)
    assert (replayed[~covered] == 0xFF800000).all()
    fin = covered & np.isfinite(ref)
    assert (np.abs(replayed.view(f32).astype(np.float64)[fin] - ref[fin]) <= np.maximum(lim[fin], 0)).all()
