"""libubresnet_tta.so on the device, exactly: ubt_flip_planes on arbitrary bit patterns for every flip, ubt_merge_view for one to four
views with a different flip each -- view 0 and K = 1 bit for bit, every other element within the derived bound of tests/tta_ref.py
of the fp64 reference -- the edge rules of lae bit for bit, the symmetry of two views, and the same calls replayed from a captured
graph.  The shapes are R.SHAPES (scalar and vector path, a misaligned base, a second partial trip of the grid-stride loop); every
buffer lies between guard margins that are checked.  tests/test_cpu_tta.py holds the case ids against the compiled kernels."""
import numpy as np
import pytest
import torch

import kref
import tta_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _tta as T

DEV = "cuda"
F32 = torch.float32
f32 = np.float32
MARGIN = 64                                                     # floats: 256 bytes, so the payload keeps the allocation's alignment
_VIEWS = {}                                                     # shape name -> four views of log-probabilities, made once
WORST = {}                                                      # case id -> worst error / bound


class Guard:
    """shape-many floats, `offset` floats past a 16-byte boundary, between two margins; begin() snapshots, check() asserts that
    nothing outside the payload (written=False: nothing at all) changed"""

    def __init__(self, name, fill=float("nan")):
        self.shape, off = R.SHAPES[name]["shape"], R.SHAPES[name]["offset"]
        self.n = int(np.prod(self.shape))
        self.full = torch.full((self.n + 2 * MARGIN + off,), fill, dtype=F32, device=DEV)
        self.lo = MARGIN + off
        self.t = self.full[self.lo:self.lo + self.n].view(self.shape)
        assert self.t.data_ptr() % 16 == 4 * off

    def set(self, v):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(v)).view(F32) if isinstance(v, np.ndarray) else v)
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


def _patterns(rs, shape):
    """arbitrary 32-bit patterns with every row of kref.edge_table(float32) among them (NaN payloads, -0.0, subnormals,
    infinities), as uint32"""
    n = int(np.prod(shape))
    v = rs.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    edge = np.array([b for _, b in kref.edge_table(F32)] + [0x7fc00001, 0xffc12345, 0x7f800001], dtype=np.uint32)
    pos = (np.arange(len(edge)) * 7) % n                         # spread over the rows; a one-element plane gets the last of them
    v[pos] = edge
    return v.reshape(shape)


def _views(name):
    if name not in _VIEWS:
        rs = np.random.RandomState(sum(R.SHAPES[name]["shape"]) % 65521)
        _VIEWS[name] = [R.logsoftmax_rows(rs, R.SHAPES[name]["shape"]) for _ in range(R.MAX_VIEWS)]
    return _VIEWS[name]


def _merge_on_device(acc, bufs, flips, after_first=None):
    K = len(flips)
    n, H, W = acc.shape
    for k, (b, flip) in enumerate(zip(bufs, flips)):
        T.merge_view(b.t.data_ptr(), acc.t.data_ptr(), n, H, W, flip, k, K, L.stream_ptr())
        if k == 0 and after_first is not None:
            torch.cuda.synchronize()
            after_first()


def test_the_geometry_is_the_header_s():
    assert (T.BLOCK, T.UNROLL, T.MAX_GRID, T.MAX_VIEWS) == (R.BLOCK, R.UNROLL, R.MAX_GRID, R.MAX_VIEWS)
    assert R.grid(R.units("second-trip")) == T.MAX_GRID < -(-R.units("second-trip") // R.TRIP)


@pytest.mark.parametrize("flip", range(4))
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_flip(name, flip):
    rs = np.random.RandomState(flip + 4 * len(name))
    pat = _patterns(rs, R.SHAPES[name]["shape"])
    src, dst = Guard(name).set(pat.view(f32)), Guard(name)
    assert np.array_equal(src.bits(), pat)                        # the upload kept every pattern
    src.begin()
    dst.begin()
    n, H, W = src.shape
    T.flip_planes(src.t.data_ptr(), dst.t.data_ptr(), n, H, W, flip, L.stream_ptr())
    torch.cuda.synchronize()
    want = R.flip_planes(pat, flip)
    kref.assert_bits(dst.t, torch.from_numpy(want.view(f32)), what="flip[%s-%d]" % (name, flip))
    assert np.array_equal(dst.bits(), want), "flip[%s-%d]: a NaN payload changed" % (name, flip)
    dst.check("flip[%s-%d]: dst" % (name, flip))
    src.check("flip[%s-%d]: src" % (name, flip), written=False)


@pytest.mark.parametrize("name,K,first", [(n, K, first) for n in R.SHAPES for K, first in R.merge_cases(n)])
def test_merge(name, K, first):
    what = "merge[%s-%d-%d]" % (name, K, first)
    flips = R.view_flips(K, first)
    views = _views(name)[:K]
    bufs = [Guard(name).set(v).begin() for v in views]
    acc = Guard(name).begin()

    def first_view_is_a_copy():
        assert np.array_equal(acc.bits(), R.flip_planes(views[0], flips[0]).view(np.uint32)), what + ": view 0 is not the un-flipped input"

    _merge_on_device(acc, bufs, flips, first_view_is_a_copy)
    torch.cuda.synchronize()
    acc.check(what + ": acc")
    for b in bufs:
        b.check(what + ": logp", written=False)
    if K == 1:
        first_view_is_a_copy()                                     # stored untouched: nothing is subtracted
        return
    ref, lim = R.merge(views, flips)
    got = acc.t.cpu().numpy().astype(np.float64)
    assert np.isfinite(ref).all() and np.isfinite(got).all(), what + ": finite wherever every input is"
    assert (np.abs(np.stack([R.flip_planes(v, f) for v, f in zip(views, flips)]).astype(np.float64) - ref).max(0) > 90).any() or name == "one", \
        what + ": no pixel has views 100 nat apart"
    ratio = np.abs(got - ref) / lim
    WORST[what] = float(ratio.max())
    print("%s: worst error / bound %.3f (max |err| %.3e)" % (what, WORST[what], float(np.abs(got - ref).max())))
    i = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert WORST[what] <= 1.0, "%s: at %s got %r, fp64 %r, |err| %.3e > bound %.3e" % (what, i, got[i], ref[i], abs(got[i] - ref[i]), lim[i])


def _edge_pairs():
    """every ordered pair of these values that lae settles without a library call: (-inf, -inf), (-inf, x), (x, x), (+inf, x), NaN"""
    vals = np.array([-np.inf, np.inf, np.nan, -0.0, 0.0, -1.25, -100.0, -1e-38, -3e38, 1e-45, 2.5], dtype=f32)
    a, b = np.repeat(vals, len(vals)), np.tile(vals, len(vals))
    with np.errstate(all="ignore"):
        out, general = R.lae32(a, b)
    keep = ~general
    return a[keep], b[keep], out[keep]


@pytest.mark.parametrize("K", [2, 3])
def test_edge_rules_bit_for_bit(K):
    """K = 2: lae(a, b) - log 2;  K = 3, the third view -inf everywhere: lae(lae(a, b), -inf) - log 3 = lae(a, b) - log 3"""
    a, b, out = _edge_pairs()
    n = len(a)
    assert n >= 60 and np.isnan(out).any() and np.isinf(out).any() and np.isfinite(out).any()
    full = {}
    for nm, v in (("a", a), ("b", b), ("c", np.full(n, -np.inf, dtype=f32))):
        full[nm] = torch.full((n + 2 * MARGIN,), float("nan"), dtype=F32, device=DEV)
        full[nm][MARGIN:MARGIN + n] = torch.from_numpy(v)
    acc = torch.full((n + 2 * MARGIN,), 7.0, dtype=F32, device=DEV)
    before = acc.clone()
    for k, nm in enumerate(("a", "b", "c")[:K]):
        T.merge_view(full[nm][MARGIN:].data_ptr(), acc[MARGIN:].data_ptr(), 1, 1, n, 0, k, K, L.stream_ptr())
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        want = (out - R.log_views(K)).astype(f32)
    kref.assert_bits(acc[MARGIN:MARGIN + n], torch.from_numpy(want), what="edge rules, K=%d" % K)
    w = torch.zeros(n + 2 * MARGIN, dtype=torch.bool, device=DEV)
    w[MARGIN:MARGIN + n] = True
    kref.assert_untouched(acc, before, w, "edge rules: acc")
    same = (a == b) & np.isfinite(a)
    assert same.any() and np.array_equal(want[same].view(np.uint32), ((a[same] + R.LN2_F32).astype(f32) - R.log_views(K)).astype(f32).view(np.uint32))


@pytest.mark.parametrize("name", ["odd", "vec20"])
def test_two_views_merge_the_same_in_either_order(name):
    views = _views(name)[:2]
    bufs = [Guard(name).set(v) for v in views]
    bits = []
    for order in ((0, 1), (1, 0)):
        acc = Guard(name)
        _merge_on_device(acc, [bufs[i] for i in order], [(1, 2)[i] for i in order])
        torch.cuda.synchronize()
        bits.append(acc.bits())
    assert np.array_equal(bits[0], bits[1]), "lae is symmetric: the order of two views must not show"
    assert not np.array_equal(bits[0], R.flip_planes(views[0], 1).view(np.uint32))


def test_a_captured_graph_replays_flip_copy_and_merge():
    """no launch argument depends on anything the device decides: flip, copy (flip 0) and a merge of two views capture as they are"""
    name = "vec20"
    n, H, W = R.SHAPES[name]["shape"]
    x, flipped, copied, acc = Guard(name), Guard(name), Guard(name), Guard(name)
    x.set(np.zeros((n, H, W), f32))
    torch.cuda.synchronize()

    def calls():
        s = L.stream_ptr()
        T.flip_planes(x.t.data_ptr(), flipped.t.data_ptr(), n, H, W, 3, s)
        T.flip_planes(flipped.t.data_ptr(), copied.t.data_ptr(), n, H, W, 0, s)
        T.merge_view(x.t.data_ptr(), acc.t.data_ptr(), n, H, W, 0, 0, 2, s)
        T.merge_view(copied.t.data_ptr(), acc.t.data_ptr(), n, H, W, 3, 1, 2, s)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls()
    torch.cuda.synchronize()
    assert bool(torch.isnan(acc.t).all()) and bool(torch.isnan(copied.t).all())        # the capture ran nothing
    for rep in range(2):
        x.set(_views(name)[rep])
        for b in (x, flipped, copied, acc):
            b.begin()
        graph.replay()
        torch.cuda.synchronize()
        replayed = [b.bits().copy() for b in (flipped, copied, acc)]
        for b in (flipped, copied, acc):
            b.check("replay %d" % rep)
            b.t.fill_(float("nan"))
        x.check("replay %d: x" % rep, written=False)
        calls()
        torch.cuda.synchronize()
        for nm, r, b in zip(("flipped", "copied", "acc"), replayed, (flipped, copied, acc)):
            assert np.array_equal(r, b.bits()), "replay %d: %s differs from the eager calls" % (rep, nm)
        assert np.array_equal(replayed[0], R.flip_planes(_views(name)[rep], 3).view(np.uint32))
        # flipped twice, every element meets itself: lae(v, v) - log 2
        v = _views(name)[rep]
        want = ((v + R.LN2_F32).astype(f32) - R.log_views(2)).astype(f32)
        assert np.array_equal(replayed[2], want.view(np.uint32))
