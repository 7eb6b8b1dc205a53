"""libubresnet_ema.so on the device, exactly: the decision of ube_advance against tests/ema_ref.py field for field, ube_update
against the numpy replay over whole buffers bit for bit (sizes from the header's geometry, edge values in both operands, a held
update that touches nothing), ube_update_segs over a table of small runs with their neighbours watched, and the two exchanges on
arbitrary bit patterns.  Every buffer lies between guard margins that are checked."""
import numpy as np
import pytest
import torch

import ema_ref as R
import kref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _ema as E
    from ubresnet_amd import _lib as L

DEV = "cuda"
F32 = torch.float32
f32 = np.float32
SIZES = R.flat_sizes()


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


def _new_ctl(updates=0):
    """a control block between two 256-byte margins of 0xA5, initialised by the library"""
    full = torch.full((R.CTL_BYTES + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    ctl = full[256:256 + R.CTL_BYTES]
    E.ctl_init(ctl.data_ptr(), updates, L.stream_ptr())
    return full, ctl


def _head(ctl):
    return E.read_ctl(ctl.cpu().numpy().tobytes())


def _margins_intact(full):
    assert bool((full[:256] == 0xA5).all()) and bool((full[-256:] == 0xA5).all()), "wrote outside the control block"


def _flag(value):
    """an optimizer's control block as far as ube_advance looks: an int32 at byte 20 of a 16-byte aligned block -> (block, address)"""
    blk = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    blk[R.APPLY_OFFSET // 4] = value
    return blk, blk.data_ptr() + R.APPLY_OFFSET


def _same_head(h, ref, what):
    got = (h.apply, f32(h.w).view(np.uint32), f32(h.d).view(np.uint32), h.reserved, h.updates, h.held)
    want = (ref.apply, f32(ref.w).view(np.uint32), f32(ref.d).view(np.uint32), 0, ref.updates, ref.held)
    assert got == want, "%s: control block %r, reference %r" % (what, got, want)


def _bits(t):
    return t.view(torch.int32)


def _rand_bits(rs, n):
    """n arbitrary 32-bit patterns as fp32 (NaNs with payloads, infinities, subnormals and both zeros among them)"""
    v = rs.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    v[:8] = [0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000000, 0x7f800000, 0x00000001, 0x807fffff][:min(n, 8)]
    return torch.from_numpy(v.view(np.int32).copy()).view(F32)


# ------------------------------------------------------------------------------------------------------------------------
# the control block and the decision
# ------------------------------------------------------------------------------------------------------------------------
def test_ctl_init_zeroes_the_block_and_seeds_the_count():
    full, ctl = _new_ctl(7)
    torch.cuda.synchronize()
    h = _head(ctl)
    assert (h.apply, h.w, h.d, h.reserved, h.updates, h.held) == (0, 0.0, 0.0, 0, 7, 0)
    raw = ctl.cpu().numpy().copy()
    raw[R.OFFSETS["updates"]:R.OFFSETS["updates"] + 8] = 0
    assert not raw.any(), "ube_ctl_init left a nonzero byte"
    _margins_intact(full)


@pytest.mark.parametrize(("decay", "warmup", "start"), [(0.999, 10, 0), (0.5, 2, 0), (0.9999, 0, 3), (0.0, 10, 0), (0.999, 10, 8985)])
def test_advance_follows_the_reference_field_for_field(decay, warmup, start):
    """applied, held and flagless calls in one sequence; (0.999, 10) from 8985 crosses the u at which the minimum changes sides"""
    assert warmup != 10 or decay != 0.999 or start == 0 or start < R.crossover(decay, warmup) < start + 12
    full, ctl = _new_ctl(start)
    ref = R.Ctl(start)
    script = [None, 1, 0, 0, -3, None, 1 << 30, 0, 1, 1, None, 1]
    for k, v in enumerate(script):
        if v is None:
            blk, addr = None, None
        else:
            blk, addr = _flag(v)
            before = blk.clone()
        E.advance(ctl.data_ptr(), addr, decay, warmup, L.stream_ptr())
        ref.advance(v, decay, warmup)
        torch.cuda.synchronize()
        _same_head(_head(ctl), ref, "call %d (flag %r)" % (k, v))
        if blk is not None:
            assert torch.equal(blk, before), "ube_advance wrote to the optimizer's block"
    assert (ref.updates, ref.held) == (start + 9, 3)
    _margins_intact(full)


# ------------------------------------------------------------------------------------------------------------------------
# ube_update
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_update_is_the_numpy_replay_over_five_updates(n):
    """warm-up 3 towards 0.9: the weight differs from update to update (2/3, 1/2, 2/5, 1/3, 2/7)"""
    decay, warmup = 0.9, 3
    rs = np.random.RandomState(n % 65521)
    host = rs.standard_normal(n).astype(f32)
    host[::7] *= f32(1e-38)                                 # some subnormal and near-subnormal operands
    s, p = Guard(n).set(host), Guard(n)
    full, ctl = _new_ctl()
    ref = R.Ctl()
    weights = []
    for k in range(5):
        hp = (rs.standard_normal(n) * (1.0 + k)).astype(f32)
        hp[3::11] = host[3::11]                             # param == shadow here and there
        p.set(hp).begin()
        s.begin()
        E.advance(ctl.data_ptr(), None, decay, warmup, L.stream_ptr())
        E.update(s.t.data_ptr(), p.t.data_ptr(), n, ctl.data_ptr(), L.stream_ptr())
        ref.advance(None, decay, warmup)
        host = R.update(host, hp, ref.w)
        weights.append(float(ref.w))
        torch.cuda.synchronize()
        kref.assert_bits(s.t, torch.from_numpy(host), what="n=%d update %d: shadow" % (n, k + 1))
        s.check("n=%d update %d: shadow" % (n, k + 1))
        p.check("n=%d update %d: param" % (n, k + 1), written=False)
    assert weights[:3] == [float(f32(1.0 - 1.0 / 3.0)), 0.5, float(f32(1.0 - 3.0 / 5.0))] and weights == sorted(set(weights), reverse=True)
    _same_head(_head(ctl), ref, "after five updates")
    _margins_intact(full)
    assert R.grid(n) == min(-(-(n // 4) // R.TRIP), R.MAX_GRID)


def test_the_sizes_cover_the_paths_of_the_launch():
    t = R.TRIP
    assert SIZES[:4] == [4, 4 * (t - 1), 4 * t, 4 * (t + 1)] and [R.grid(n) for n in SIZES[:4]] == [1, 1, 1, 2]
    ragged, past = SIZES[4], SIZES[5]
    g = R.grid(ragged)
    assert 1 < g < R.MAX_GRID and (ragged // 4) % (g * R.BLOCK) != 0 and ragged // 4 < g * t          # one grid trip, its last round partly filled
    assert R.grid(past) == R.MAX_GRID and past // 4 == R.MAX_GRID * t + 37                            # a second trip of 37 units


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.999])
def test_update_on_edge_values_in_both_operands(decay):
    """every pair of kref.edge_table(float32) values: subnormals, both zeros, infinities, NaN, the largest finite value"""
    edge = kref.edge_values(F32).numpy()
    k = len(edge)
    hs, hp = np.repeat(edge, k), np.tile(edge, k)
    n = (len(hs) + 3) // 4 * 4
    hs, hp = np.concatenate([hs, np.ones(n - len(hs), f32)]), np.concatenate([hp, np.ones(n - len(hp), f32)])
    s, p = Guard(n, fill=1.0).set(hs).begin(), Guard(n, fill=1.0).set(hp).begin()
    full, ctl = _new_ctl()
    E.advance(ctl.data_ptr(), None, decay, 0, L.stream_ptr())
    E.update(s.t.data_ptr(), p.t.data_ptr(), n, ctl.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    w, _ = R.schedule(decay, 0, 0)
    want = R.update(hs, hp, w)
    with np.errstate(all="ignore"):
        assert np.isnan(want).any() and np.isinf(want).any() and ((want != 0) & (np.abs(want) < f32(1.1754944e-38))).any()
    kref.assert_bits(s.t, torch.from_numpy(want), what="edge values, decay %g" % decay)           # finite: the bits; NaN: NaN
    s.check("edge values: shadow")
    p.check("edge values: param", written=False)


@pytest.mark.parametrize("n", [SIZES[0], SIZES[4]])
def test_a_held_update_touches_neither_buffer(n):
    rs = np.random.RandomState(5)
    s, p = Guard(n), Guard(n)
    s.t.copy_(_rand_bits(rs, n))
    p.t.copy_(_rand_bits(rs, n))
    full, ctl = _new_ctl(4)
    E.advance(ctl.data_ptr(), None, 0.5, 0, L.stream_ptr())            # an applied update first: w is set and apply is 1
    blk, addr = _flag(0)
    s.begin()
    p.begin()
    E.advance(ctl.data_ptr(), addr, 0.5, 0, L.stream_ptr())
    E.update(s.t.data_ptr(), p.t.data_ptr(), n, ctl.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    s.check("held: shadow", written=False)
    p.check("held: param", written=False)
    h = _head(ctl)
    assert (h.apply, h.updates, h.held, h.w) == (0, 5, 1, 0.5)
    blk[R.APPLY_OFFSET // 4] = 2                                       # the same launches with the flag up do act
    E.advance(ctl.data_ptr(), addr, 0.5, 0, L.stream_ptr())
    E.update(s.t.data_ptr(), p.t.data_ptr(), n, ctl.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    assert not torch.equal(_bits(s.full), _bits(s.before))
    h = _head(ctl)
    assert (h.apply, h.updates, h.held) == (1, 6, 1)
    _margins_intact(full)


# ------------------------------------------------------------------------------------------------------------------------
# the table calls
# ------------------------------------------------------------------------------------------------------------------------
def _seg_layout(counts, gap=1):
    """runs of these lengths in one buffer, `gap` watched floats between neighbours and a 64-float margin at either end: the runs
    start on 4-byte boundaries only -> (offsets, total length)"""
    offs, at = [], 64
    for c in counts:
        offs.append(at)
        at += c + gap
    return offs, at - gap + 64


def _seg_buffers(counts, rs, bits=False):
    offs, total = _seg_layout(counts)
    mk = (lambda: _rand_bits(rs, total)) if bits else (lambda: torch.from_numpy(rs.standard_normal(total).astype(f32)))
    shadow, live = mk().to(DEV), mk().to(DEV)
    table = E.seg_table([shadow.data_ptr() + 4 * o for o in offs], [live.data_ptr() + 4 * o for o in offs], counts)
    dev_table = torch.from_numpy(table.view(np.int64).reshape(-1, 4).copy()).to(DEV)
    inside = torch.zeros(total, dtype=torch.bool, device=DEV)
    for o, c in zip(offs, counts):
        inside[o:o + c] = True
    return shadow, live, dev_table, inside, offs


@pytest.mark.parametrize("counts", [[1, 3, 16, 257], [2] * (R.SEG_GRID + 44) + [R.BLOCK + 1]], ids=["1-3-16-257", "more-rows-than-workgroups"])
def test_update_segs_is_the_replay_on_every_run_and_spares_the_neighbours(counts):
    rs = np.random.RandomState(len(counts))
    shadow, live, table, inside, offs = _seg_buffers(counts, rs)
    edge = kref.edge_values(F32)
    o, c = offs[-1], counts[-1]
    shadow[o:o + len(edge)] = edge.to(DEV)                       # edge values in the long run, against ordinary values and each other
    live[o + 7:o + 7 + len(edge)] = edge.to(DEV)
    full, ctl = _new_ctl()
    ref = R.Ctl()
    host_s, host_l = shadow.cpu().numpy().copy(), live.cpu().numpy().copy()
    s0, l0 = shadow.clone(), live.clone()
    blk, addr = _flag(1)
    for k, flag in enumerate([1, 1, 0, 1]):
        blk[R.APPLY_OFFSET // 4] = flag
        E.advance(ctl.data_ptr(), addr, 0.9, 3, L.stream_ptr())
        E.update_segs(table.data_ptr(), len(counts), ctl.data_ptr(), L.stream_ptr())
        if ref.advance(flag, 0.9, 3):
            for o, c in zip(offs, counts):
                host_s[o:o + c] = R.update(host_s[o:o + c], host_l[o:o + c], ref.w)
        torch.cuda.synchronize()
        kref.assert_bits(shadow, torch.from_numpy(host_s), what="update_segs call %d" % (k + 1))
        kref.assert_untouched(shadow, s0, inside, "update_segs call %d: shadow" % (k + 1))
        kref.assert_untouched(live, l0, None, "update_segs call %d: live" % (k + 1))
    h = _head(ctl)
    assert (h.updates, h.held) == (3, 1)
    assert not torch.equal(_bits(shadow), _bits(s0))
    _margins_intact(full)


@pytest.mark.parametrize("counts", [[1, 3, 16, 257], [2] * (R.SEG_GRID + 44) + [R.BLOCK + 1]], ids=["1-3-16-257", "more-rows-than-workgroups"])
def test_swap_segs_exchanges_bit_patterns_and_a_second_call_restores(counts):
    rs = np.random.RandomState(100 + len(counts))
    shadow, live, table, inside, offs = _seg_buffers(counts, rs, bits=True)
    special = _rand_bits(rs, 8).to(DEV)                          # NaNs with payloads, -0, an infinity, subnormals: inside the last run
    shadow[offs[-1] + 1:offs[-1] + 9] = special
    live[offs[-1] + 5:offs[-1] + 13] = special
    s0, l0 = shadow.clone(), live.clone()
    E.swap_segs(table.data_ptr(), len(counts), L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(shadow), torch.where(inside, _bits(l0), _bits(s0))), "shadow is not live's bits inside the runs and its own outside"
    assert torch.equal(_bits(live), torch.where(inside, _bits(s0), _bits(l0)))
    assert bool(torch.isnan(s0[inside]).any()) and not torch.equal(_bits(shadow), _bits(s0))
    E.swap_segs(table.data_ptr(), len(counts), L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(shadow), _bits(s0)) and torch.equal(_bits(live), _bits(l0))


# ------------------------------------------------------------------------------------------------------------------------
# ube_swap
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_bit_patterns_and_a_second_call_restores(n):
    rs = np.random.RandomState(n % 65519)
    a, b = Guard(n), Guard(n)
    a.t.copy_(_rand_bits(rs, n))
    b.t.copy_(_rand_bits(rs, n))
    a.begin()
    b.begin()
    a0, b0 = a.t.clone(), b.t.clone()
    E.swap(a.t.data_ptr(), b.t.data_ptr(), n, L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.t), _bits(b0)) and torch.equal(_bits(b.t), _bits(a0)), "n=%d: not exchanged bit for bit" % n
    assert int(_bits(a0)[0]) == 0x7fc00001 and int(_bits(a.t)[0]) == int(_bits(b0)[0])                  # a NaN payload went across
    a.check("n=%d swap: a" % n)
    b.check("n=%d swap: b" % n)
    E.swap(a.t.data_ptr(), b.t.data_ptr(), n, L.stream_ptr())
    torch.cuda.synchronize()
    a.check("n=%d swap back: a" % n, written=False)
    b.check("n=%d swap back: b" % n, written=False)
