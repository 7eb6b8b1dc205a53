"""Every launch of the HBM-bound streaming kernels (csrc/ubr_elem.hip, csrc/ubr_head.hip) the product makes -- block tail forward
and backward, BatchNorm backward, max-pool, channel sums, stem expansion, log-softmax backward, the NLL loss pair -- at its real
shape, strides and aliasing, against the float64 references of tests/kref.py on exact operands: bit for bit (only
logsoftmax_bwd, which calls expf, is held to a derived bound).

The legs of test_gpu_kernels_exact.py run once with the operators wrapped; each distinct call is replayed in
NaN-guarded buffers of the recorded layout, and nothing outside the output views may change (the bytes beyond C in each
pixel of a sliced view included).  EXTRA_CASES are shapes the legs do not produce (odd max-pool extents, ties on a sliced
view, non-power-of-two unit counts, a partial last trip under the workgroup cap, every flush form / template switch / partial
trip of the one-pass frozen-BatchNorm kernels, the masked two-pass fallback) and a dozen of the captured ones as plain
cases.  The frozen and mixed legs also assert WHICH kernels the step takes.  A table row is printed per case."""
import inspect
import time

import pytest
import torch

import kref
from kref import ESZ, TV, Buffers
from test_gpu_kernels_exact import _leg

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import ops, plan
    from ubresnet_amd.ops import Affine

DEV = "cuda"
D = torch.float64
NS, RS = kref.STAT_SLOTS, kref.RED_SLOTS

# operator -> its NHWC view arguments
VIEWS = {
    "block_tail_fwd": ("c2", "sc", "out"), "block_tail_fwd_fin": ("c2", "sc", "out"),
    "block_tail_bwd_reduce": ("go", "go2", "out", "c2", "cb"),
    "block_tail_bwd_apply": ("go", "go2", "out", "c2", "cb", "g_c2", "g_sc"),
    "block_tail_bwd_apply_fin": ("go", "go2", "c2", "cb", "g_c2", "g_sc"),
    "bn_bwd_reduce": ("ga", "ga2", "c"), "bn_bwd_apply": ("ga", "ga2", "c", "gc"), "bn_bwd_apply_fin": ("ga", "ga2", "c", "gc"),
    "block_tail_bwd_frozen": ("go", "go2", "c2", "cb", "g_c2", "g_sc"), "bn_bwd_frozen": ("ga", "ga2", "c", "gc"),
    "maxpool_fwd": ("x", "pooled", "xcopy"), "maxpool_bwd": ("x", "g_pooled", "g_extra", "gx"),
    "channel_sum": ("g",), "stem_expand": ("out",), "logsoftmax_bwd": ("g_logits",),
    "pixelwise_nll_fwd": (), "pixelwise_nll_bwd": (),
}
OUT_VIEWS = {"block_tail_fwd": ("out",), "block_tail_fwd_fin": ("out",), "block_tail_bwd_apply": ("g_c2", "g_sc"),
             "block_tail_bwd_apply_fin": ("g_c2", "g_sc"), "bn_bwd_apply": ("gc",), "bn_bwd_apply_fin": ("gc",),
             "block_tail_bwd_frozen": ("g_c2", "g_sc"), "bn_bwd_frozen": ("gc",),
             "maxpool_fwd": ("pooled", "xcopy"), "maxpool_bwd": ("gx",), "stem_expand": ("out",), "logsoftmax_bwd": ("g_logits",)}
# what the headline bf16 train step must keep calling (ubresnet_amd/engine.py: fused finalizes, masked tails, saved arg-max)
HEADLINE_OPS = ("block_tail_fwd_fin", "block_tail_bwd_reduce", "block_tail_bwd_apply_fin", "bn_bwd_reduce", "bn_bwd_apply_fin",
                "maxpool_fwd", "maxpool_bwd", "channel_sum", "stem_expand", "logsoftmax_bwd", "pixelwise_nll_fwd", "pixelwise_nll_bwd")
HEADLINE_SLICED = ("block_tail_fwd_fin", "block_tail_bwd_apply_fin", "maxpool_fwd")
# a step whose BatchNorm sites are all frozen takes the one-pass kernels at every site, and no two-pass kernel anywhere
FROZEN_OPS = ("bn_bwd_frozen", "block_tail_bwd_frozen")
TWO_PASS_OPS = ("bn_bwd_reduce", "bn_bwd_apply", "bn_bwd_apply_fin", "block_tail_bwd_reduce", "block_tail_bwd_apply", "block_tail_bwd_apply_fin")

if torch.cuda.is_available():
    _SIGS = {n: inspect.signature(getattr(ops, n)) for n in VIEWS}
    _ORIG = {n: getattr(ops, n) for n in VIEWS}


# ------------------------------------------------------------------------------------------------------------------
# capture
# ------------------------------------------------------------------------------------------------------------------
def _record(op, args, kwargs):
    b = _SIGS[op].bind(*args, **kwargs)
    b.apply_defaults()
    a = dict(b.arguments)
    for n, v in list(a.items()):
        if n in VIEWS[op]:
            a[n] = TV(v) if v is not None else None
        elif isinstance(v, torch.Tensor):
            a[n] = ("t", str(v.dtype), tuple(v.shape))
        elif isinstance(v, Affine):
            a[n] = ("affine", tuple(v.lo.float().cpu().tolist()))
        elif isinstance(v, L.BnFwdFin):
            a[n] = ("fin", round(float(v.momentum), 6), float(v.eps), bool(v.running_mean))
    return {"op": op, "a": a}


def _signature(rec):
    """dedup key: everything but addresses (views keep their offsets inside a storage group and their 256-byte alignment)"""
    a = rec["a"]
    views = [v for v in a.values() if isinstance(v, TV)]
    gids = {}
    for v in views:
        gids.setdefault(v.gid, min(w.ptr for w in views if w.gid == v.gid))
    parts = [rec["op"]]
    for k in sorted(a):
        v = a[k]
        if isinstance(v, TV):
            parts.append((k, v.key(gids[v.gid]), list(gids).index(v.gid), v.ptr % 256))
        else:
            parts.append((k, v))
    return repr(parts)


class Capture:
    def __init__(self, monkeypatch):
        self.calls = []
        for n in VIEWS:
            monkeypatch.setattr(ops, n, self._wrap(n))

    def _wrap(self, n):
        def f(*args, **kw):
            self.calls.append(_record(n, args, kw))
            return _ORIG[n](*args, **kw)
        return f

    def distinct(self):
        seen = {}
        for r in self.calls:
            seen.setdefault(_signature(r), r)
        return list(seen.values())


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
_seed = [5000]


def _next_seed():
    _seed[0] += 13
    return _seed[0]


def _pick(vals, n, dtype=torch.float32):
    g = torch.Generator().manual_seed(_next_seed())
    return torch.tensor(vals, dtype=dtype)[torch.randint(0, len(vals), (n,), generator=g)].to(DEV)


def _fill(view, exp, density=None):
    npix = view.shape[0] * view.shape[1] * view.shape[2]
    d = density if density is not None else (0.3 if npix <= (1 << 18) else 0.12)
    view.copy_(kref.exact_operands(tuple(view.shape), view.dtype, density=d, seed=_next_seed(), exp=exp, device=DEV))
    return view.clone()


class Guard:
    """a flat buffer of n elements between two 64-element margins that must keep their contents"""

    def __init__(self, n, dtype, fill):
        self.full = torch.full((n + 128,), fill, dtype=dtype, device=DEV)
        self.t = self.full[64:64 + n]
        self.n = n

    def begin(self):
        self.before = self.full.clone()

    def check(self, what, written=True):
        w = torch.zeros(self.n + 128, dtype=torch.bool, device=DEV)
        if written:
            w[64:64 + self.n] = True
        kref.assert_untouched(self.full, self.before, w, what)


def _geom(v):
    N, H, W, C = v.shape
    cpu = kref.CPU[v.dtype]
    return N * H * W, C, cpu, C // cpu


def _bn_vectors(C):
    """(mean, scale, shift, invstd) of a BatchNorm site, exact on exact operands"""
    return _pick([-1., 0., 1.], C), _pick([0.5, 1., 2.], C), _pick([-1., 0., 1.], C), _pick([0.5, 1., 2.], C)


def _tvs(a, op):
    return [a[n] for n in VIEWS[op] if a.get(n) is not None]


def _begin(B, a, op, guards=()):
    snap = B.snapshot()
    for n in OUT_VIEWS.get(op, ()):
        if a.get(n) is not None:
            B.mark_written(a[n])
    for g in guards:
        g.begin()
    return snap


def _stripes(total, first=RS, rows=NS):
    """[rows][n] fp64 whose first `first` rows sum to `total` exactly (quarters and halves of it), the others zero"""
    w = torch.tensor([0.5, 0.0, 0.25, -0.25, 0.0, 0.25, 0.25, 0.0], dtype=D, device=DEV)[:first]
    out = torch.zeros((rows, total.numel()), dtype=D, device=DEV)
    out[:first] = w.view(-1, 1) * total.double().view(1, -1)
    return out


def _red_guard(n):
    """a reduce pass's accumulator [UBR_STAT_SLOTS][n] with nonzero exact contents everywhere (they must be added to)"""
    g = Guard(NS * n, D, 0.0)
    g.t.copy_(kref.exact_operands((NS * n,), D, density=0.7, seed=_next_seed(), device=DEV, maxmag=8))
    return g, g.t.clone().view(NS, n)


def _check_red(g, init, slots, refs, units, what):
    """stripes >= slots unchanged; the first `slots` stripes grew by exactly the reference sums (refs: [(sum, abs)], concatenated)"""
    now = g.t.view(NS, -1)
    assert torch.equal(now[slots:], init[slots:]), "%s: stripes beyond the first %d changed" % (what, slots)
    got = (now[:slots] - init[:slots]).sum(0)
    off = 0
    for (ref, ab), unit in zip(refs, units):
        n = ref.numel()
        kref.assert_sums_exact(got[off:off + n], ref, ab, unit, what)
        off += n
    g.check(what)


# ------------------------------------------------------------------------------------------------------------------
# replays: each returns (result, workgroups of the documented grid rule)
# ------------------------------------------------------------------------------------------------------------------
def replay_tail_fwd(a, op):
    B = Buffers(_tvs(a, op))
    c2v, scv, outv = B.view(a["c2"]), B.view(a["sc"]), B.view(a["out"])
    npix, C, cpu, CU = _geom(c2v)
    dt = c2v.dtype
    fin = op == "block_tail_fwd_fin"
    byp = (a["fin_b"] if fin else a["mean_b"]) is not None
    res = "exact"
    for mom in ((0.1, None) if fin else (0,)):
        c2 = _fill(c2v, 0, 0.6 if npix <= (1 << 18) else None)
        sc = _fill(scv, -1)
        mask = Guard(npix * CU, torch.uint8, 0xA5) if a["relu_mask"] is not None else None
        guards = [mask] if mask else []
        if not fin:
            m2, s2, t2, _ = _bn_vectors(C)
            mb, sb, tb, _ = _bn_vectors(C) if byp else (None,) * 4
            snap = _begin(B, a, op, guards)
            _ORIG[op](c2v, m2, s2, t2, scv, mb, sb, tb, outv, relu_mask=mask.t if mask else None)
        else:
            count = float(a["count"])
            sites, keep = [], []
            for spec in (a["fin2"], a["fin_b"]):
                if spec is None:
                    sites.append(None)
                    continue
                m, var = _pick([-1., 0., 1.], C, D), _pick([0.0, 0.75, 3.75], C, D)          # eps = 0.25: invstd in {2, 1, 0.5}
                stats = torch.cat([_stripes(count * m), _stripes(count * (var + m * m))], 1).contiguous()
                bn = torch.nn.BatchNorm2d(C, eps=0.25, momentum=mom, track_running_stats=spec[3]).to(DEV)
                bn.weight.data.copy_(_pick([0.5, 1., 2.], C))
                bn.bias.data.copy_(_pick([-1., 0., 1.], C))
                if spec[3]:
                    bn.running_mean.copy_(_pick([-0.5, 0., 0.5], C))
                    bn.running_var.copy_(_pick([0.5, 1., 2.], C))
                    bn.num_batches_tracked.fill_(3)
                vec = [Guard(C, torch.float32, float("nan")) for _ in range(4)]
                guards += vec
                momentum = float(torch.tensor(0.25 if mom is None else mom, dtype=torch.float32))     # None: 1 / (3 + 1)
                exp = kref.bn_finalize_ref(stats[:RS, :C].sum(0), stats[:RS, C:].sum(0), count, bn.weight.data, bn.bias.data, 0.25,
                                           bn.running_mean.clone() if spec[3] else None, bn.running_var.clone() if spec[3] else None, momentum)
                f = ops.bn_fwd_fin(stats.view(-1), bn, *[v.t for v in vec])
                sites.append((f, exp, vec, bn))
                keep.append(stats)
            snap = _begin(B, a, op, guards)
            _ORIG[op](c2v, sites[0][0], scv, sites[1][0] if byp else None, count, outv, relu_mask=mask.t if mask else None)
            torch.cuda.synchronize()
            for nm, site in zip(("bn2", "bnpass"), sites):
                if site is None:
                    continue
                f, exp, vec, bn = site
                for k, what in enumerate(("scale", "shift", "mean", "invstd")):
                    assert torch.equal(vec[k].t, exp[k]), "fwd_fin %s %s (momentum %s) differs from ubr_bn_finalize's formula" % (nm, what, mom)
                if exp[4] is not None:
                    assert torch.equal(bn.running_mean, exp[4]) and torch.equal(bn.running_var, exp[5]), \
                        "fwd_fin %s running statistics (momentum %s)" % (nm, mom)
                    assert int(bn.num_batches_tracked) == 4, "fwd_fin %s batch counter" % nm
            (m2, s2, t2), (mb, sb, tb) = [(e[1][2], e[1][0], e[1][1]) if e else (None,) * 3 for e in sites]
        torch.cuda.synchronize()
        ref = kref.tail_fwd_ref(c2, m2, s2, t2, sc, mb, sb, tb)
        kref.assert_exact(outv, ref, dt, ref.abs(), 0.125, op)
        if mask:
            want = kref.mask_pack(kref.round_to(ref, dt) > 0, cpu)
            assert torch.equal(mask.t, want), "%s: %d mask bytes differ from [stored output > 0]" % (op, int((mask.t != want).sum()))
        for g in guards:
            g.check(op)
        B.check_sentinel(snap, op)
    return res, kref.pick_blocks(npix, CU, 1024 if fin else 2048, 4)


def _gate(a, B, shape, cpu):
    """the final ReLU's gate of a block tail's backward, as recorded: mask bytes, or the block output"""
    npix = shape[0] * shape[1] * shape[2]
    if a.get("relu_mask") is not None:
        m = torch.randint(0, 256, (npix * (shape[3] // cpu),), dtype=torch.uint8, device=DEV,
                          generator=torch.Generator(device=DEV).manual_seed(_next_seed()))
        return m, None, kref.mask_unpack(m, shape, cpu)
    outv = B.view(a["out"])
    o = _fill(outv, 0, 0.5)
    return None, outv, o > 0


def _fin_red(C, count):
    """`red` of an apply pass with the finalize fused: count * k over the stripes -> (red [32*2C], k1, k2)"""
    k = _pick([-0.5, -0.25, 0., 0.25, 0.5], 2 * C, D)
    return _stripes(count * k).view(-1).contiguous(), k[:C].float(), k[C:].float()


def _check_dgrads(red, C, dgamma, dbeta, what):
    s = red.view(NS, 2 * C)[:RS].sum(0)
    for g, ref, nm in ((dbeta, s[:C], "dbeta"), (dgamma, s[C:], "dgamma")):
        if g is not None:
            assert torch.equal(g.t, ref.float()), "%s: %s differs from ubr_bn_bwd_finalize's formula" % (what, nm)
            g.check(what)


def replay_tail_bwd(a, op):
    B = Buffers(_tvs(a, op))
    c2v = B.view(a["c2"])
    npix, C, cpu, CU = _geom(c2v)
    dt = c2v.dtype
    go = _fill(B.view(a["go"]), -1)
    go2 = _fill(B.view(a["go2"]), -1) if a["go2"] is not None else None
    c2 = _fill(c2v, 0, 0.6)
    byp = a["cb"] is not None
    cb = _fill(B.view(a["cb"]), 0, 0.6) if byp else None
    mask, outv, positive = _gate(a, B, c2v.shape, cpu)
    m2, s2, t2, i2 = _bn_vectors(C)
    mb, sb, _, ib = _bn_vectors(C) if byp else (None,) * 4
    gz, gy2, xh2, xhb = kref.tail_bwd_ref(go, go2, positive, c2, s2, t2, m2, i2, cb, mb, ib)
    V = lambda n: B.view(a[n]) if a.get(n) is not None else None
    if op == "block_tail_bwd_reduce":
        r2, init2 = _red_guard(2 * C)
        rb, initb = _red_guard(2 * C) if byp else (None, None)
        snap = _begin(B, a, op, [g for g in (r2, rb) if g])
        _ORIG[op](V("go"), V("go2"), outv, c2v, s2, t2, m2, i2, V("cb"), mb, ib, r2.t, rb.t if byp else None, relu_mask=mask)
        torch.cuda.synchronize()
        s, sx, a1, a2 = kref.reduce_ref(gy2, xh2)
        _check_red(r2, init2, RS, [(s, a1), (sx, a2)], (0.5, 0.25), op + " (bn2)")
        if byp:
            s, sx, a1, a2 = kref.reduce_ref(gz, xhb)
            _check_red(rb, initb, RS, [(s, a1), (sx, a2)], (0.5, 0.25), op + " (bnpass)")
        B.check_sentinel(snap, op)
        return "exact", kref.pick_blocks(npix, CU, 512, 8)
    guards = []
    if op == "block_tail_bwd_apply":
        k = _pick([-0.5, -0.25, 0., 0.25, 0.5], 4 * C)
        k12, k22, k1b, k2b = k[:C], k[C:2 * C], k[2 * C:3 * C], k[3 * C:]
        snap = _begin(B, a, op)
        _ORIG[op](V("go"), V("go2"), outv, c2v, s2, t2, m2, i2, k12, k22, V("cb"), sb, mb, ib, k1b if byp else None, k2b if byp else None,
                  V("g_c2"), V("g_sc"), relu_mask=mask)
    else:
        count = float(a["count"])
        red2, k12, k22 = _fin_red(C, count)
        redb, k1b, k2b = _fin_red(C, count) if byp else (None, None, None)
        dg = {n: (Guard(C, torch.float32, float("nan")) if a[n] is not None else None) for n in ("dgamma2", "dbeta2", "dgamma_b", "dbeta_b")}
        guards = [g for g in dg.values() if g]
        snap = _begin(B, a, op, guards)
        T = lambda n: dg[n].t if dg[n] else None
        _ORIG[op](V("go"), V("go2"), mask, c2v, s2, t2, m2, i2, red2, T("dgamma2"), T("dbeta2"), V("cb"), sb, mb, ib, redb,
                  T("dgamma_b"), T("dbeta_b"), count, V("g_c2"), V("g_sc"))
        torch.cuda.synchronize()
        _check_dgrads(red2, C, dg["dgamma2"], dg["dbeta2"], op + " (bn2)")
        if byp:
            _check_dgrads(redb, C, dg["dgamma_b"], dg["dbeta_b"], op + " (bnpass)")
    torch.cuda.synchronize()
    ref = kref.apply_ref(gy2, xh2, s2, k12, k22)
    kref.assert_exact(V("g_c2"), ref, dt, ref.abs(), 2.0 ** -5, op + " g_c2")
    if a.get("g_sc") is not None:
        ref = kref.apply_ref(gz, xhb, sb, k1b, k2b) if byp else gz
        kref.assert_exact(V("g_sc"), ref, dt, ref.abs(), 2.0 ** -5, op + " g_sc")
    else:
        assert not byp, "a bypass block always writes g_cb"
    B.check_sentinel(snap, op)           # (with g_sc = None nothing but g_c2 may have changed)
    return "exact", kref.pick_blocks(npix, CU, 2048, 2)


def replay_bn_bwd(a, op):
    B = Buffers(_tvs(a, op))
    cv = B.view(a["c"])
    npix, C, cpu, CU = _geom(cv)
    dt = cv.dtype
    ga = _fill(B.view(a["ga"]), -1)
    ga2 = _fill(B.view(a["ga2"]), -1) if a["ga2"] is not None else None
    c = _fill(cv, 0, 0.6)
    mean, scale, shift, invstd = _bn_vectors(C)
    gy, xh = kref.bn_bwd_ref(ga, ga2, c, scale, shift, mean, invstd, a["relu"])
    V = lambda n: B.view(a[n]) if a.get(n) is not None else None
    if op == "bn_bwd_reduce":
        r, init = _red_guard(2 * C)
        snap = _begin(B, a, op, [r])
        _ORIG[op](V("ga"), V("ga2"), cv, scale, shift, mean, invstd, a["relu"], r.t)
        torch.cuda.synchronize()
        s, sx, a1, a2 = kref.reduce_ref(gy, xh)
        _check_red(r, init, RS, [(s, a1), (sx, a2)], (0.5, 0.25), op)
        B.check_sentinel(snap, op)
        return "exact", kref.pick_blocks(npix, CU, 512, 8)
    if op == "bn_bwd_apply":
        k = _pick([-0.5, -0.25, 0., 0.25, 0.5], 2 * C)
        k1, k2 = k[:C], k[C:]
        snap = _begin(B, a, op)
        _ORIG[op](V("ga"), V("ga2"), cv, scale, shift, mean, invstd, a["relu"], k1, k2, V("gc"))
    else:
        count = float(a["count"])
        red, k1, k2 = _fin_red(C, count)
        dgam = Guard(C, torch.float32, float("nan")) if a["dgamma"] is not None else None
        dbet = Guard(C, torch.float32, float("nan")) if a["dbeta"] is not None else None
        snap = _begin(B, a, op, [g for g in (dgam, dbet) if g])
        _ORIG[op](V("ga"), V("ga2"), cv, scale, shift, mean, invstd, a["relu"], red, count, dgam.t if dgam else None,
                  dbet.t if dbet else None, V("gc"))
        torch.cuda.synchronize()
        _check_dgrads(red, C, dgam, dbet, op)
    torch.cuda.synchronize()
    ref = kref.apply_ref(gy, xh, scale, k1, k2)
    kref.assert_exact(V("gc"), ref, dt, ref.abs(), 2.0 ** -5, op)
    B.check_sentinel(snap, op)
    return "exact", kref.pick_blocks(npix, CU, 2048, 4)


def replay_tail_bwd_frozen(a, op):
    """ubr_block_tail_bwd_frozen: both data gradients and both pairs of sums in one walk; the mask is an input"""
    B = Buffers(_tvs(a, op))
    c2v = B.view(a["c2"])
    npix, C, cpu, CU = _geom(c2v)
    dt = c2v.dtype
    go = _fill(B.view(a["go"]), -1)
    go2 = _fill(B.view(a["go2"]), -1) if a["go2"] is not None else None
    c2 = _fill(c2v, 0, 0.6)
    byp = a["cb"] is not None
    cb = _fill(B.view(a["cb"]), 0, 0.6) if byp else None
    mask = Guard(npix * CU, torch.uint8, 0)
    mask.t.copy_(torch.randint(0, 256, (npix * CU,), dtype=torch.uint8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(_next_seed())))
    m2, s2, t2, i2 = _bn_vectors(C)
    mb, sb, _, ib = _bn_vectors(C) if byp else (None,) * 4
    g_c2, g_sc, sums2, sumsb = kref.tail_bwd_frozen_ref(go, go2, kref.mask_unpack(mask.t, c2v.shape, cpu), c2, s2, t2, m2, i2, cb, sb, mb, ib)
    V = lambda n: B.view(a[n]) if a.get(n) is not None else None
    r2, init2 = _red_guard(2 * C)
    rb, initb = _red_guard(2 * C) if byp else (None, None)
    snap = _begin(B, a, op, [g for g in (mask, r2, rb) if g])
    _ORIG[op](V("go"), V("go2"), mask.t, c2v, s2, t2, m2, i2, r2.t, V("cb"), sb, mb, ib, rb.t if byp else None, V("g_c2"), V("g_sc"))
    torch.cuda.synchronize()
    kref.assert_exact(V("g_c2"), g_c2, dt, g_c2.abs(), 2.0 ** -5, op + " g_c2")
    if a.get("g_sc") is not None:
        kref.assert_exact(V("g_sc"), g_sc, dt, g_sc.abs(), 2.0 ** -5, op + " g_sc")
    else:
        assert not byp, "a bypass block always writes g_cb"
    _check_red(r2, init2, RS, sums2, (0.5, 0.25), op + " (bn2)")
    if byp:
        _check_red(rb, initb, RS, sumsb, (0.5, 0.25), op + " (bnpass)")
    mask.check(op + " (mask)", written=False)
    B.check_sentinel(snap, op)           # (with g_sc = None nothing but g_c2 and the stripes may have changed)
    return "exact", kref.pick_blocks(npix, CU, 512, 8)


def replay_bn_bwd_frozen(a, op):
    """ubr_bn_bwd_frozen: with `red` the data gradient and the sums in one walk; without, the data gradient alone"""
    B = Buffers(_tvs(a, op))
    cv = B.view(a["c"])
    npix, C, cpu, CU = _geom(cv)
    dt = cv.dtype
    ga = _fill(B.view(a["ga"]), -1)
    ga2 = _fill(B.view(a["ga2"]), -1) if a["ga2"] is not None else None
    c = _fill(cv, 0, 0.6)
    mean, scale, shift, invstd = _bn_vectors(C)
    gc, dbeta, dgamma = kref.bn_bwd_frozen_ref(ga, ga2, c, scale, shift, mean, invstd, a["relu"])
    V = lambda n: B.view(a[n]) if a.get(n) is not None else None
    r, init = _red_guard(2 * C) if a["red"] is not None else (None, None)
    snap = _begin(B, a, op, [r] if r else [])
    _ORIG[op](V("ga"), V("ga2"), cv, scale, shift, mean, invstd, a["relu"], r.t if r else None, V("gc"))
    torch.cuda.synchronize()
    kref.assert_exact(V("gc"), gc, dt, gc.abs(), 2.0 ** -5, op)
    if r:
        _check_red(r, init, RS, [dbeta, dgamma], (0.5, 0.25), op)
    B.check_sentinel(snap, op)           # (pure apply: nothing but gc may have changed)
    return "exact", kref.pick_blocks(npix, CU, 512, 8) if r else kref.pick_blocks(npix, CU, 2048, 4)


def _pool_xf(a, C):
    if a["xf"] is None:
        return None, None
    lo = torch.tensor(a["xf"][1][:C], dtype=torch.float32)
    assert bool(((lo == 0) | (lo <= -1e30)).all())
    v = kref.exact_affine(C, _next_seed(), device=DEV, relu=lo)
    return v, Affine(*v)


def replay_maxpool_fwd(a, op):
    B = Buffers(_tvs(a, op))
    xv, pv = B.view(a["x"]), B.view(a["pooled"])
    N, H, W, C = xv.shape
    dt, S = xv.dtype, a["stride"]
    x = _fill(xv, 0, 0.3)                      # sparse small integers: nearly every window holds ties
    xf_ref, xf = _pool_xf(a, C)
    am = Guard(pv.numel(), torch.uint8, 0xA5) if a["argmax"] is not None else None
    snap = _begin(B, a, op, [am] if am else [])
    _ORIG[op](xv, xf, pv, B.view(a["xcopy"]) if a["xcopy"] is not None else None, S, argmax=am.t.view(pv.shape) if am else None)
    torch.cuda.synchronize()
    pooled, idx, v = kref.maxpool_ref(x, xf_ref, S)
    kref.assert_exact(pv, pooled, dt, pooled.abs(), 0.5, op + " pooled")
    if a["xcopy"] is not None:
        kref.assert_exact(B.view(a["xcopy"]), v, dt, v.abs(), 0.5, op + " xcopy")
    if am:
        got = am.t.view(pv.shape).long()
        assert torch.equal(got, idx), "%s: %d arg-max entries are not the first maximum in scan order" % (op, int((got != idx).sum()))
        am.check(op)
    B.check_sentinel(snap, op)
    return "exact", kref.pick_blocks(pv.shape[0] * pv.shape[1] * pv.shape[2], C // kref.CPU[dt], 4096)


def replay_maxpool_bwd(a, op):
    B = Buffers(_tvs(a, op))
    xv, gpv, gxv = B.view(a["x"]), B.view(a["g_pooled"]), B.view(a["gx"])
    N, H, W, C = xv.shape
    dt, S = xv.dtype, a["stride"]
    x = _fill(xv, 0, 0.3)
    gp = _fill(gpv, -1, 0.5)
    ge = _fill(B.view(a["g_extra"]), -1, 0.5) if a["g_extra"] is not None else None
    xf_ref, xf = _pool_xf(a, C)
    _, idx, _ = kref.maxpool_ref(x, xf_ref, S)
    ref = kref.maxpool_bwd_ref(gp, idx, (H, W), S, ge)
    # stride 2: once through the saved arg-max (as recorded, when the engine keeps one) and once re-scanning the windows
    variants = [a["argmax"] is not None] if S == 1 else [True, False]
    for saved in variants:
        am = idx.to(torch.uint8).contiguous() if saved else None
        gxv.fill_(float("nan"))
        snap = _begin(B, a, op)
        _ORIG[op](xv, xf, gpv, B.view(a["g_extra"]) if ge is not None else None, gxv, S, argmax=am)
        torch.cuda.synchronize()
        what = "%s (%s)" % (op, "saved arg-max" if saved else "re-scan")
        kref.assert_exact(gxv, ref, dt, ref.abs(), 0.5, what)
        B.check_sentinel(snap, what)
    even = S == 2 and H % 2 == 0 and W % 2 == 0
    return "exact", kref.pick_blocks(gpv.shape[0] * gpv.shape[1] * gpv.shape[2] if even else N * H * W, C // kref.CPU[dt])


def replay_channel_sum(a, op):
    B = Buffers(_tvs(a, op))
    gv = B.view(a["g"])
    npix, C, cpu, CU = _geom(gv)
    g = _fill(gv, -1)
    r, init = _red_guard(C)
    snap = _begin(B, a, op, [r])
    _ORIG[op](gv, r.t)
    torch.cuda.synchronize()
    s, _, a1, _ = kref.reduce_ref(g.double())
    _check_red(r, init, NS, [(s, a1)], (0.5,), op)
    B.check_sentinel(snap, op)
    return "exact", kref.pick_blocks(npix, CU, 1024)


def replay_stem_expand(a, op):
    B = Buffers(_tvs(a, op))
    ov = B.view(a["out"])
    N, H, W, C16 = ov.shape
    x = kref.exact_operands((N, C16 // 16, H, W), torch.float32, density=0.5, seed=_next_seed(), exp=-1, zero_tiles=0, device=DEV)
    snap = _begin(B, a, op)
    _ORIG[op](x, ov)
    torch.cuda.synchronize()
    ref = kref.stem_expand_ref(x)
    kref.assert_exact(ov, ref, ov.dtype, ref.abs(), 0.5, op)
    assert float(ov.reshape(N, H, W, -1, 16)[..., 7:].abs().max()) == 0.0
    B.check_sentinel(snap, op)
    return "exact", min((x.numel() + 255) // 256, 8192)


def replay_logsoftmax_bwd(a, op):
    B = Buffers(_tvs(a, op))
    ov = B.view(a["g_logits"])
    _, _, shp = a["logp"]
    N, C, H, W = shp
    p = 2.0 ** -_pick([1., 2., 3., 4.], N * C * H * W, D).view(shp)          # dyadic probabilities
    g = kref.exact_operands(shp, D, density=0.4, seed=_next_seed(), exp=-2, zero_tiles=0, device=DEV)
    snap = _begin(B, a, op)
    _ORIG[op](g.float().contiguous(), p.log().float().contiguous(), ov)
    torch.cuda.synchronize()
    ref, lim = kref.logsoftmax_bwd_ref(g, p, ov.dtype)
    kref.assert_within(ov[..., :C], ref, lim, op)
    assert float(ov[..., C:].abs().max()) == 0.0, "%s: padded channels are not zero" % op
    B.check_sentinel(snap, op)
    return "bounded", min((N * H * W + 255) // 256, 4096)


def _nll_operands(shp, classw, ignore_index, n_bad=0):
    N, C, H, W = shp
    pred = -kref.exact_operands(shp, torch.float32, density=0.9, seed=_next_seed(), exp=-2, zero_tiles=0, device=DEV, maxmag=16).abs()
    gen = torch.Generator(device=DEV).manual_seed(_next_seed())
    tgt = torch.randint(0, C, (N, H, W), device=DEV, generator=gen)
    tgt[torch.rand((N, H, W), device=DEV, generator=gen) < 0.1] = ignore_index
    if n_bad:
        tgt.view(-1)[torch.randperm(tgt.numel(), device=DEV, generator=gen)[:n_bad]] = C + 2
    pw = _pick([0., 0.5, 1., 2., 4.], N * H * W).view(N, H, W)
    cw = _pick([0.5, 1., 2.], C) if classw else None
    return pred, tgt, pw, cw


def replay_nll_fwd(a, op, n_bad=0):
    shp = a["predict"][2]
    pred, tgt, pw, cw = _nll_operands(shp, a["classw"] is not None, a["ignore_index"], n_bad)
    acc = Guard(NS + 1, D, 0.0)
    acc.begin()
    _ORIG[op](pred, tgt, pw, cw, a["ignore_index"], acc.t, bad=acc.t[NS:] if a["bad"] is not None else None)
    torch.cuda.synchronize()
    s, ab, bad, _, _ = kref.nll_ref(pred, tgt, pw, cw, a["ignore_index"])
    kref.assert_sums_exact(acc.t[:NS].sum().view(1), s.view(1), ab.view(1) * 2.0 ** -29, 2.0 ** -5, op)    # fp64 accumulator: 2^53 units
    if a["bad"] is not None:
        assert int(acc.t[NS:].view(torch.int64)) == bad == n_bad
    acc.check(op)
    return "exact", min((tgt.numel() + 255) // 256, 1024)


def replay_nll_bwd(a, op):
    shp = tuple(a["shape"])
    pred, tgt, pw, cw = _nll_operands(shp, a["classw"] is not None, a["ignore_index"])
    pw = torch.where(pw == 0, pw, torch.ones_like(pw)) * _pick([0.5, 1., 2., 4.], pw.numel()).view(pw.shape)     # 0 or a power of two
    g = Guard(pred.numel(), torch.float32, float("nan"))
    g.begin()
    gl = torch.full((), 0.5, device=DEV)
    _ORIG[op](gl, tgt, pw, cw, a["ignore_index"], shp, g.t.view(shp))
    torch.cuda.synchronize()
    ref = kref.nll_bwd_ref(0.5, tgt, pw, cw, a["ignore_index"], shp[1])
    kref.assert_exact(g.t.view(shp), ref, torch.float32, what=op)
    g.check(op)
    return "exact", min((tgt.numel() + 255) // 256, 4096)


REPLAY = {"block_tail_fwd": replay_tail_fwd, "block_tail_fwd_fin": replay_tail_fwd,
          "block_tail_bwd_reduce": replay_tail_bwd, "block_tail_bwd_apply": replay_tail_bwd, "block_tail_bwd_apply_fin": replay_tail_bwd,
          "bn_bwd_reduce": replay_bn_bwd, "bn_bwd_apply": replay_bn_bwd, "bn_bwd_apply_fin": replay_bn_bwd,
          "block_tail_bwd_frozen": replay_tail_bwd_frozen, "bn_bwd_frozen": replay_bn_bwd_frozen,
          "maxpool_fwd": replay_maxpool_fwd, "maxpool_bwd": replay_maxpool_bwd, "channel_sum": replay_channel_sum,
          "stem_expand": replay_stem_expand, "logsoftmax_bwd": replay_logsoftmax_bwd,
          "pixelwise_nll_fwd": replay_nll_fwd, "pixelwise_nll_bwd": replay_nll_bwd}


def _main_view(rec):
    a = rec["a"]
    for n in VIEWS[rec["op"]]:
        if a.get(n) is not None:
            return a[n]
    return None


def _shape_str(rec):
    a = rec["a"]
    v = _main_view(rec)
    if v is None:
        return "x".join(map(str, a["predict"][2] if "predict" in a else a["shape"]))
    ps = sorted({a[n].stride[2] for n in VIEWS[rec["op"]] if a.get(n) is not None})
    return "%s %s ps=%s" % ("x".join(map(str, v.shape)), str(v.dtype).replace("torch.", ""), "/".join(map(str, ps)))


def _flags(rec):
    a = rec["a"]
    f = [k for k in ("go2", "ga2", "cb", "relu_mask", "g_sc", "argmax", "xcopy", "g_extra", "xf", "fin_b", "classw") if a.get(k) is not None]
    for k in ("relu", "stride"):
        if a.get(k):
            f.append("%s=%s" % (k, int(a[k])))
    if a.get("xf") is not None:
        f.append("lo=%s" % ("0" if all(v == 0 for v in a["xf"][1]) else "mixed"))
    if rec["op"] == "bn_bwd_frozen" and a.get("red") is None:
        f.append("pure-apply")
    return ",".join(f)


def run_cases(leg, recs):
    rows, fails = [], []
    for r in recs:
        t0 = time.perf_counter()
        try:
            res, wgs = REPLAY[r["op"]](r["a"], r["op"])
        except Exception as e:          # a mismatch, or a launch the replay could not make: a row either way
            res, wgs = "FAIL", 0
            fails.append("%s %s %s [%s]: %s" % (leg, r["op"], _shape_str(r), _flags(r), e))
        rows.append((leg, r["op"], _shape_str(r), _flags(r), wgs, res, time.perf_counter() - t0))
        torch.cuda.empty_cache()
    return rows, fails


def _print_table(rows, capsys, title):
    with capsys.disabled():
        print("\n%s: %d rows" % (title, len(rows)))
        for leg, op, shp, fl, wgs, res, sec in rows:
            print("  %-9s %-25s %-40s %-44s wgs=%-5d %-8s %5.2fs" % (leg, op, shp, fl, wgs, res, sec))


def _sliced(rec):
    return any(v.stride[2] > v.shape[3] for v in _tvs(rec["a"], rec["op"]))


def _assert_frozen_schedule(leg, recs):
    """which kernels a frozen / mixed-mode step must take (ubresnet_amd/engine.py: Engine._bn_bwd, Engine.block_bwd): a fall back to
    the two-pass kernels computes the same gradients and would only show as lost time"""
    used = {r["op"] for r in recs}
    if leg in ("frozen", "frozen-aspp"):
        for op in FROZEN_OPS:
            assert op in used, "the %s step no longer calls ops.%s" % (leg, op)
        two = sorted(used & set(TWO_PASS_OPS))
        assert not two, "the %s step fell back to the two-pass kernels: %s" % (leg, ", ".join(two))
        if leg == "frozen":
            assert any(r["op"] == "block_tail_bwd_frozen" and r["a"]["cb"] is None and r["a"]["g_sc"] is None for r in recs), \
                "no identity tail of the frozen step leaves its skip gradient to conv1's data gradient (g_sc = None)"
        else:
            assert any(r["op"] in FROZEN_OPS and _sliced(r) for r in recs), \
                "the frozen ASPP step no longer passes a channel slice (pixel stride > C) to a one-pass kernel"
    if leg == "mixed":
        assert any(r["op"] == "block_tail_bwd_apply" and r["a"]["relu_mask"] is not None for r in recs), \
            "a tail with sites in different modes no longer takes the masked two-pass fallback (ops.block_tail_bwd_apply)"
        assert "block_tail_bwd_apply_fin" in used, "the all-train tails of the mixed step no longer fuse their finalizes"


@pytest.mark.parametrize("leg", ["headline", "aspp", "infer", "fp32", "frozen", "frozen-aspp", "mixed"])
def test_every_streaming_launch_of_the_leg_matches_the_fp64_reference(leg, monkeypatch, capsys):
    monkeypatch.setattr(plan, "ENABLED", False)
    t0 = time.perf_counter()
    run = _leg(leg)
    cap = Capture(monkeypatch)
    run()
    recs = cap.distinct()
    del run
    torch.cuda.empty_cache()
    if leg == "headline":
        used = {r["op"] for r in recs}
        for op in HEADLINE_OPS:
            assert op in used, "the headline step no longer calls ops.%s" % op
        for op in HEADLINE_SLICED:
            assert any(r["op"] == op and any(v.stride[2] > v.shape[3] for v in _tvs(r["a"], op)) for r in recs), \
                "the headline step no longer passes a channel slice (pixel stride > C) to ops.%s" % op
    _assert_frozen_schedule(leg, recs)
    rows, fails = run_cases(leg, recs)
    _print_table(rows, capsys, "%s (%d launches captured, %.1fs)" % (leg, len(cap.calls), time.perf_counter() - t0))
    assert len(rows) == len(recs)
    assert not fails, "\n".join(fails[:20])
    assert all(res == ("bounded" if op == "logsoftmax_bwd" else "exact") for _, op, _, _, _, res, _ in rows)


# ------------------------------------------------------------------------------------------------------------------
# shapes the legs do not produce, and a dozen they do, as plain cases
# ------------------------------------------------------------------------------------------------------------------
BF, F32 = torch.bfloat16, torch.float32
_base = [1 << 44]


def _v(shape, dt=BF, ps=None, off=0, base=None):
    """a pixel-dense NHWC view of `shape`: channels [off, off + C) of a buffer with pixel stride ps (own storage unless `base`)"""
    N, H, W, C = shape
    ps = ps or C
    if base is None:
        _base[0] += 1 << 36
        base = _base[0]
    return TV.make(shape, (H * W * ps, W * ps, ps, 1), dt, base, base + off * ESZ[dt])


def _case(op, **a):
    for n, p in _SIGS[op].parameters.items():
        a.setdefault(n, None if p.default is inspect.Parameter.empty else p.default)
    return {"op": op, "a": a}


def _tail_fwd(shape, dt=BF, byp=True, ps=None, off=0, fin=True):
    out = _v(shape, dt, ps, off)
    sc = _v(shape, dt) if byp else _v(shape, dt, ps and ps // 2, 0)
    if fin:
        spec = ("fin", 0.1, 1e-5, True)
        return _case("block_tail_fwd_fin", c2=_v(shape, dt), fin2=spec, sc=sc, fin_b=spec if byp else None,
                     count=shape[0] * shape[1] * shape[2], out=out, relu_mask=True)
    return _case("block_tail_fwd", c2=_v(shape, dt), sc=sc, mean_b=True if byp else None, out=out, relu_mask=True)


def _tail_bwd(kind, shape, dt=BF, byp=True, go2_ps=None, go2_off=0, mask=True, g_sc=True):
    a = dict(go=_v(shape, dt), go2=_v(shape, dt, go2_ps, go2_off) if go2_ps else None, c2=_v(shape, dt), cb=_v(shape, dt) if byp else None)
    if kind != "reduce":
        a.update(g_c2=_v(shape, dt), g_sc=_v(shape, dt) if (g_sc or byp) else None)
    if kind == "apply_fin":
        a.update(count=shape[0] * shape[1] * shape[2], dgamma2=True, dbeta2=True, dgamma_b=True if byp else None, dbeta_b=True if byp else None)
    a["relu_mask"] = True if mask else None
    if not mask:
        a["out"] = _v(shape, dt)
    return _case("block_tail_bwd_" + kind, **a)


def _bn_bwd(kind, shape, dt=BF, relu=True, ga_ps=None, ga_off=0, c_ps=None, c_off=0, ga2=False):
    a = dict(ga=_v(shape, dt, ga_ps, ga_off), ga2=_v(shape, dt) if ga2 else None, c=_v(shape, dt, c_ps, c_off), relu=relu)
    if kind != "reduce":
        a["gc"] = _v(shape, dt)
    if kind == "apply_fin":
        a.update(count=shape[0] * shape[1] * shape[2], dgamma=True, dbeta=True)
    return _case("bn_bwd_" + kind, **a)


def _tail_frozen(shape, dt=BF, byp=True, go2_ps=None, go2_off=0, g_sc=True, gc2_ps=None, gc2_off=0):
    return _case("block_tail_bwd_frozen", go=_v(shape, dt), go2=_v(shape, dt, go2_ps, go2_off) if go2_ps else None, relu_mask=True,
                 c2=_v(shape, dt), red2=True, cb=_v(shape, dt) if byp else None, red_b=True if byp else None,
                 g_c2=_v(shape, dt, gc2_ps, gc2_off), g_sc=_v(shape, dt) if (g_sc or byp) else None)


def _bn_frozen(shape, dt=BF, relu=True, ga2=False, red=True, ga_ps=None, ga_off=0, c_ps=None, c_off=0):
    return _case("bn_bwd_frozen", ga=_v(shape, dt, ga_ps, ga_off), ga2=_v(shape, dt) if ga2 else None, c=_v(shape, dt, c_ps, c_off),
                 relu=relu, red=True if red else None, gc=_v(shape, dt))


def _pool(bwd, shape, stride, dt=BF, xf=True, argmax=False, slice_ps=None, slice_off=0, extra=True, xcopy=False):
    N, H, W, C = shape
    oshape = (N, kref.pool_out(H, stride), kref.pool_out(W, stride), C)
    spec = ("affine", (0.0,) * C) if xf else None
    if bwd:
        return _case("maxpool_bwd", x=_v(shape, dt), xf=spec, g_pooled=_v(oshape, dt, slice_ps, slice_off),
                     g_extra=_v(shape, dt) if extra else None, gx=_v(shape, dt), stride=stride, argmax=True if argmax else None)
    return _case("maxpool_fwd", x=_v(shape, dt), xf=spec, pooled=_v(oshape, dt, None if xcopy else slice_ps, slice_off),
                 xcopy=_v(shape, dt, slice_ps, slice_off) if xcopy else None, stride=stride, argmax=True if argmax else None)


PARTIAL = (2, 1000, 721, 16)      # 1 442 000 pixels: with the grid capped, the second trip is partial, and only for some threads
# The one-pass kernels of frozen sites walk trips of four pixels per thread (UNR = 4), pixel u of a trip at p + u * pstep.
# 316 683 pixels x 32 bf16 channels = 1 266 732 units: pick_blocks(npix, 4, 512, 8) wants 619 workgroups and is capped at 512, so
# pstep = 512 * 256 / 4 = 32 768 and a trip covers 131 072 pixels: two full trips, then 54 539 pixels = 32 768 + 21 771 -- in the
# third trip pixel 0 of the unroll is full, pixel 1 is partial (only for the threads below 21 771 * 4), pixels 2 and 3 are empty.
# With 64 channels and no sums (pure apply), pick_blocks(npix, 8, 2048, 4) wants 2475 and is capped at 2048: pstep = 65 536, a trip
# covers 262 144 pixels, and the second trip (54 539 pixels) is partial in its first pixel.
PARTIAL_FROZEN = (3, 333, 317, 32)
PARTIAL_FROZEN_APPLY = (3, 333, 317, 64)
SWITCH = (2, 64, 64, 32)          # 8192 pixels: 16 workgroups with sums (32 in fp32), 32 for pure apply (64 in fp32): whole trips only
# (shape, type) per form of the sums flush (red_flush_mode / flush_sums_pow2 / flush_sums in csrc/ubr_elem.hip); workgroups with
# sums = pick_blocks(npix, CU, 512, 8); no trip is partial at these sizes (the flush is what differs)
FLUSH_FORMS = [("C16", (4, 32, 32, 16), BF),           # CU 2: register butterfly over five lane bits; 4 workgroups
               ("C80", (4, 32, 32, 80), BF),           # CU 10: not a power of two, below a wave: fp64 LDS atomics; 20 workgroups (a multiple of 5)
               ("C96", (4, 32, 32, 96), BF),           # CU 12: the same; 24 workgroups (a multiple of 3)
               ("C512", (16, 16, 16, 512), BF),        # CU 64: one unit per lane, no butterfly; 128 workgroups
               ("C512-f32", (4, 16, 16, 512), F32),    # CU 128: a wave covers half the units: the per-wave rows are zeroed first; 64 workgroups
               ("C768", (4, 16, 16, 768), BF)]         # CU 96: >= 64 and not a power of two, routed to the row flush by rule; 48 workgroups


def _frozen_cases():
    """the one-pass backward of frozen BatchNorm sites (ubr_block_tail_bwd_frozen, ubr_bn_bwd_frozen) at the smallest shapes that
    still take each of its paths, and the two-pass paths that only a frozen or mixed-mode step reaches"""
    c = []
    # every form of the sums flush, through both one-pass kernels
    for nm, shp, dt in FLUSH_FORMS:
        c += [("frozen-tail-" + nm, _tail_frozen(shp, dt)), ("frozen-bn-" + nm, _bn_frozen(shp, dt))]
    # CU = 96 through the two-pass reduce kernels, which share the rule
    c += [("bn-reduce-C768", _bn_bwd("reduce", FLUSH_FORMS[-1][1])), ("tail-reduce-C768", _tail_bwd("reduce", FLUSH_FORMS[-1][1]))]
    # a last trip that is partial for only some of the four unrolled pixels, under the workgroup cap (see PARTIAL_FROZEN)
    c += [("frozen-tail-partial", _tail_frozen(PARTIAL_FROZEN, go2_ps=64, go2_off=32)),
          ("frozen-bn-partial", _bn_frozen(PARTIAL_FROZEN, ga2=True)),
          ("frozen-bn-partial-pure-apply", _bn_frozen(PARTIAL_FROZEN_APPLY, red=False))]
    # the template switches, in all three element types
    for tn, dt in (("f32", F32), ("bf16", BF), ("f16", torch.float16)):
        for byp in (True, False):
            for two in (False, True):
                c.append(("frozen-tail-%s-%s%s" % (tn, "bypass" if byp else "identity", "-go2" if two else ""),
                          _tail_frozen(SWITCH, dt, byp=byp, go2_ps=32 if two else None)))
        c.append(("frozen-tail-%s-identity-lazy" % tn, _tail_frozen(SWITCH, dt, byp=False, g_sc=False)))
        for relu in (True, False):
            for two in (False, True):
                for red in (True, False):
                    c.append(("frozen-bn-%s%s%s%s" % (tn, "-relu" if relu else "", "-ga2" if two else "", "" if red else "-pure-apply"),
                              _bn_frozen(SWITCH, dt, relu=relu, ga2=two, red=red)))
    # channel slices: ga and c as channels 32..48 of 80-channel buffers (the ASPP concat layout); a tail whose g_c2 is channels
    # 32..64 of a 64-channel buffer (a byte written beyond C lands in the sentinel or in the next pixel's other half)
    c += [("frozen-bn-slice80", _bn_frozen((4, 32, 32, 16), ga_ps=80, ga_off=32, c_ps=80, c_off=32)),
          ("frozen-bn-slice80-pure-apply", _bn_frozen((4, 32, 32, 16), ga_ps=80, ga_off=32, c_ps=80, c_off=32, red=False)),
          ("frozen-tail-gc2-slice64", _tail_frozen(SWITCH, gc2_ps=64, gc2_off=32)),
          ("frozen-tail-identity-lazy-gc2-slice64", _tail_frozen(SWITCH, byp=False, g_sc=False, gc2_ps=64, gc2_off=32))]
    # the two-pass fallback of a tail with sites in different modes: the masked apply pass with k1 / k2 from standalone finalizes
    c += [("tail-apply-masked-bypass", _tail_bwd("apply", SWITCH, mask=True)),
          ("tail-apply-masked-identity", _tail_bwd("apply", SWITCH, byp=False, mask=True)),
          ("tail-apply-masked-partial", _tail_bwd("apply", PARTIAL_FROZEN, mask=True))]
    return c


def _extra_cases():
    c = []
    # the general max-pool backward kernel: stride 2 with odd H and W, with and without the saved arg-max, g_extra added
    c += [("pool-odd-fwd", _pool(False, (2, 33, 47, 16), 2, argmax=True)),
          ("pool-odd-bwd-argmax", _pool(True, (2, 33, 47, 16), 2, argmax=True)),
          ("pool-odd-bwd-rescan", _pool(True, (2, 33, 47, 16), 2)),
          # stride 1, ties everywhere, the pooled map / its gradient a 16-channel slice of an 80-channel buffer
          ("pool-s1-fwd-slice80", _pool(False, (2, 32, 52, 16), 1, xf=False, slice_ps=80, slice_off=64)),
          ("pool-s1-bwd-slice80", _pool(True, (2, 32, 52, 16), 1, xf=False, slice_ps=80, slice_off=64))]
    # unit counts that are not powers of two (the atomic flush of the reduce passes), and 64 units (one unit per lane)
    for C in (96, 80, 512):
        shp = (4, 32, 32, C) if C < 512 else (16, 16, 16, 512)
        c += [("bn-reduce-C%d" % C, _bn_bwd("reduce", shp)), ("tail-reduce-C%d" % C, _tail_bwd("reduce", shp)),
              ("channel-sum-C%d" % C, _case("channel_sum", g=_v(shp))), ("tail-fwd-C%d" % C, _tail_fwd(shp, fin=False)),
              ("bn-apply-C%d" % C, _bn_bwd("apply_fin", shp))]
    # a last trip that is partial for only some threads, under the workgroup cap
    c += [("partial-tail-fwd", _tail_fwd(PARTIAL, ps=32, off=16)), ("partial-tail-reduce", _tail_bwd("reduce", PARTIAL, go2_ps=32, go2_off=16)),
          ("partial-tail-apply", _tail_bwd("apply_fin", PARTIAL, go2_ps=32, go2_off=16)), ("partial-tail-apply-out", _tail_bwd("apply", PARTIAL, mask=False)),
          ("partial-bn-reduce", _bn_bwd("reduce", PARTIAL, ga2=True)), ("partial-bn-apply", _bn_bwd("apply", PARTIAL)),
          ("partial-channel-sum", _case("channel_sum", g=_v(PARTIAL, BF, 32, 16)))]
    c += _frozen_cases()
    # captured shapes of the headline / ASPP / fp32 legs
    c += [("tail-fwd-16x256x256x32", _tail_fwd((16, 256, 256, 32), ps=64, off=32)),
          ("tail-fwd-identity-16x256x256x16", _tail_fwd((16, 256, 256, 16), byp=False)),
          ("tail-reduce-16x256x256x32", _tail_bwd("reduce", (16, 256, 256, 32), go2_ps=64, go2_off=32)),
          ("tail-apply-16x256x256x32", _tail_bwd("apply_fin", (16, 256, 256, 32), go2_ps=64, go2_off=32)),
          ("tail-apply-identity-lazy", _tail_bwd("apply_fin", (16, 128, 128, 64), byp=False, g_sc=False)),
          ("tail-apply-f32", _tail_bwd("apply_fin", (2, 256, 256, 32), dt=F32)),
          ("bn-reduce-16x512x512x16", _bn_bwd("reduce", (16, 512, 512, 16))),
          ("bn-apply-16x512x512x16", _bn_bwd("apply_fin", (16, 512, 512, 16))),
          ("bn-aspp-slice80", _bn_bwd("apply_fin", (16, 128, 208, 16), ga_ps=80, ga_off=32, c_ps=80, c_off=32)),
          ("pool-fwd-16x512x512x16", _pool(False, (16, 512, 512, 16), 2, argmax=True, slice_ps=32, slice_off=16, xcopy=True)),
          ("pool-bwd-16x512x512x16", _pool(True, (16, 512, 512, 16), 2, argmax=True)),
          ("channel-sum-16x512x512x16", _case("channel_sum", g=_v((16, 512, 512, 16)))),
          ("stem-expand-16x512x512", _case("stem_expand", out=_v((16, 512, 512, 16)))),
          ("stem-expand-3-planes", _case("stem_expand", out=_v((2, 64, 104, 48), F32))),
          ("logsoftmax-bwd-16x3x512x512", _case("logsoftmax_bwd", logp=("t", "torch.float32", (16, 3, 512, 512)), g_logits=_v((16, 512, 512, 16)))),
          ("nll-fwd-classw-ignore", _case("pixelwise_nll_fwd", predict=("t", "torch.float32", (16, 3, 512, 512)), classw=True, ignore_index=-100, bad=True)),
          ("nll-bwd-classw-ignore", _case("pixelwise_nll_bwd", classw=True, ignore_index=-100, shape=(16, 3, 512, 832)))]
    return c


EXTRA_CASES = _extra_cases() if torch.cuda.is_available() else []


@pytest.mark.parametrize("case", EXTRA_CASES, ids=[c[0] for c in EXTRA_CASES])
def test_streaming_case_matches_the_fp64_reference(case, capsys):
    name, rec = case
    rows, fails = run_cases("case", [rec])
    _print_table(rows, capsys, name)
    assert not fails, "\n".join(fails)
    assert rows[0][5] == ("bounded" if rec["op"] == "logsoftmax_bwd" else "exact")


def test_nll_counts_bad_labels_and_confusion_is_exact():
    rec = _case("pixelwise_nll_fwd", predict=("t", "torch.float32", (3, 4, 97, 131)), classw=True, ignore_index=2, bad=True)
    replay_nll_fwd(rec["a"], rec["op"], n_bad=7)
    N, C, H, W = 5, 4, 301, 517
    lp = -kref.exact_operands((N, C, H, W), torch.float32, density=0.6, seed=91, zero_tiles=0, device=DEV).abs()      # ties are the rule
    tgt = torch.randint(-1, C + 1, (N, H, W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(92))
    cm = Guard(C * C, torch.int64, 3)
    cm.begin()
    ops.confusion(lp, tgt, cm.t)
    torch.cuda.synchronize()
    assert torch.equal(cm.t - 3, kref.confusion_ref(lp, tgt))
    cm.check("confusion")
