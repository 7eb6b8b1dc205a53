"""The parameter side of a pass -- the small launches every step or every deployment depends on -- against the float64 references of
tests/kref.py:

  1. weight images   ubr_pack_weights, ubr_pack_weights_batched: raw bits, scaled or not, fp32 / bf16 / f16; every image of the
                     train and inference tables of three networks, and edge extents on both entry points
  2. BatchNorm fold  ubr_bn_fold_batched: scale = the fp32 rounding of the fp64 value, bias within half an fp32 ulp + 2^-50 of its terms
  3. finalizes       ubr_bn_finalize, ubr_bn_eval_affine, ubr_bn_bwd_finalize(_frozen), ubr_cast_f64_to_f32: the fp32 rounding of the
                     fp64 value summed in stripe order (eval_affine, which works in fp32: gamma(3) / gamma(4))
  4. optimizer steps ubr_adam_step, ubr_sgd_step: a running-error bound per output from rounding counts (kref.adam_ref / sgd_ref)
  5. tiles           ubr_crop_tiles, ubr_stitch_tiles: pure data movement, torch.equal

Every output lives between guard margins that must keep their bits; the UBR_EINVAL cases are host-side checks and launch nothing.
A table row is printed per case: operator, signature, elements, and the worst ratio to the bound or "exact"."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import kref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import deploy, ops, plan, synthetic
    from ubresnet_amd.models.ASPP_ResNet import ASPP_ResNet
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

DEV = "cuda"
D = torch.float64
F32, BF, H16 = torch.float32, torch.bfloat16, torch.float16
NS = kref.STAT_SLOTS
EINVAL = -1
PACK_FMT, FOLD_FMT = "<QQqqqQiiiiii", "<QQQQQQQif"        # ubr_pack_item, ubr_bn_fold_item as ubresnet_amd/engine.py writes them
PACK_WGS = 128                                            # workgroups per image of ubr_pack_weights_batched
PACK_LDS = 8192                                           # kPackLdsFloats

_seed = [9000]


def _next_seed():
    _seed[0] += 17
    return _seed[0]


def _gen():
    return torch.Generator().manual_seed(_next_seed())


def _randn(n, dtype=torch.float32, scale=1.0):
    return (torch.randn(n, generator=_gen(), dtype=D) * scale).to(dtype).to(DEV)


class Guard:
    """n elements between two 64-element margins; begin() snapshots, check() asserts that nothing outside `written` changed"""

    def __init__(self, n, dtype, fill=float("nan")):
        self.full = torch.full((n + 128,), fill, dtype=dtype, device=DEV)
        self.t = self.full[64:64 + n]
        self.n = n

    def set(self, v):
        self.t.copy_(v)
        return self

    def begin(self):
        self.before = self.full.clone()
        return self

    def check(self, what, written=True):
        w = torch.zeros(self.n + 128, dtype=torch.bool, device=DEV)
        if written is True:
            w[64:64 + self.n] = True
        elif written is not False and written is not None:
            w[64:64 + self.n] = written.reshape(-1)
        kref.assert_untouched(self.full, self.before, w, what)


def _print_rows(rows, capsys, title):
    with capsys.disabled():
        print("\n%s: %d rows" % (title, len(rows)))
        for op, sig, n, res in rows:
            print("  %-26s %-72s n=%-9d %s" % (op, sig, n, res if isinstance(res, str) else "ratio %.3f" % res))


def _ratio(got, ref, lim, what):
    """worst |got - ref| / lim; asserts <= 1 element for element (kref.assert_within); lim == 0 demands equality"""
    kref.assert_within(got, ref, lim, what)
    err = (got.double() - ref.to(got.device)).abs()
    lim = lim.to(got.device)
    r = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.zeros_like(err))
    return float(r.max()) if r.numel() else 0.0


def _bits_equal(got, exp, what):
    exp = exp.to(got.device)
    assert got.shape == exp.shape and got.dtype == exp.dtype, "%s: %s %s against %s %s" % (what, got.dtype, tuple(got.shape), exp.dtype, tuple(exp.shape))
    if not torch.equal(kref.bits(got), kref.bits(exp)):
        bad = (kref.bits(got) != kref.bits(exp))
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d elements differ in their bits; first at %s: got %r, expected %r"
                             % (what, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(exp[idx])))


def _bits_either(got, a, b, what):
    """element for element the bits of `a` or of `b` (the two evaluations of kref.bn_finalize_ref)"""
    a, b = a.to(got.device), b.to(got.device)
    bad = (kref.bits(got) != kref.bits(a)) & (kref.bits(got) != kref.bits(b))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at %d: got %r, expected %r (or %r with the multiply-adds fused)"
                             % (what, int(bad.sum()), bad.numel(), i, float(got[i]), float(a[i]), float(b[i])))


# ------------------------------------------------------------------------------------------------------------------
# 1. weight images
# ------------------------------------------------------------------------------------------------------------------
def _pack_tiles(dt, Mpad, KU, nt):
    """tiles of one image in the staged (dense-layout) path of pack_batched_kernel, and its K block"""
    KB = max(1, min(PACK_LDS // (16 * kref.CPU[dt] * nt), KU, 16))
    return (Mpad // 16) * ((KU + KB - 1) // KB), KB


def _mode(sm, sk, tstride, nt):
    if tstride == 1 and sk == nt:
        return "A"
    if tstride == 1 and sm == nt:
        return "B"
    return "gather"


def _find(tensors, ptr):
    for t in tensors:
        if t.data_ptr() <= ptr < t.data_ptr() + t.numel() * t.element_size():
            return t
    return None


def _check_table(tbl, n, params, images, vec, dt, net, group, rows, flags):
    """decode a device table of ubr_pack_item and compare every image it names with pack_ref of the live parameter"""
    raw = bytes(tbl.cpu().numpy().tobytes())
    assert len(raw) == n * struct.calcsize(PACK_FMT)
    cpu = kref.CPU[dt]
    by_ptr = {}
    for k, img in images.items():
        by_ptr.setdefault(img.data_ptr(), []).append(img)
    seen = set()
    for src, dst, sm, sk, tstride, osc, M, Mpad, Kv, KU, nt, _ in struct.iter_unpack(PACK_FMT, raw):
        w = _find(params, src)
        assert w is not None, "%s %s: item source %#x is no parameter of the model" % (net, group, src)
        soff = (src - w.data_ptr()) // 4
        img = [i for i in by_ptr.get(dst, []) if tuple(i.shape) == (nt, KU, Mpad, cpu)]
        assert len(img) == 1, "%s %s: item destination is not one image of the plan" % (net, group)
        img = img[0]
        seen.add(dst)
        scale = None
        if osc:
            assert vec is not None and vec.data_ptr() <= osc < vec.data_ptr() + 4 * vec.numel()
            o = (osc - vec.data_ptr()) // 4
            scale = vec[o:o + M]
        ref = kref.pack_ref(w.detach(), M, Mpad, Kv, KU * cpu, sm, sk, [t * tstride for t in range(nt)], dt, oscale=scale, src_offset=soff)
        what = "%s %s %s M%d K%d/%d taps%d mode %s%s" % (net, group, tuple(w.shape), M, Kv, KU * cpu, nt, _mode(sm, sk, tstride, nt), " scaled" if osc else "")
        _bits_equal(img, ref, what)
        mode = _mode(sm, sk, tstride, nt)
        tiles, KB = _pack_tiles(dt, Mpad, KU, nt)
        if mode != "gather" and tiles > PACK_WGS:
            flags.add("multi-trip")
        if mode != "gather" and KU % KB:
            flags.add("short-k-tile")
        if mode == "gather" and tstride == 7 and Kv == 7 and KU * cpu == 16:
            flags.add("stem-gather")
        if group == "bwd" and Kv < 16 and KU * cpu == 16 and nt == 49:
            flags.add("head-k-padded")
        if nt == 16:
            flags.add("4x4-mode-" + mode)
        rows.append(("pack_weights_batched", what, img.numel(), "exact"))
    return seen


def _fold_check(tbl, n, tensors, vec, what, rows):
    raw = bytes(tbl.cpu().numpy().tobytes())
    assert len(raw) == n * struct.calcsize(FOLD_FMT)
    worst = 0.0
    for ga, be, rm, rv, cb, sc, bi, Cn, eps in struct.iter_unpack(FOLD_FMT, raw):
        g, b, m, v = (_find(tensors, p)[:Cn] for p in (ga, be, rm, rv))
        assert all(_find(tensors, p).data_ptr() == p for p in (ga, be, rm, rv))
        bias = _find(tensors, cb) if cb else None
        s_ref, b_ref, lim = kref.bn_fold_ref(g.detach(), b.detach(), m, v, eps, bias.detach() if bias is not None else None)
        so, bo = (sc - vec.data_ptr()) // 4, (bi - vec.data_ptr()) // 4
        _bits_equal(vec[so:so + Cn], s_ref, "%s fold scale C=%d" % (what, Cn))
        worst = max(worst, _ratio(vec[bo:bo + Cn], b_ref, lim, "%s fold bias C=%d" % (what, Cn)))
    rows.append(("bn_fold_batched", "%s %d sites" % (what, n), n, worst))
    return worst


NETS = {"uresnet_ip16": lambda: (UResNet(num_classes=3, input_channels=1, inplanes=16), (1, 1, 64, 64)),
        "uresnet_ip32": lambda: (UResNet(num_classes=3, input_channels=1, inplanes=32), (1, 1, 64, 64)),
        "aspp_ip16": lambda: (ASPP_ResNet(num_classes=3, in_channels=3, inplanes=16, showsizes=False), (1, 3, 64, 96))}


def _randomize_bn(m):
    """running statistics and affine parameters a fold can get wrong: signs, small variances, biases that matter"""
    g = torch.Generator().manual_seed(77)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            n = mod.num_features
            mod.weight.data.copy_(torch.randn(n, generator=g))
            mod.bias.data.copy_(torch.randn(n, generator=g))
            mod.running_mean.copy_(torch.randn(n, generator=g))
            mod.running_var.copy_(torch.rand(n, generator=g) * 2 + 0.05)


def _train_pass(m, x, lab, wgt):
    m.zero_grad(set_to_none=True)
    PixelWiseNLLLoss()(m(x), lab, wgt).backward()
    torch.cuda.synchronize()


def _batch(shape, seed=1000):
    B, Cin, H, W = shape
    return tuple(torch.from_numpy(t).to(DEV) for t in synthetic.make_batch(B, H, W, seed, planes=Cin))


@pytest.mark.parametrize("net", sorted(NETS))
def test_network_weight_images_and_folds_match_the_fp64_reference(net, capsys):
    torch.manual_seed(3)
    m, shape = NETS[net]()
    _randomize_bn(m)
    m = m.to(DEV)
    x, lab, wgt = _batch(shape)
    params = [p for p in m.parameters()]
    tensors = params + [b for b in m.buffers()]
    rows, flags, worst = [], set(), 0.0
    for dt in (BF, F32):
        m.train()
        m.compute_dtype = dt
        _train_pass(m, x, lab, wgt)
        eng = m.__dict__["_ubr_engine"]
        pl = eng._pack_plan(dt, x.device)
        seen = set()
        for group in ("fwd", "bwd"):
            assert pl["counts"][group] > 0
            seen |= _check_table(pl[group], pl["counts"][group], params, pl["images"], None, dt, net, group, rows, flags)
        assert seen == {i.data_ptr() for i in pl["images"].values()}, "an image of the plan is in neither table"
    for dt in (BF, F32, H16):
        m.eval()
        m.compute_dtype = dt
        with torch.no_grad():
            m(x)
        torch.cuda.synchronize()
        pl = m.__dict__["_ubr_engine"]._plans.get(("inf", dt, x.device))
        assert pl is not None, "the eval forward no longer runs the folded inference schedule"
        worst = max(worst, _fold_check(pl["fold"], pl["nfold"], tensors, pl["vec"], "%s %s" % (net, dt), rows))
        seen = _check_table(pl["pack"], pl["npack"], params, pl["images"], pl["vec"], dt, net, "infer", rows, flags)
        assert seen == {i.data_ptr() for i in pl["images"].values()}
        assert any("scaled" in r[1] for r in rows)
    _print_rows(rows, capsys, "%s weight images (flags: %s; worst fold ratio %.3f)" % (net, ", ".join(sorted(flags)), worst))
    need = {"multi-trip", "stem-gather", "head-k-padded", "4x4-mode-A", "4x4-mode-B"}
    assert need <= flags, "the tables of %s no longer contain: %s" % (net, ", ".join(sorted(need - flags)))


SPECIALS = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1023 * 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -0.0,
            -(1 + 2.0 ** -8), -(1 + 2.0 ** -11), -(2.0 ** -25), 65504.0, 2.0 ** -24, 1 + 2.0 ** -9, 1 + 2.0 ** -12]


def _pack_edge_cases():
    c = []
    for M in (1, 3, 17, 40):
        for mode in "AB":
            c.append(("M%d-K20-t9-%s" % (M, mode), dict(M=M, K=20, nt=9, mode=mode)))
    c += [("M17-K3-pad16-A", dict(M=17, K=3, Kpad=16, nt=9, mode="A")), ("M3-K7-pad16-B", dict(M=3, K=7, Kpad=16, nt=49, mode="B")),
          ("stem-gather", dict(M=16, K=7, Kpad=16, nt=7, mode="stem")), ("gather-M3-K5-pad16", dict(M=3, K=5, Kpad=16, nt=4, mode="scatter")),
          ("short-k-tile-A", dict(M=40, K=80, nt=9, mode="A")), ("short-k-tile-B", dict(M=40, K=80, nt=9, mode="B")),
          ("t49-A", dict(M=17, K=24, nt=49, mode="A")), ("t49-B", dict(M=17, K=24, nt=49, mode="B")),
          ("t64-A", dict(M=17, K=24, nt=64, mode="A")), ("t64-B", dict(M=17, K=24, nt=64, mode="B")),
          ("t16-A", dict(M=40, K=72, nt=16, mode="A")), ("t16-B", dict(M=40, K=72, nt=16, mode="B")),
          # 3 x 44 = 132 tiles for 128 workgroups, the last K tile short: the second trip of the tile loop
          ("two-trips-A", dict(M=40, K=None, nt=1, mode="A")), ("two-trips-B", dict(M=40, K=None, nt=1, mode="B"))]
    return c


PACK_EDGES = _pack_edge_cases()


def _run_batched(dt, items, keep):
    tbl = b"".join(struct.pack(PACK_FMT, *i) for i in items)
    dev = torch.frombuffer(bytearray(tbl), dtype=torch.uint8).to(DEV)
    keep.append(dev)
    L.check(L.lib().ubr_pack_weights_batched(L.dtype_id(dt), dev.data_ptr(), len(items), L.stream_ptr()), "pack_weights_batched")


@pytest.mark.parametrize("dt", [F32, BF, H16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", PACK_EDGES, ids=[c[0] for c in PACK_EDGES])
def test_pack_edge_extents_on_both_entry_points(case, dt, capsys):
    name, a = case
    cpu = kref.CPU[dt]
    M, nt, mode = a["M"], a["nt"], a["mode"]
    K = a["K"] if a["K"] is not None else 16 * cpu * 43 + 3 * cpu - 1
    Kpad = a.get("Kpad") or (K + cpu - 1) // cpu * cpu
    Mpad = (M + 15) // 16 * 16
    off = 12
    if mode == "A":
        sm, sk, ts, numel = K * nt, nt, 1, M * K * nt
    elif mode == "B":
        sm, sk, ts, numel = nt, M * nt, 1, M * K * nt
    elif mode == "stem":                     # packed[ky][kx][co] = w[co][ci][ky][kx], plane ci = 1 of 3
        sm, sk, ts, numel, off = 3 * 49, 1, 7, M * 3 * 49, 49
    else:
        sm, sk, ts, numel = K * nt * 2, nt * 2, 2, M * K * nt * 2
    taps = [t * ts for t in range(nt)]
    src = kref.exact_operands((off + numel + 5,), F32, density=0.8, seed=_next_seed(), exp=-3, maxmag=7, device=DEV)
    sp = torch.tensor(SPECIALS, dtype=F32, device=DEV)
    idx = torch.randperm(numel, generator=_gen())[:4 * len(SPECIALS)].to(DEV) + off
    src[idx] = sp.repeat(4)
    src[off:off + len(SPECIALS)] = sp
    assert int((kref.bits(src) == -2 ** 31).sum()) > 0
    generic = torch.randn(M, generator=_gen()).to(DEV)
    scales = {"none": None, "dyadic": torch.tensor([0.5, 1.0, 2.0, -1.0], device=DEV)[torch.randint(0, 4, (M,), generator=_gen()).to(DEV)],
              "generic": generic}
    n = nt * (Kpad // cpu) * Mpad * cpu
    keep, rows = [], []
    # the single entry point (no scale; its tap list in any order)
    order = torch.randperm(nt, generator=_gen()).tolist()
    g = Guard(n, dt).begin()
    tix = (C.c_int32 * nt)(*[taps[i] for i in order])
    L.check(L.lib().ubr_pack_weights(L.dtype_id(dt), src.data_ptr() + 4 * off, g.t.data_ptr(), M, Mpad, K, Kpad, sm, sk, nt, tix, L.stream_ptr()), "pack_weights")
    torch.cuda.synchronize()
    ref = kref.pack_ref(src, M, Mpad, K, Kpad, sm, sk, [taps[i] for i in order], dt, src_offset=off)
    _bits_equal(g.t.view(ref.shape), ref, "pack_weights %s" % name)
    g.check("pack_weights %s" % name)
    rows.append(("pack_weights", "%s M%d K%d/%d taps%d" % (name, M, K, Kpad, nt), n, "exact"))
    # the batched entry point: the three scale forms as three items of one launch
    guards, items = {}, []
    for k, sc in scales.items():
        guards[k] = Guard(n, dt).begin()
        items.append((src.data_ptr() + 4 * off, guards[k].t.data_ptr(), sm, sk, ts, sc.data_ptr() if sc is not None else 0, M, Mpad, K, Kpad // cpu, nt, 0))
    _run_batched(dt, items, keep)
    torch.cuda.synchronize()
    for k, sc in scales.items():
        ref = kref.pack_ref(src, M, Mpad, K, Kpad, sm, sk, taps, dt, oscale=sc, src_offset=off)
        _bits_equal(guards[k].t.view(ref.shape), ref, "pack_weights_batched %s scale %s" % (name, k))
        guards[k].check("pack_weights_batched %s scale %s" % (name, k))
        tiles, KB = _pack_tiles(dt, Mpad, Kpad // cpu, nt)
        rows.append(("pack_weights_batched", "%s scale %s mode %s tiles %d KB %d" % (name, k, _mode(sm, sk, ts, nt), tiles, KB), n, "exact"))
    if name.startswith("two-trips"):
        assert _pack_tiles(dt, Mpad, Kpad // cpu, nt)[0] > PACK_WGS
    if name.startswith("short-k-tile") or name.startswith("two-trips"):
        assert (Kpad // cpu) % _pack_tiles(dt, Mpad, Kpad // cpu, nt)[1]
    if name.startswith("t49") and dt != F32:
        assert _pack_tiles(dt, Mpad, Kpad // cpu, nt)[1] == 1
    _print_rows(rows, capsys, "pack %s %s" % (name, dt))


# ------------------------------------------------------------------------------------------------------------------
# 2. BatchNorm fold
# ------------------------------------------------------------------------------------------------------------------
def test_bn_fold_extents_null_bias_zero_variance_and_cancellation(capsys):
    sites, tbl, keep = [], b"", []
    for Cn in (1, 40, 1024, 1040):
        for with_bias in (False, True):
            gam, bet, mean = _randn(Cn), _randn(Cn), _randn(Cn)
            var = (torch.rand(Cn, generator=_gen()) * 2 + 0.01).to(DEV)
            var[::7] = 0.0                                                 # running_var = 0: scale = gamma / sqrt(eps)
            cb = _randn(Cn) if with_bias else None
            eps = 1e-5
            # a channel where (b - mean) * s and beta cancel to the last fp32 bit of the product
            s64 = gam.double() / torch.sqrt(var.double() + kref.f32(eps))
            t64 = ((cb.double() if with_bias else 0.0) - mean.double()) * s64
            bet[Cn // 2] = -t64[Cn // 2].float()
            sc, bi = Guard(Cn, F32).begin(), Guard(Cn, F32).begin()
            tbl += struct.pack(FOLD_FMT, gam.data_ptr(), bet.data_ptr(), mean.data_ptr(), var.data_ptr(), cb.data_ptr() if with_bias else 0,
                               sc.t.data_ptr(), bi.t.data_ptr(), Cn, eps)
            sites.append((Cn, with_bias, gam, bet, mean, var, cb, eps, sc, bi))
    dev = torch.frombuffer(bytearray(tbl), dtype=torch.uint8).to(DEV)
    L.check(L.lib().ubr_bn_fold_batched(dev.data_ptr(), len(sites), L.stream_ptr()), "bn_fold_batched")
    torch.cuda.synchronize()
    rows = []
    for Cn, with_bias, gam, bet, mean, var, cb, eps, sc, bi in sites:
        what = "bn_fold C=%d conv_bias %s" % (Cn, "set" if with_bias else "NULL")
        s_ref, b_ref, lim = kref.bn_fold_ref(gam, bet, mean, var, eps, cb)
        _bits_equal(sc.t, s_ref, what + " scale")
        r = _ratio(bi.t, b_ref, lim, what + " bias")
        # the cancelling channel is a test of the bound: its fp32 evaluation is outside
        s32 = gam / torch.sqrt(var + eps)
        b32 = ((cb if with_bias else 0.0) - mean) * s32 + bet
        assert bool(((b32.double() - b_ref).abs() > lim).any()) or Cn == 1
        sc.check(what)
        bi.check(what)
        rows.append(("bn_fold_batched", what, Cn, r))
    _print_rows(rows, capsys, "bn_fold")
    assert L.lib().ubr_bn_fold_batched(dev.data_ptr(), 0, L.stream_ptr()) == EINVAL


# ------------------------------------------------------------------------------------------------------------------
# 3. per-channel finalizes
# ------------------------------------------------------------------------------------------------------------------
FIN_OPS = ("bn_finalize", "bn_eval_affine", "bn_bwd_finalize", "bn_bwd_finalize_frozen", "cast_f64_to_f32")


class FinCapture:
    """wraps the five ops, records what a replay needs: extents, modes and which pointers are NULL -- no addresses"""

    def __init__(self, monkeypatch):
        self.sigs = {}
        self.ncalls = 0
        for n in FIN_OPS:
            monkeypatch.setattr(ops, n, self._wrap(n, getattr(ops, n)))

    def _wrap(self, n, orig):
        def f(*a, **kw):
            self.ncalls += 1
            self.sigs.setdefault(getattr(self, "_" + n)(*a, **kw), None)
            return orig(*a, **kw)
        return f

    @staticmethod
    def _bn_finalize(stats, count, gamma, beta, rmean, rvar, nbt, momentum, eps, scale, shift, mean, invstd):
        return ("bn_finalize", gamma.numel(), float(count), None if momentum < 0 else round(float(momentum), 6), rmean is not None, float(eps))

    @staticmethod
    def _bn_eval_affine(gamma, beta, rmean, rvar, eps, scale, shift, mean, invstd):
        return ("bn_eval_affine", gamma.numel(), float(eps))

    @staticmethod
    def _bn_bwd_finalize(red, count, Cn, dgamma, dbeta, accumulate, k1, k2):
        return ("bn_bwd_finalize", Cn, float(count), dgamma is not None, dbeta is not None, bool(accumulate))

    @staticmethod
    def _bn_bwd_finalize_frozen(red, Cn, dgamma, dbeta, k1=None, k2=None, stream=None):
        return ("bn_bwd_finalize_frozen", Cn, dgamma is not None, dbeta is not None, k1 is not None)

    @staticmethod
    def _cast_f64_to_f32(src, dst, n, scale=1.0, accumulate=False, stride=None, slots=NS):
        return ("cast_f64_to_f32", n, n if stride is None else stride, slots, float(scale), bool(accumulate))


def _stripes(slots, n):
    """[slots][n] fp64, every stripe different.  With 8 or more stripes, stripe 2 holds a value of magnitude 2^40 and stripe slots-2 its
    negative: the stripes added in between lose their bits below 2^-12, so a sum in any other order differs well above fp32 rounding"""
    g = _gen()
    v = torch.randn((slots, n), generator=g, dtype=D)
    if slots >= 8:
        v[2] = torch.randn(n, generator=g, dtype=D) * 2.0 ** 40
        v[slots - 2] = -v[2]
    return v.to(DEV)


def run_bn_finalize(Cn, count, momentum, tracked, eps, nbt0=3, clamp=True):
    what = "bn_finalize C=%d count=%g momentum=%s tracked=%s nbt=%d" % (Cn, count, momentum, tracked, nbt0)
    st = _stripes(NS, 2 * Cn)
    # sums of squares that leave a positive variance: s2 = count*(var + m^2) spread over the stripes like s1
    m = st[:, :Cn].sum(0) / count
    var = (torch.rand(Cn, generator=_gen(), dtype=D) * 3 + 0.01).to(DEV)
    st[:, Cn:] = st[:, Cn:].abs()
    st[NS - 2, Cn:] = -st[2, Cn:]
    st[0, Cn:] += count * (var + m * m) - st[:, Cn:].sum(0)
    if clamp:
        # a constant channel with a large mean: s2/count lies a few ulps BELOW m*m, so s2/count - m*m < 0 in fp64 whether or not
        # the multiply is fused into the subtraction, and the clamp makes the variance exactly 0
        st[:, 0] = 0.0
        st[:, Cn] = 0.0
        mc = 1000.1
        st[5, 0] = count * mc
        st[9, Cn] = count * (mc * mc * (1.0 - 2.0 ** -49))
    G = Guard(NS * 2 * Cn, D).set(st.reshape(-1))
    gam, bet = _randn(Cn), _randn(Cn)
    outs = [Guard(Cn, F32) for _ in range(4)]
    rm = Guard(Cn, F32).set(_randn(Cn)) if tracked else None
    rv = Guard(Cn, F32).set(_randn(Cn).abs() + 0.1) if tracked else None
    nbt = Guard(1, torch.int64, 0).set(torch.tensor([nbt0])) if tracked else None
    rm0, rv0 = (rm.t.clone(), rv.t.clone()) if tracked else (None, None)
    guards = [G] + outs + ([rm, rv, nbt] if tracked else [])
    for g in guards:
        g.begin()
    ops.bn_finalize(G.t, count, gam, bet, rm.t if tracked else None, rv.t if tracked else None, nbt.t if tracked else None,
                    -1.0 if momentum is None else momentum, eps, *[o.t for o in outs])
    torch.cuda.synchronize()
    s = kref.stripe_sum(st.reshape(-1), NS, 2 * Cn, 2 * Cn)
    if clamp:
        mm = s[0] / count
        assert float(s[Cn] / count - mm * mm) < 0.0, "the clamp case is not negative in fp64"
    mom = kref.f32(1.0 / (nbt0 + 1)) if momentum is None else kref.f32(momentum)
    # the kernel's statements allow two evaluations (the compiler may contract var = s2/count - m*m and the running-statistics
    # update into multiply-adds); each element must be one of them
    exp, expf = (kref.bn_finalize_ref(s[:Cn], s[Cn:], count, gam, bet, eps, rm0, rv0, mom, fused=f) for f in (False, True))
    for k, nm in enumerate(("scale", "shift", "mean", "invstd")):
        _bits_either(outs[k].t, exp[k], expf[k], "%s %s" % (what, nm))
    if clamp:
        assert outs[3].t[0].item() == float((1.0 / torch.sqrt(torch.tensor(kref.f32(eps), dtype=D))).float())
    if tracked:
        _bits_either(rm.t, exp[4], expf[4], what + " running_mean")
        _bits_either(rv.t, exp[5], expf[5], what + " running_var")
        assert int(nbt.t) == nbt0 + 1, "%s: the batch counter went from %d to %d" % (what, nbt0, int(nbt.t))
    G.check(what, written=False)
    for g in guards[1:]:
        g.check(what)
    return ("bn_finalize", what[12:], Cn, "exact")


def run_bn_eval_affine(Cn, eps):
    what = "bn_eval_affine C=%d" % Cn
    gam, bet, rm = _randn(Cn), _randn(Cn), _randn(Cn)
    rv = (torch.rand(Cn, generator=_gen()) * 4).to(DEV)
    rv[::5] = 0.0
    outs = [Guard(Cn, F32).begin() for _ in range(4)]
    ops.bn_eval_affine(gam, bet, rm, rv, eps, *[o.t for o in outs])
    torch.cuda.synchronize()
    inv, sc = kref.bn_eval_affine_ref(gam, rv, eps)
    r1 = _ratio(outs[3].t, inv, kref.gamma(3) * inv.abs(), what + " invstd")
    r2 = _ratio(outs[0].t, sc, kref.gamma(4) * sc.abs(), what + " scale")
    _bits_equal(outs[1].t, bet, what + " shift")
    _bits_equal(outs[2].t, rm, what + " mean")
    for o in outs:
        o.check(what)
    return ("bn_eval_affine", "C=%d eps=%g (invstd %.3f, scale %.3f)" % (Cn, eps, r1, r2), Cn, max(r1, r2))


def run_bn_bwd_finalize(Cn, count, has_dg, has_db, accumulate, frozen=False, has_k=True):
    op = "bn_bwd_finalize_frozen" if frozen else "bn_bwd_finalize"
    what = "%s C=%d count=%s dgamma=%s dbeta=%s accumulate=%s k=%s" % (op, Cn, count, has_dg, has_db, accumulate, has_k)
    st = _stripes(NS, 2 * Cn)
    G = Guard(NS * 2 * Cn, D).set(st.reshape(-1)).begin()
    # old gradients of the sums' own magnitude, so that the accumulate form's extra rounding shows
    dg = Guard(Cn, F32).set(_randn(Cn, scale=4.0)).begin()
    db = Guard(Cn, F32).set(_randn(Cn, scale=4.0)).begin()
    k1, k2 = Guard(Cn, F32).begin(), Guard(Cn, F32).begin()
    dg0, db0 = dg.t.clone(), db.t.clone()
    if frozen:
        ops.bn_bwd_finalize_frozen(G.t, Cn, dg.t if has_dg else None, db.t if has_db else None, k1.t if has_k else None, k2.t if has_k else None)
    else:
        ops.bn_bwd_finalize(G.t, count, Cn, dg.t if has_dg else None, db.t if has_db else None, accumulate, k1.t, k2.t)
    torch.cuda.synchronize()
    e_dg, e_db, e_k1, e_k2 = kref.bn_bwd_finalize_ref(st, Cn, None if frozen else count, dg0, db0, accumulate)
    for g, e, on, nm in ((dg, e_dg, has_dg, "dgamma"), (db, e_db, has_db, "dbeta"), (k1, e_k1, has_k, "k1"), (k2, e_k2, has_k, "k2")):
        if on:
            _bits_equal(g.t, e, "%s %s" % (what, nm))
        g.check(what, written=on)
    if frozen and has_k:
        assert not bool(kref.bits(k1.t).any()) and not bool(kref.bits(k2.t).any()), what + ": k1 / k2 of a frozen site must be +0"
    G.check(what, written=False)
    return (op, what[len(op) + 1:], Cn, "exact")


def run_cast(n, stride, slots, scale, accumulate):
    what = "cast_f64_to_f32 n=%d stride=%d slots=%d scale=%g accumulate=%s" % (n, stride, slots, scale, accumulate)
    st = _stripes(slots, stride)
    G = Guard(slots * stride, D).set(st.reshape(-1)).begin()
    dst = Guard(n, F32).set(_randn(n, scale=4.0)).begin()
    d0 = dst.t.clone()
    ops.cast_f64_to_f32(G.t, dst.t, n, scale, accumulate, stride=stride, slots=slots)
    torch.cuda.synchronize()
    _bits_equal(dst.t, kref.cast_ref(st, stride, slots, n, scale, d0, accumulate), what)
    dst.check(what)
    G.check(what, written=False)
    return ("cast_f64_to_f32", what[16:], n, "exact")


def replay_fin(sig):
    op = sig[0]
    if op == "bn_finalize":
        _, Cn, count, mom, tracked, eps = sig
        return run_bn_finalize(Cn, count, mom, tracked, eps, clamp=count > 1)
    if op == "bn_eval_affine":
        return run_bn_eval_affine(sig[1], sig[2])
    if op == "bn_bwd_finalize":
        return run_bn_bwd_finalize(*sig[1:])
    if op == "bn_bwd_finalize_frozen":
        _, Cn, has_dg, has_db, has_k = sig
        return run_bn_bwd_finalize(Cn, None, has_dg, has_db, False, frozen=True, has_k=has_k)
    return run_cast(*sig[1:])


def _set_modes(m, mode):
    """train / all BatchNorm frozen / the mixed case one_bnpass_frozen of test_gpu_frozen_bn.py (the first bnpass site frozen: a
    block tail whose two sites are in different modes takes the two-pass fallback with the standalone finalizes)"""
    m.train()
    if mode == "frozen":
        m.eval()
    elif mode == "mixed":
        name, mod = next((n, b) for n, b in m.named_modules() if n.endswith("bnpass"))
        mod.eval()


@pytest.mark.parametrize("net", ["uresnet_ip16", "aspp_ip16"])
def test_every_finalize_signature_of_the_passes_matches_the_fp64_reference(net, monkeypatch, capsys):
    monkeypatch.setattr(plan, "ENABLED", False)
    torch.manual_seed(3)
    m, shape = NETS[net]()
    m = m.to(DEV)
    B, Cin, H, W = shape
    x, lab, wgt = _batch((2, Cin, H, W))
    cap = FinCapture(monkeypatch)
    for mode in ("train", "frozen", "mixed"):
        _set_modes(m, mode)
        _train_pass(m, x, lab, wgt)
    sigs = list(cap.sigs)
    used = {s[0] for s in sigs}
    assert set(FIN_OPS) <= used, "the passes no longer call: %s" % ", ".join(sorted(set(FIN_OPS) - used))
    rows = [replay_fin(s) for s in sigs]
    _print_rows(rows, capsys, "%s finalizes (%d calls, %d signatures)" % (net, cap.ncalls, len(sigs)))
    assert len(rows) == len(sigs)


def _fin_extra():
    c = []
    for Cn in (16, 100, 129, 1024):
        for mom in (0.1, 0.0, 1.0):
            c.append(("finalize-C%d-mom%g" % (Cn, mom), ("bn_finalize", Cn, 4096.0, mom, True, 1e-5)))
        c += [("finalize-C%d-untracked" % Cn, ("bn_finalize", Cn, 4096.0, 0.1, False, 1e-5)),
              ("finalize-C%d-count1" % Cn, ("bn_finalize", Cn, 1.0, 0.1, True, 1e-5)),
              ("eval-affine-C%d" % Cn, ("bn_eval_affine", Cn, 1e-5)),
              ("bwd-finalize-C%d" % Cn, ("bn_bwd_finalize", Cn, 4096.0, True, True, False)),
              ("bwd-finalize-C%d-accumulate" % Cn, ("bn_bwd_finalize", Cn, 4096.0, True, True, True)),
              ("bwd-finalize-C%d-no-dgamma" % Cn, ("bn_bwd_finalize", Cn, 4096.0, False, True, True)),
              ("bwd-finalize-C%d-no-dbeta" % Cn, ("bn_bwd_finalize", Cn, 1.0, True, False, False)),
              ("frozen-finalize-C%d-k" % Cn, ("bn_bwd_finalize_frozen", Cn, True, True, True)),
              ("frozen-finalize-C%d-no-k" % Cn, ("bn_bwd_finalize_frozen", Cn, True, True, False)),
              ("frozen-finalize-C%d-no-dgamma" % Cn, ("bn_bwd_finalize_frozen", Cn, False, True, True)),
              ("frozen-finalize-C%d-no-dbeta" % Cn, ("bn_bwd_finalize_frozen", Cn, True, False, False))]
    for slots in (1, 8, 32):
        c += [("cast-slots%d-head-bias" % slots, ("cast_f64_to_f32", 3, 16, slots, 1.0, False)),
              ("cast-slots%d-n129-accumulate" % slots, ("cast_f64_to_f32", 129, 200, slots, 0.25, True)),
              ("cast-slots%d-n1024" % slots, ("cast_f64_to_f32", 1024, 1024, slots, 1.0, False))]
    return c


FIN_EXTRA = _fin_extra()


@pytest.mark.parametrize("case", FIN_EXTRA, ids=[c[0] for c in FIN_EXTRA])
def test_finalize_case_matches_the_fp64_reference(case, capsys):
    _print_rows([replay_fin(case[1])], capsys, case[0])


@pytest.mark.parametrize("nbt0", [0, 7])
@pytest.mark.parametrize("Cn", [16, 100, 1024])
def test_bn_finalize_cumulative_average_is_one_workgroup_and_advances_the_counter_once(Cn, nbt0, capsys):
    """momentum None: the factor is 1 / (batches tracked, this one included), read by every thread before thread 0 advances it"""
    _print_rows([run_bn_finalize(Cn, 4096.0, None, True, 1e-5, nbt0=nbt0)], capsys, "cumulative C=%d nbt=%d" % (Cn, nbt0))


def test_finalize_argument_checks_launch_nothing():
    lib, st = L.lib(), L.stream_ptr()
    Cn = 1025
    stats = torch.zeros(NS * 2 * Cn, dtype=D, device=DEV)
    v = [Guard(Cn, F32).begin() for _ in range(8)]
    nbt = Guard(1, torch.int64, 0).begin()
    p = [g.t.data_ptr() for g in v]
    a = (stats.data_ptr(), 16.0, p[0], p[1], p[2], p[3], nbt.t.data_ptr())
    assert lib.ubr_bn_finalize(*a, -1.0, 1e-5, 1025, p[4], p[5], p[6], p[7], st) == EINVAL          # cumulative: one workgroup, C <= 1024
    assert lib.ubr_bn_finalize(*a[:6], None, -1.0, 1e-5, 16, p[4], p[5], p[6], p[7], st) == EINVAL  # ... and it needs the counter
    assert lib.ubr_bn_finalize(*a[:4], p[2], None, None, 0.1, 1e-5, 16, p[4], p[5], p[6], p[7], st) == EINVAL   # running stats come together
    assert lib.ubr_bn_finalize(stats.data_ptr(), 0.5, *a[2:], 0.1, 1e-5, 16, p[4], p[5], p[6], p[7], st) == EINVAL
    assert lib.ubr_bn_bwd_finalize_frozen(stats.data_ptr(), 16, p[0], p[1], p[2], None, st) == EINVAL     # k1 and k2: both or neither
    assert lib.ubr_cast_f64_to_f32(stats.data_ptr(), 8, 4, p[0], 16, 1.0, 0, st) == EINVAL              # stride < n
    assert lib.ubr_cast_f64_to_f32(stats.data_ptr(), 16, 0, p[0], 16, 1.0, 0, st) == EINVAL
    torch.cuda.synchronize()
    for g in v + [nbt]:
        g.check("argument checks", written=False)


# ------------------------------------------------------------------------------------------------------------------
# 4. flat optimizer steps
# ------------------------------------------------------------------------------------------------------------------
N_TWO_TRIPS = 4 * (256 * 4096) + 4          # one float4 more than 4096 workgroups of 256 threads cover in one trip


def _opt_buffers(n):
    g = torch.Generator(device=DEV).manual_seed(_next_seed())
    rnd = lambda: torch.randn(n, generator=g, device=DEV)
    mag = lambda: 10.0 ** (torch.rand(n, generator=g, device=DEV) * 11 - 8)            # 1e-8 .. 1e3
    p, grad = rnd(), rnd() * mag()
    m = grad * (0.5 + torch.rand(n, generator=g, device=DEV)) * torch.sign(rnd())
    v = (grad * grad) * (0.25 + torch.rand(n, generator=g, device=DEV))
    z = slice(0, n, 5)                     # every fifth element: zero gradient on zero state
    grad[z], m[z], v[z] = 0.0, 0.0, 0.0
    return [Guard(n, F32).set(t) for t in (p, grad, m, v)]


def _adam(bufs, n, lr, wd, step, gs=1.0, b1=0.9, b2=0.999, eps=1e-8):
    return L.lib().ubr_adam_step(bufs[0].t.data_ptr(), bufs[1].t.data_ptr(), bufs[2].t.data_ptr(), bufs[3].t.data_ptr(), n, lr, b1, b2, eps, wd,
                                 step, gs, L.stream_ptr())


ADAM_CASES = [(1020, s, wd, lr, 1.0) for s in (1, 2, 100000) for wd in (0.0, 1e-4) for lr in (1e-5, 1e-3)] + \
             [(4, 1, 1e-4, 1e-3, 1.0), (4, 100000, 0.0, 1e-5, 1.0), (1020, 2, 1e-4, 1e-3, 0.5), (N_TWO_TRIPS, 2, 1e-4, 1e-3, 1.0),
              (N_TWO_TRIPS, 100000, 0.0, 1e-5, 0.5)]


@pytest.mark.parametrize("n,step,wd,lr,gs", ADAM_CASES, ids=["n%d-step%d-wd%g-lr%g-gs%g" % c for c in ADAM_CASES])
def test_adam_step_is_within_its_running_error_bound(n, step, wd, lr, gs, capsys):
    bufs = _opt_buffers(n)
    p0, g0, m0, v0 = (b.t.clone() for b in bufs)
    for b in bufs:
        b.begin()
    assert _adam(bufs, n, lr, wd, step, gs) == 0
    torch.cuda.synchronize()
    refs, lims = kref.adam_ref(p0, g0, m0, v0, lr, 0.9, 0.999, 1e-8, wd, step, gs)
    what = "adam_step n=%d step=%d wd=%g lr=%g grad_scale=%g" % (n, step, wd, lr, gs)
    ratios = [_ratio(b.t, r, e, "%s %s" % (what, nm)) for b, r, e, nm in zip((bufs[0], bufs[2], bufs[3]), refs, lims, ("param", "exp_avg", "exp_avg_sq"))]
    assert bool(torch.isfinite(bufs[0].t).all())
    z = slice(0, n, 5)
    if wd == 0.0:                          # zero gradient on zero state: nothing moves
        assert torch.equal(bufs[0].t[z], p0[z]) and not bool(bufs[2].t[z].any()) and not bool(bufs[3].t[z].any())
    bufs[1].check(what + " grad", written=False)
    for b in (bufs[0], bufs[2], bufs[3]):
        b.check(what)
    if n >= 1020:                          # the update is no rounding-level event: an untouched vector is far outside the bounds
        assert float(((m0.double() - refs[1]).abs() / lims[1].clamp_min(1e-300)).max()) > 1e3
    if gs != 1.0:                          # scaling inside the kernel == a run on the scaled gradient (0.5 * g is exact)
        b2 = [Guard(n, F32).set(t) for t in (p0, g0 * gs, m0, v0)]
        assert _adam(b2, n, lr, wd, step, 1.0) == 0
        torch.cuda.synchronize()
        for a, b in zip(bufs, b2):
            if a is not bufs[1]:
                _bits_equal(a.t, b.t, what + ": grad_scale against a pre-scaled gradient")
    _print_rows([("adam_step", what[10:] + " (param %.3f, exp_avg %.3f, exp_avg_sq %.3f)" % tuple(ratios), n, max(ratios))], capsys, "adam")


SGD_CASES = [(1020, mom, damp, nest, first, 1.0) for mom in (0.0, 0.9) for damp in (0.0, 0.5) for nest in (0, 1) for first in (0, 1)] + \
            [(4, 0.9, 0.0, 1, 0, 1.0), (4, 0.0, 0.0, 0, 1, 1.0), (1020, 0.9, 0.5, 1, 0, 0.5), (1020, 0.0, 0.0, 0, 0, 0.5),
             (N_TWO_TRIPS, 0.9, 0.0, 1, 0, 1.0), (N_TWO_TRIPS, 0.9, 0.5, 0, 1, 0.5)]


def _sgd(bufs, n, lr, mom, damp, wd, nest, first, gs):
    return L.lib().ubr_sgd_step(bufs[0].t.data_ptr(), bufs[1].t.data_ptr(), bufs[2].t.data_ptr() if mom != 0 else None, n, lr, mom, damp, wd,
                                nest, first, gs, L.stream_ptr())


@pytest.mark.parametrize("n,mom,damp,nest,first,gs", SGD_CASES, ids=["n%d-mom%g-damp%g-nest%d-first%d-gs%g" % c for c in SGD_CASES])
def test_sgd_step_is_within_its_running_error_bound(n, mom, damp, nest, first, gs, capsys):
    lr, wd = 1e-2, 1e-4
    bufs = _opt_buffers(n)[:3]
    if first:
        bufs[2].t.fill_(float("nan"))       # the first step must not read the buffer
    p0, g0, b0 = (b.t.clone() for b in bufs)
    for b in bufs:
        b.begin()
    assert _sgd(bufs, n, lr, mom, damp, wd, nest, first, gs) == 0
    torch.cuda.synchronize()
    (p_ref, b_ref), (Ep, Eb) = kref.sgd_ref(p0, g0, b0 if mom != 0 else None, lr, mom, damp, wd, bool(nest), bool(first), gs)
    what = "sgd_step n=%d momentum=%g dampening=%g nesterov=%d first_step=%d grad_scale=%g" % (n, mom, damp, nest, first, gs)
    assert bool(torch.isfinite(bufs[0].t).all()), what + ": parameters are not finite"
    ratios = [_ratio(bufs[0].t, p_ref, Ep, what + " param")]
    if mom != 0:
        assert bool(torch.isfinite(bufs[2].t).all()), what + ": the momentum buffer is not finite"
        ratios.append(_ratio(bufs[2].t, b_ref, Eb, what + " momentum buffer"))
    bufs[0].check(what)
    bufs[1].check(what + " grad", written=False)
    bufs[2].check(what + " momentum buffer", written=mom != 0)
    if n >= 1020:                          # the update is no rounding-level event: an untouched vector is far outside the bound
        assert float(((p0.double() - p_ref).abs() / Ep.clamp_min(1e-300)).max()) > 1e3
    if gs != 1.0:
        b2 = [Guard(n, F32).set(t) for t in (p0, g0 * gs, b0)]
        assert _sgd(b2, n, lr, mom, damp, wd, nest, first, 1.0) == 0
        torch.cuda.synchronize()
        _bits_equal(bufs[0].t, b2[0].t, what + ": grad_scale against a pre-scaled gradient")
        if mom != 0:
            _bits_equal(bufs[2].t, b2[2].t, what + ": grad_scale against a pre-scaled gradient (buffer)")
    _print_rows([("sgd_step", what[9:] + " (" + ", ".join("%.3f" % r for r in ratios) + ")", n, max(ratios))], capsys, "sgd")


def test_optimizer_argument_checks_launch_nothing():
    n = 64
    bufs = _opt_buffers(n)
    for b in bufs:
        b.begin()
    lib, st = L.lib(), L.stream_ptr()
    p = [b.t.data_ptr() for b in bufs]
    hyp = (1e-3, 0.9, 0.999, 1e-8, 1e-4)
    assert lib.ubr_adam_step(p[0], p[1], p[2], p[3], 62, *hyp, 1, 1.0, st) == EINVAL                # n % 4
    assert lib.ubr_adam_step(p[0], p[1], p[2], p[3], n, *hyp, 0, 1.0, st) == EINVAL                 # step = 0
    for i in range(4):                                                                             # a pointer off by 4 bytes
        q = list(p)
        q[i] += 4
        assert lib.ubr_adam_step(q[0], q[1], q[2], q[3], 60, *hyp, 1, 1.0, st) == EINVAL
    assert lib.ubr_adam_step(p[0], None, p[2], p[3], n, *hyp, 1, 1.0, st) == EINVAL
    sg = (1e-2, 0.9, 0.0, 1e-4, 0, 0, 1.0)
    assert lib.ubr_sgd_step(p[0], p[1], p[2], 62, *sg, st) == EINVAL
    assert lib.ubr_sgd_step(p[0], p[1], None, n, *sg, st) == EINVAL                                 # momentum with a NULL buffer
    assert lib.ubr_sgd_step(p[0], p[1], p[2], n, 1e-2, 0.0, 0.0, 1e-4, 0, 0, 1.0, st) == EINVAL     # a buffer with zero momentum
    for i in range(3):
        q = list(p[:3])
        q[i] += 4
        assert lib.ubr_sgd_step(q[0], q[1], q[2], 60, *sg, st) == EINVAL
    torch.cuda.synchronize()
    for b in bufs:
        b.check("argument checks", written=False)


# ------------------------------------------------------------------------------------------------------------------
# 5. tile crop and stitch
# ------------------------------------------------------------------------------------------------------------------
def _desc(tiles):
    flat = [int(v) for t in tiles for v in t]
    return (C.c_int32 * len(flat))(*flat)


def _crop(view, tiles, th, tw, what):
    P, rows, cols = view.shape
    out = Guard(len(tiles) * th * tw, F32).begin()
    L.check(L.lib().ubr_crop_tiles(view.data_ptr(), P, rows, cols, _desc(tiles), len(tiles), th, tw, out.t.data_ptr(), L.stream_ptr()), "crop_tiles")
    torch.cuda.synchronize()
    ref = torch.from_numpy(kref.crop_tiles_ref(view.cpu().numpy(), tiles, th, tw))
    _bits_equal(out.t.view(ref.shape), ref, what + " crop")
    out.check(what + " crop")
    return out.t.view(ref.shape)


def _stitch(scores, tiles, P, Cn, rows, cols, what):
    n, _, th, tw = scores.shape
    out = Guard(P * Cn * rows * cols, F32).begin()
    L.check(L.lib().ubr_stitch_tiles(scores.data_ptr(), Cn, th, tw, _desc(tiles), n, out.t.data_ptr(), P, rows, cols, L.stream_ptr()), "stitch_tiles")
    torch.cuda.synchronize()
    ref = kref.stitch_tiles_ref(scores.cpu().numpy(), tiles, np.full((P, Cn, rows, cols), np.nan, dtype=np.float32))
    _bits_equal(out.t.view(P, Cn, rows, cols), torch.from_numpy(ref), what + " stitch")      # NaN where no keep window reaches
    out.check(what + " stitch")
    return ref


def _scores(n, Cn, th, tw):
    return torch.randn((n, Cn, th, tw), generator=torch.Generator(device=DEV).manual_seed(_next_seed()), device=DEV)


def _view(P, rows, cols):
    return torch.randn((P, rows, cols), generator=torch.Generator(device=DEV).manual_seed(_next_seed()), device=DEV) + 3.0


def _tile_cases():
    c = {}
    # the tile overhangs the view at the bottom and at the right
    c["overhang-40x70"] = dict(P=1, rows=40, cols=70, th=64, tw=96, tiles=[(0, 0, 0, 0, 64, 0, 96)], covered=True)
    c["overhang-partial"] = dict(P=2, rows=40, cols=70, th=64, tw=96, tiles=[(1, 8, 16, 0, 64, 0, 96), (0, 0, 0, 0, 8, 0, 96), (0, 8, 0, 0, 64, 0, 96),
                                                                             (1, 0, 0, 0, 8, 0, 96), (1, 8, 0, 0, 64, 0, 16)], covered=True)
    t = deploy.view_tiles(100, 200, 3, 64, 96, False)
    perm = torch.randperm(len(t), generator=torch.Generator().manual_seed(4)).tolist()
    c["shuffled-planes-100x200"] = dict(P=3, rows=100, cols=200, th=64, tw=96, tiles=[t[i] for i in perm], covered=True)
    c["stacked-100x200"] = dict(P=3, rows=100, cols=200, th=64, tw=96, tiles=deploy.view_tiles(100, 200, 3, 64, 96, True), stacked=3, covered=True)
    t = deploy.view_tiles(64, 128, 1, 8, 16, False)
    assert len(t) == 64
    c["64-descriptors"] = dict(P=1, rows=64, cols=128, th=8, tw=16, tiles=t, covered=True)
    t = deploy.view_tiles(100, 200, 1, 64, 96, False)
    c["empty-keep-window"] = dict(P=1, rows=100, cols=200, th=64, tw=96, tiles=t + [(0, 10, 20, 5, 5, 7, 30), (0, 3, 4, 0, 64, 9, 9)], covered=True)
    # a strip (rows 40..43, and the columns right of 150) outside every keep window
    c["uncovered-strip"] = dict(P=1, rows=100, cols=200, th=64, tw=96, covered=False,
                                tiles=[(0, 0, 0, 0, 40, 0, 96), (0, 0, 90, 0, 40, 6, 60), (0, 36, 0, 8, 64, 0, 96), (0, 36, 96, 8, 64, 0, 54)])
    return c


TILE_CASES = _tile_cases() if torch.cuda.is_available() else {}


@pytest.mark.parametrize("Cn", [1, 4])
@pytest.mark.parametrize("name", sorted(TILE_CASES))
def test_crop_and_stitch_move_exactly_the_pixels_of_the_descriptors(name, Cn, capsys):
    a = TILE_CASES[name]
    P, rows, cols, th, tw, tiles = a["P"], a["rows"], a["cols"], a["th"], a["tw"], a["tiles"]
    view = _view(P, rows, cols)
    ctiles = deploy.stacked_crop_desc(tiles, a["stacked"]) if a.get("stacked") else tiles
    crop = _crop(view, ctiles, th, tw, name)
    if rows < th:
        assert not bool(crop[0, rows:].any()) and not bool(crop[0, :, cols:].any()), "the overhang of the crop is not zero"
    oP = 1 if a.get("stacked") else P
    scores = _scores(len(tiles), Cn, th, tw)
    ref = _stitch(scores, tiles, oP, Cn, rows, cols, name)
    holes = int(np.isnan(ref).sum())
    assert (holes == 0) == a["covered"], "%s: %d output pixels outside every keep window" % (name, holes)
    if Cn == 1 and not a.get("stacked") and a["covered"] and name != "empty-keep-window":
        # crop then stitch of a tiling that partitions the view gives the view back
        back = _stitch(crop.unsqueeze(1).contiguous(), tiles, P, 1, rows, cols, name + " round trip")
        assert np.array_equal(back[:, 0], view.cpu().numpy())
    _print_rows([("crop_tiles", "%s %dx%d tile %dx%d P=%d" % (name, rows, cols, th, tw, P), len(ctiles) * th * tw, "exact"),
                 ("stitch_tiles", "%s C=%d %d descriptors, %d pixels left alone" % (name, Cn, len(tiles), holes), oP * Cn * rows * cols, "exact")],
                capsys, "tiles " + name)


def test_tile_argument_checks_launch_nothing():
    lib, st = L.lib(), L.stream_ptr()
    rows, cols, th, tw = 64, 128, 8, 16
    view = _view(1, rows, cols)
    out = Guard(65 * th * tw, F32).begin()
    sc = _scores(65, 1, th, tw)
    so = Guard(rows * cols, F32).begin()
    t65 = deploy.view_tiles(rows, cols, 1, th, tw, False) + [(0, 0, 0, 0, 0, 0, 0)]
    crop = lambda tiles, n=None: lib.ubr_crop_tiles(view.data_ptr(), 1, rows, cols, _desc(tiles), len(tiles) if n is None else n, th, tw, out.t.data_ptr(), st)
    stitch = lambda tiles: lib.ubr_stitch_tiles(sc.data_ptr(), 1, th, tw, _desc(tiles), len(tiles), so.t.data_ptr(), 1, rows, cols, st)
    assert crop(t65) == EINVAL and stitch(t65) == EINVAL                              # 65 descriptors
    assert crop(t65, 0) == EINVAL
    assert crop([(0, rows, 0, 0, 0, 0, 0)]) == EINVAL and stitch([(0, rows, 0, 0, 8, 0, 16)]) == EINVAL      # an origin at `rows`
    assert crop([(0, 0, cols, 0, 0, 0, 0)]) == EINVAL and crop([(1, 0, 0, 0, 0, 0, 0)]) == EINVAL and crop([(0, -1, 0, 0, 0, 0, 0)]) == EINVAL
    assert stitch([(0, 0, 0, 0, th + 1, 0, tw)]) == EINVAL and stitch([(0, 0, 0, 0, th, 0, tw + 1)]) == EINVAL   # keep window beyond the tile
    assert stitch([(0, 0, 0, 5, 4, 0, tw)]) == EINVAL and stitch([(0, 0, 0, -1, 4, 0, tw)]) == EINVAL
    torch.cuda.synchronize()
    out.check("argument checks", written=False)
    so.check("argument checks", written=False)
