"""Every conv / weight-gradient launch the product makes, at its real shape, against the float64 references of
tests/kref.py on exact operands (see kref's docstring): bit for bit where the budget holds, within a stated bound
where it cannot.

The legs (the bench's headline train step, its ASPP leg, the inference leg, the fp32 train step, and three small steps through the
frozen-BatchNorm schedule: every site frozen on the U-ResNet and on ASPP_ResNet, and a train-mode step with two frozen sites) run once with
ops.conv / ops.conv_phases / ops.wgrad wrapped: every call is recorded -- tensor views (shape, strides, how they
share storage), taps, flags, and the kernel variant that ran.  Each distinct call is then replayed on fresh exact
operands, in buffers of the same layout and aliasing whose every element outside the views holds a NaN sentinel:
the replay must launch the same kernel variant, every output must equal the reference, the statistics must be exact
or within kref's bound, and the sentinel must be untouched.  Weight gradients are replayed as one launch and
through ops.ReduceBatch, as the engine defers their slab sums.  A table row is printed per case.

FAST_CASES are a dozen of those shapes as plain parametrized cases, each pinned to the kernel variant it runs (a failure
names its shape without the capture)."""
import ctypes as C
import inspect
import os
import time

import pytest
import torch

import kref
from kref import ESZ, TV, Buffers

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import ops, plan, synthetic
    from ubresnet_amd.ops import Affine

DEV = "cuda"
Q = 0.25               # grid of every product and partial sum: x ints, xform(x) halves, weights / gradients halves
_DT_NAME = {torch.float32: "float", torch.bfloat16: "bf16_t", torch.float16: "f16_t"}


if torch.cuda.is_available():
    # the operators' own parameter lists (ops._timed sets __wrapped__), taken before any test wraps them
    _SIGS = {"conv": inspect.signature(ops.conv), "phases": inspect.signature(ops.conv_phases), "wgrad": inspect.signature(ops.wgrad)}
_VIEWS = {"conv": ("x", "y", "addend"), "phases": ("x", "y0", "y_full", "addend_full"), "wgrad": ("x", "g")}


def wgrad_kernel_name(dt):
    lib = L.lib()
    a, b, c, d, e = (C.c_int(0) for _ in range(5))
    lib.ubr_wgrad_last_config(C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e))
    return "wgrad_kernel<%s, %d, %d, %d, %s, %s, %s>" % (_DT_NAME[dt], a.value, b.value, c.value, "true" if d.value else "false",
                                                         "true" if e.value else "false", "true" if lib.ubr_wgrad_last_pc() else "false")


# ------------------------------------------------------------------------------------------------------------------
# capture
# ------------------------------------------------------------------------------------------------------------------
def _record(op, args, kwargs):
    """-> call record: {op, a: {name: value}} with tensors replaced by descriptors"""
    b = _SIGS[op].bind(*args, **kwargs)
    b.apply_defaults()
    a = dict(b.arguments)
    torch.cuda.synchronize()
    rec = {"op": op}
    for n in _VIEWS[op]:
        if a.get(n) is not None:
            a[n] = TV(a[n])
    if op in ("conv", "phases"):
        a["wp"] = tuple(a["wp"].shape)
        a["taps"] = tuple(tuple(t) for t in a["taps"])
        if op == "phases":
            a["phases"] = tuple((ry, rx, tuple(tuple(t) for t in tp)) for ry, rx, tp in a["phases"])
        if a.get("xf") is not None:
            a["xf"] = ("affine", tuple(a["xf"].lo[:a["x"].shape[3]].float().cpu().tolist()))
        for n in ("bias", "stats", "addend_mask"):
            if a.get(n) is not None:
                a[n] = (n, a[n].numel())
        if op == "conv" and a.get("bnb") is not None:
            a["bnb"] = ("bnb", TV(a["bnb"][0]))
        a.pop("in_hw", None)
    else:
        if a.get("xf") is not None:
            a["xf"] = ("affine", tuple(a["xf"].lo[:a["x"].shape[3]].float().cpu().tolist()))
        a["taps"] = tuple(tuple(t) for t in a["taps"])
        a["dst"] = a["dst"].numel()
        a["defer"] = a["defer"] is not None
        for n in ("ws", "stream"):
            a.pop(n)
    rec["a"] = a
    return rec


def _signature(rec):
    """dedup key: everything but addresses (views keep their offsets inside a storage group and their 256-byte alignment)"""
    a = rec["a"]
    views = [v for v in a.values() if isinstance(v, TV)]
    if a.get("bnb") is not None and isinstance(a["bnb"], tuple) and a["bnb"][0] == "bnb":
        views.append(a["bnb"][1])
    gids = {}
    for v in views:
        gids.setdefault(v.gid, min(w.ptr for w in views if w.gid == v.gid))
    parts = [rec["op"], rec.get("kernel")]
    for k in sorted(a):
        v = a[k]
        if isinstance(v, TV):
            parts.append((k, v.key(gids[v.gid]), list(gids).index(v.gid), v.ptr % 256))
        elif isinstance(v, tuple) and v and v[0] == "bnb":
            parts.append((k, v[1].key(gids[v[1].gid]), list(gids).index(v[1].gid)))
        else:
            parts.append((k, v))
    return repr(parts)


class Capture:
    def __init__(self, monkeypatch):
        self.calls = []
        self.orig = {"conv": ops.conv, "phases": ops.conv_phases, "wgrad": ops.wgrad}
        o = self.orig

        def conv(*args, **kw):
            rec = _record("conv", args, kw)
            o["conv"](*args, **kw)
            rec["kernel"] = ops.last_conv_kernel()
            self.calls.append(rec)

        def phases(*args, **kw):
            rec = _record("phases", args, kw)
            o["phases"](*args, **kw)
            rec["kernel"] = ops.last_conv_kernel()
            self.calls.append(rec)

        def wgrad(*args, **kw):
            rec = _record("wgrad", args, kw)
            o["wgrad"](*args, **kw)
            rec["kernel"] = wgrad_kernel_name(args[0].dtype)
            self.calls.append(rec)

        monkeypatch.setattr(ops, "conv", conv)
        monkeypatch.setattr(ops, "conv_phases", phases)
        monkeypatch.setattr(ops, "wgrad", wgrad)

    def distinct(self):
        seen = {}
        for r in self.calls:
            seen.setdefault(_signature(r), r)
        return list(seen.values())


# ------------------------------------------------------------------------------------------------------------------
# replay
# ------------------------------------------------------------------------------------------------------------------
_seed = [1000]


def _next_seed():
    _seed[0] += 17
    return _seed[0]


def _density(npix):
    return 0.25 if npix <= (1 << 18) else 0.1


def _fill(view, dt, exp, density=None):
    npix = view.shape[0] * view.shape[1] * view.shape[2]
    v = kref.exact_operands(tuple(view.shape), dt, density=density or _density(npix), seed=_next_seed(), exp=exp, device=DEV)
    view.copy_(v)
    return v


def _affine(spec, C):
    lo = torch.tensor(spec[1], dtype=torch.float32)
    assert bool(((lo == 0) | (lo <= -1e30)).all()), "unexpected clamp values %s" % lo.unique()
    sub, scale, shift, lo = kref.exact_affine(C, _next_seed(), device=DEV, relu=lo)
    return (sub, scale, shift, lo), Affine(sub, scale, shift, lo)


def _packed(shape, dt, Cout):
    wp = kref.exact_operands(shape, dt, density=0.5, seed=_next_seed(), exp=-1, device=DEV)
    wp[:, :, Cout:, :] = 0            # rows >= Cout of the packed image are zero (ubr_pack_weights)
    return wp


def replay_conv(rec, orig):
    """-> (result, detail); raises AssertionError on a mismatch"""
    a, op = rec["a"], rec["op"]
    dt = a["x"].dtype
    views = [v for k, v in a.items() if isinstance(v, TV)]
    bnb_tv = a["bnb"][1] if op == "conv" and a.get("bnb") is not None else None
    if bnb_tv is not None:
        views.append(bnb_tv)
    B = Buffers(views)
    x = B.view(a["x"])
    Cin, Cout = x.shape[3], a["Cout"]
    xin = _fill(x, dt, 0)
    wp = _packed(a["wp"], dt, Cout)
    W = kref.unpack_weights(wp, Cin, Cout)
    xf_ref, xf = _affine(a["xf"], Cin) if a.get("xf") is not None else (None, None)
    bias = None
    if a.get("bias") is not None:
        bias = torch.zeros(a["bias"][1], dtype=torch.float32, device=DEV)
        bias[:Cout] = kref.exact_operands((Cout,), torch.float32, density=0.8, seed=_next_seed(), exp=-2, device=DEV)
    if op == "conv":
        yv = a["y"]
        y = B.view(yv)
        ad = None
        if a.get("addend") is not None:
            av = B.view(a["addend"])
            _fill(av, dt, -2)
            ad = av.clone()
        mask = None
        if a.get("addend_mask") is not None:
            mask = torch.randint(0, 256, (a["addend_mask"][1],), dtype=torch.uint8, device=DEV,
                                 generator=torch.Generator(device=DEV).manual_seed(_next_seed()))
        stats = torch.zeros(a["stats"][1], dtype=torch.float64, device=DEV) if a.get("stats") is not None else None
        bnb = bnb_ref = None
        if bnb_tv is not None:
            c = B.view(bnb_tv)
            _fill(c, dt, 0, density=0.6)
            vec = lambda vals, s: torch.tensor(vals, dtype=torch.float32)[torch.randint(0, len(vals), (Cout,), generator=torch.Generator().manual_seed(s))].to(DEV)
            mean, scale, shift, invstd = vec([-1., 0., 1.], _next_seed()), vec([0.5, 1., 2.], _next_seed()), vec([-1., 0., 1.], _next_seed()), vec([0.5, 1., 2.], _next_seed())
            bnb = (c, mean, scale, shift, invstd)
            bnb_ref = (c.clone(), mean, scale, shift, invstd)
        x_in = x.clone()
        snap = B.snapshot()
        B.mark_written(yv)
        orig["conv"](x, wp, y, list(a["taps"]), Cout, S=a["S"], iy0=a["iy0"], ix0=a["ix0"], xf=xf, bias=bias, addend=B.view(a["addend"]) if ad is not None else None,
                     stats=stats, logsoftmax=a["logsoftmax"], tile_hint=a["tile_hint"], act=a["act"], addend_mask=mask, bnb=bnb,
                     stats_slots=a["stats_slots"])
        torch.cuda.synchronize()
        kern = ops.last_conv_kernel()
        N = x.shape[0]
        OH, OW = (y.shape[2], y.shape[3]) if a["logsoftmax"] else (y.shape[1], y.shape[2])
        ref, ab = kref.conv_ref(x_in, W, list(a["taps"]), Cout, OH, OW, S=a["S"], iy0=a["iy0"], ix0=a["ix0"], xf=xf_ref,
                                bias=bias, addend=ad, addend_mask=mask, act=a["act"])
        what = "%s %s" % (op, kern)
        if a["logsoftmax"]:
            kref.assert_exact(ref, ref, torch.float32, ab, Q, what + " (logits)")      # the logits are exact in fp32
            ls, lim = kref.logsoftmax_ref(ref)
            kref.assert_within(y, ls.permute(0, 3, 1, 2), lim.permute(0, 3, 1, 2), what)
            res = "bounded"
        else:
            kref.assert_exact(y, ref, dt, ab, Q, what)
            res = "exact"
        if stats is not None:
            nslots = kref.RED_SLOTS if (bnb is not None or a["stats_slots"] == kref.RED_SLOTS) else kref.STAT_SLOTS
            sv = stats.view(kref.STAT_SLOTS, -1)
            if nslots < kref.STAT_SLOTS:
                assert float(sv[nslots:].abs().max()) == 0.0, "%s: statistics beyond the %d stripes in use" % (what, nslots)
            s = sv.sum(0)
            refs = kref.conv_stats_ref(ref, bnb_ref, dt)
            st = kref.assert_stats(s, refs, kref.stats_chain(N, OH, OW), Q, Q * 0.5 if bnb is not None else None, what)
            res += "/stats " + st
        B.check_sentinel(snap, what)
        return res, kern
    # phased
    yf = B.view(a["y_full"])
    ad = None
    if a.get("addend_full") is not None:
        av = B.view(a["addend_full"])
        _fill(av, dt, -2)
        ad = av.clone()
    x_in = x.clone()
    snap = B.snapshot()
    for ry, rx, _ in a["phases"]:
        B.mark_written(_phase_tv(a["y_full"], ry, rx))
    y0 = yf[:, 0::2, 0::2, :]
    orig["phases"](x, wp, y0, list(a["taps"]), Cout, phases=[(ry, rx, list(tp)) for ry, rx, tp in a["phases"]], y_full=yf,
                   addend_full=None if a.get("addend_full") is None else B.view(a["addend_full"]), xf=xf, bias=bias)
    torch.cuda.synchronize()
    kern = ops.last_conv_kernel()
    OH, OW = yf.shape[1] // 2, yf.shape[2] // 2
    ref, ab = kref.conv_phases_ref(x_in, W, [(ry, rx, list(tp)) for ry, rx, tp in a["phases"]], Cout, OH, OW, xf=xf_ref, bias=bias,
                                   addend_full=ad)
    written = torch.zeros(ref.shape, dtype=torch.bool, device=DEV)
    for ry, rx, _ in a["phases"]:
        written[:, ry::2, rx::2, :] = True
    got = yf.clone()
    if ad is not None:
        ref = torch.where(written, ref, ad.double())       # positions no phase writes keep the addend (in place) ...
    kref.assert_exact(got[written], ref[written], dt, ab[written], Q, "phases %s" % kern)
    B.check_sentinel(snap, "phases %s" % kern)
    return "exact", kern


def _phase_tv(tv, ry, rx):
    t = TV.__new__(TV)
    t.shape = (tv.shape[0], tv.shape[1] // 2, tv.shape[2] // 2, tv.shape[3])
    t.stride = (tv.stride[0], 2 * tv.stride[1], 2 * tv.stride[2], tv.stride[3])
    t.dtype, t.gid = tv.dtype, tv.gid
    t.ptr = tv.ptr + (ry * tv.stride[1] + rx * tv.stride[2]) * ESZ[tv.dtype]
    return t


def _wgrad_operands(a):
    """fresh exact operands of a recorded weight gradient: (buffers, x, g, reference affine, affine, destination size, initial dst)"""
    dt = a["x"].dtype
    B = Buffers([a["x"], a["g"]])
    x, g = B.view(a["x"]), B.view(a["g"])
    _fill(x, dt, 0)
    _fill(g, dt, -1)
    xf_ref, xf = _affine(a["xf"], x.shape[3]) if a.get("xf") is not None else (None, None)
    n = a["dst"] + 64
    init = None
    if a["accumulate"]:
        init = kref.exact_operands((n,), torch.float32, density=0.5, seed=_next_seed(), exp=-2, device=DEV)
    return B, x, g, xf_ref, xf, n, init


def _wgrad_launch(a, orig, x, g, xf, dst, ws, defer=None):
    orig["wgrad"](x, g, list(a["taps"]), dst, a["sm"], a["sk"], a["Cout_valid"], a["Cin_valid"], ws, S=a["S"], iy0=a["iy0"],
                  ix0=a["ix0"], xf=xf, accumulate=a["accumulate"], dst_offset=a["dst_offset"], exclusive=a["exclusive"], defer=defer)


def _wgrad_check(a, x, g, xf_ref, n, init, outs, what):
    """every destination in `outs` (name -> tensor) equals the fp64 weight gradient on the entries the launch owns, and its
    initial contents everywhere else"""
    taps = list(a["taps"])
    dW, ab = kref.wgrad_ref(x, g, taps, S=a["S"], iy0=a["iy0"], ix0=a["ix0"], xf=xf_ref)
    exp, touched = kref.wgrad_scatter(dW, n, taps, a["sm"], a["sk"], a["Cout_valid"], a["Cin_valid"], a["dst_offset"], init=init)
    abs_, _ = kref.wgrad_scatter(ab, n, taps, a["sm"], a["sk"], a["Cout_valid"], a["Cin_valid"], a["dst_offset"],
                                 init=None if init is None else init.abs())
    before = torch.full((n,), float("nan"), device=DEV) if init is None else init
    for nm, dst in outs.items():
        kref.assert_exact(dst[touched], exp[touched], torch.float32, abs_[touched], Q, "%s (%s)" % (what, nm))
        assert torch.equal(dst[~touched].view(torch.int32), before[~touched].view(torch.int32)), \
            "%s (%s): wrote outside the weight-gradient entries it owns" % (what, nm)


def replay_wgrad(rec, orig):
    a = rec["a"]
    dt = a["x"].dtype
    B, x, g, xf_ref, xf, n, init = _wgrad_operands(a)
    snap = B.snapshot()
    outs, kerns, nsplit = {}, [], None
    for deferred in (False, True):
        dst = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV) if init is None else init.clone()
        ws = ops.WgradWorkspace()
        if deferred:
            batch = ops.ReduceBatch(ws)
            _wgrad_launch(a, orig, x, g, xf, dst, ws, defer=batch)
            kerns.append(wgrad_kernel_name(dt))
            if batch.items:
                nsplit = batch.items[0][0].nsplit
            batch.flush()
        else:
            _wgrad_launch(a, orig, x, g, xf, dst, ws)
            kerns.append(wgrad_kernel_name(dt))
        torch.cuda.synchronize()
        outs["ReduceBatch" if deferred else "single launch"] = dst
    what = "wgrad %s" % kerns[0]
    assert kerns[0] == kerns[1]
    _wgrad_check(a, x, g, xf_ref, n, init, outs, what)
    B.check_sentinel(snap, what)
    return "exact", kerns[0], nsplit


def replay_wgrad_batched(recs, orig):
    """every non-accumulating weight gradient of a leg deferred into ONE ops.ReduceBatch, as the engine defers a backward
    stage's slab sums (UBR_REDUCE_BATCH items per wgrad_reduce_batched launch, slabs side by side in one arena), each item
    against its own fp64 reference.  Returns the number of items."""
    ws = ops.WgradWorkspace()
    batch = ops.ReduceBatch(ws)
    pend = []
    for r in recs:
        a = r["a"]
        if r["op"] != "wgrad" or a["accumulate"]:
            continue
        B, x, g, xf_ref, xf, n, init = _wgrad_operands(a)
        dst = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
        _wgrad_launch(a, orig, x, g, xf, dst, ws, defer=batch)
        pend.append((r, B, x, g, xf_ref, n, dst))
    assert len(batch.items) == len(pend)
    batch.flush()
    torch.cuda.synchronize()
    for r, B, x, g, xf_ref, n, dst in pend:
        _wgrad_check(r["a"], x, g, xf_ref, n, None, {"batched with %d others" % (len(pend) - 1): dst},
                     "wgrad %s %s" % (_shape_str(r), r["kernel"]))
    return len(pend)


def replay(rec, orig):
    t0 = time.perf_counter()
    nsplit = None
    if rec["op"] == "wgrad":
        res, kern, nsplit = replay_wgrad(rec, orig)
    else:
        res, kern = replay_conv(rec, orig)
    if rec["kernel"] is not None:
        assert kern == rec["kernel"], "replay launched %s, the product launched %s" % (kern, rec["kernel"])
    return res, kern, nsplit, time.perf_counter() - t0


def _shape_str(rec):
    a = rec["a"]
    if rec["op"] == "wgrad":
        return "x%s g%s taps%d S%d" % ("x".join(map(str, a["x"].shape)), "x".join(map(str, a["g"].shape)), len(a["taps"]), a["S"])
    y = a["y"] if rec["op"] == "conv" else a["y_full"]
    return "x%s y%s taps%d S%d" % ("x".join(map(str, a["x"].shape)), "x".join(map(str, y.shape)), len(a["taps"]),
                                   a.get("S", 1))


def _flags(rec):
    a = rec["a"]
    f = [k for k in ("xf", "bias", "addend", "addend_full", "stats", "addend_mask", "bnb") if a.get(k) is not None]
    for k in ("act", "logsoftmax", "accumulate", "exclusive", "dst_offset", "tile_hint"):
        if a.get(k):
            f.append("%s=%s" % (k, a[k]))
    if rec["op"] == "conv" and a.get("addend") is not None and a["addend"].ptr == a["y"].ptr:
        f.append("in-place")
    return ",".join(f)


def run_cases(leg, recs, orig):
    rows, fails = [], []
    for r in recs:
        try:
            res, kern, nsplit, sec = replay(r, orig)
        except Exception as e:          # a mismatch, or a launch the replay could not make: a row either way
            res, kern, nsplit, sec = "FAIL", r["kernel"], None, 0.0
            fails.append("%s %s %s: %s" % (leg, r["op"], _shape_str(r), e))
        rows.append((leg, r["op"], _shape_str(r), _flags(r), kern, "-" if nsplit is None else str(nsplit), res, sec))
    return rows, fails


def _print_table(rows, capsys, title):
    with capsys.disabled():
        print("\n%s: %d distinct launches" % (title, len(rows)))
        for leg, op, shp, fl, kern, ns, res, sec in rows:
            print("  %-10s %-6s %-44s %-38s %-52s nsplit=%-3s %-22s %5.2fs" % (leg, op, shp, fl, kern, ns, res, sec))


# ------------------------------------------------------------------------------------------------------------------
# the legs
# ------------------------------------------------------------------------------------------------------------------
def _train_pass(model, x, lab, wgt):
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    out = model(x)
    loss = PixelWiseNLLLoss()(out, lab, wgt)
    loss.backward()
    torch.cuda.synchronize()


def _leg(name):
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.models.ASPP_ResNet import ASPP_ResNet
    torch.manual_seed(3)
    if name == "infer":
        from ubresnet_amd import deploy
        m = deploy.load_model(None, DEV, num_classes=4)
        m.eval()
        m.compute_dtype = torch.float16
        x = torch.from_numpy(synthetic.make_batch(30, 512, 832, 5000)[0]).cuda()
        return lambda: _no_grad(m, x)
    if name in FROZEN_LEGS:
        # small steps through the frozen-BatchNorm schedule: every site frozen (model.eval()), or two sites of a train-mode model,
        # each leaving one block tail with sites in different modes (the mixed cases of test_gpu_frozen_bn.py, both at once)
        if name == "frozen-aspp":
            m = ASPP_ResNet(num_classes=3, in_channels=3, inplanes=16, showsizes=False).cuda().eval()
            dt, (B, H, W, planes) = torch.bfloat16, (1, 64, 96, 3)
        else:
            m = UResNet(num_classes=3, input_channels=1, inplanes=16).cuda()
            dt, (B, H, W, planes) = torch.bfloat16, (2, 128, 128, 1)
            if name == "frozen":
                m.eval()
            else:
                m.train()
                m.enc_layer2.res1.bnpass.eval()
                m.dec_layer3.res.res1.bn2.eval()
    elif name == "aspp":
        m = ASPP_ResNet(num_classes=3, in_channels=3, inplanes=16, showsizes=False).cuda().train()
        dt, (B, H, W, planes) = torch.bfloat16, (16, 512, 832, 3)
    else:
        m = UResNet(num_classes=3, input_channels=1, inplanes=16).cuda().train()
        dt, (B, H, W, planes) = (torch.bfloat16, (16, 512, 512, 1)) if name == "headline" else (torch.float32, (2, 512, 512, 1))
    m.compute_dtype = dt
    x, lab, wgt = (torch.from_numpy(t).cuda() for t in synthetic.make_batch(B, H, W, 1000, planes=planes))
    return lambda: _train_pass(m, x, lab, wgt)


def _no_grad(m, x):
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()


FROZEN_LEGS = ("frozen", "frozen-aspp", "mixed")

# the kernel-variant switches are read once per process; with any of them set, other variants run than the ones named here
_SWITCHED = any(os.environ.get(k) for k in ("UBR_WGRAD_PC", "UBR_CONV_PC", "UBR_CONV_THIN"))
HEADLINE_VARIANTS = ("wgrad_kernel<bf16_t, 2, 4, 9, true, false, true>", "conv_pc_kernel", "conv_thin_kernel")


@pytest.mark.parametrize("leg", ["headline", "aspp", "infer", "fp32", "frozen", "frozen-aspp", "mixed"])
def test_every_launch_of_the_leg_matches_the_fp64_reference(leg, monkeypatch, capsys):
    monkeypatch.setattr(plan, "ENABLED", False)
    t0 = time.perf_counter()
    run = _leg(leg)
    cap = Capture(monkeypatch)
    run()
    recs = cap.distinct()
    del run
    torch.cuda.empty_cache()
    kinds = {r["kernel"] for r in cap.calls}
    if leg == "headline" and not _SWITCHED:
        for v in HEADLINE_VARIANTS:
            assert any(k.startswith(v) for k in kinds), "the headline step no longer runs %s" % v
        assert any(r["op"] == "phases" and r["kernel"].startswith("conv_thin_kernel") for r in recs)
        assert any(r["op"] == "wgrad" and r["a"]["exclusive"] for r in recs)
    rows, fails = run_cases(leg, recs, cap.orig)
    try:
        nb = replay_wgrad_batched(recs, cap.orig)
        if nb:
            rows.append((leg, "wgrad", "%d weight gradients in one ReduceBatch" % nb, "", "wgrad_reduce_batched_kernel", "-", "exact",
                         0.0))
    except Exception as e:
        fails.append("%s: weight gradients in one ReduceBatch: %s" % (leg, e))
    _print_table(rows, capsys, "%s (%d launches captured, %.1fs)" % (leg, len(cap.calls), time.perf_counter() - t0))
    assert not fails, "\n".join(fails[:20])


# ------------------------------------------------------------------------------------------------------------------
# fast subset: real shapes of the legs above as plain cases (contiguous NHWC tensors, one storage each)
# ------------------------------------------------------------------------------------------------------------------
class _Fake:
    """stands in for a tensor when building a call record by hand"""
    _next = [1 << 40]

    def __init__(self, shape, dtype, stride=None, base=None, off=0):
        self.shape, self.dtype = tuple(shape), dtype
        st, acc = [], 1
        for n in reversed(shape):
            st.append(acc)
            acc *= n
        self.stride_ = tuple(stride) if stride else tuple(reversed(st))
        if base is None:
            _Fake._next[0] += 1 << 36
            base = _Fake._next[0]
        self.base, self.off = base, off

    def tv(self):
        t = TV.__new__(TV)
        t.shape, t.stride, t.dtype = self.shape, self.stride_, self.dtype
        t.gid = self.base
        t.ptr = self.base + self.off * ESZ[self.dtype]
        return t


def _conv_case(dt, N, H, W, Cin, Cout, k, S=1, dil=1, xf=False, bias=False, stats=False, addend=False, act=0, kernel=None):
    from ubresnet_amd import ops as _ops
    pad = dil * (k // 2)
    OH, OW = (H + 2 * pad - dil * (k - 1) - 1) // S + 1, (W + 2 * pad - dil * (k - 1) - 1) // S + 1
    cpu = kref.CPU[dt]
    a = dict(x=_Fake((N, H, W, Cin), dt).tv(), wp=(k * k, Cin // cpu, (Cout + 15) // 16 * 16, cpu), y=_Fake((N, OH, OW, Cout), dt).tv(),
             taps=tuple(_ops.conv_taps(k, dil, pad)), Cout=Cout, S=S, iy0=0, ix0=0, xf=("affine", (0.0,) * Cin) if xf else None,
             bias=("bias", Cout) if bias else None, addend=_Fake((N, OH, OW, Cout), dt).tv() if addend else None,
             stats=("stats", 2 * Cout * kref.STAT_SLOTS) if stats else None, logsoftmax=False, tile_hint=0, act=act,
             addend_mask=None, bnb=None, stats_slots=0)
    return {"op": "conv", "a": a, "kernel": kernel}


def _phases_case(dt, N, H, W, Cin, Cout, k, kernel=None, addend=False):
    """k=4: ConvTranspose2d(k4, s2, p1) forward; k=3: data gradient of a stride-2 3x3 conv (input grid H x W = its output)"""
    from ubresnet_amd import ops as _ops
    phases = tuple((ry, rx, tuple(_ops.transposed_phase_taps(k, 1, 1, 2, ry, rx))) for ry in range(2) for rx in range(2))
    cpu = kref.CPU[dt]
    yf = _Fake((N, 2 * H, 2 * W, Cout), dt)
    y0 = _Fake((N, H, W, Cout), dt, stride=(yf.stride_[0], 2 * yf.stride_[1], 2 * yf.stride_[2], 1), base=yf.base)
    a = dict(x=_Fake((N, H, W, Cin), dt).tv(), wp=(k * k, Cin // cpu, (Cout + 15) // 16 * 16, cpu), y0=y0.tv(),
             taps=tuple(t for p in phases for t in p[2]), Cout=Cout, phases=phases, y_full=yf.tv(),
             addend_full=_Fake((N, 2 * H, 2 * W, Cout), dt).tv() if addend else None, xf=None, bias=None)
    return {"op": "phases", "a": a, "kernel": kernel}


def _wgrad_case(dt, N, H, W, Cin, Cout, k, S=1, dil=1, xf=False, exclusive=False, kernel=None):
    from ubresnet_amd import ops as _ops
    pad = dil * (k // 2)
    OH, OW = (H + 2 * pad - dil * (k - 1) - 1) // S + 1, (W + 2 * pad - dil * (k - 1) - 1) // S + 1
    a = dict(x=_Fake((N, H, W, Cin), dt).tv(), g=_Fake((N, OH, OW, Cout), dt).tv(), taps=tuple(_ops.conv_taps(k, dil, pad)),
             dst=Cout * Cin * k * k, sm=Cin * k * k, sk=k * k, Cout_valid=Cout, Cin_valid=Cin, S=S, iy0=0, ix0=0,
             xf=("affine", (0.0,) * Cin) if xf else None, accumulate=False, dst_offset=0, exclusive=exclusive, defer=True)
    return {"op": "wgrad", "a": a, "kernel": kernel}


BF, F16, F32 = "bf16", "f16", "f32"
FAST_CASES = [
    # (op, dtype, shape and flags, the kernel variant the planner picks for it -- a planner change that moves a case shows here)
    # the steady state of the wide producer / consumer weight gradient: one workgroup sums every tile of the batch
    ("wgrad", BF, dict(N=16, H=16, W=16, Cin=512, Cout=512, k=3, xf=True),
     "wgrad_kernel<bf16_t, 2, 4, 9, true, false, true>"),
    ("wgrad", BF, dict(N=16, H=32, W=32, Cin=256, Cout=256, k=3),
     "wgrad_kernel<bf16_t, 2, 4, 9, true, false, true>"),
    ("wgrad", BF, dict(N=16, H=64, W=64, Cin=128, Cout=128, k=3, xf=True),
     "wgrad_kernel<bf16_t, 2, 4, 9, true, false, true>"),
    ("wgrad", BF, dict(N=16, H=512, W=512, Cin=16, Cout=16, k=7),
     "wgrad_kernel<bf16_t, 1, 1, 25, false, false, false>"),
    ("wgrad", BF, dict(N=16, H=256, W=256, Cin=32, Cout=64, k=3, S=2),
     "wgrad_kernel<bf16_t, 2, 1, 9, false, false, false>"),
    ("wgrad", BF, dict(N=16, H=32, W=52, Cin=256, Cout=16, k=3, dil=5),
     "wgrad_kernel<bf16_t, 1, 2, 9, false, true, false>"),          # ASPP branch: a halo of 5
    ("wgrad", F32, dict(N=2, H=128, W=128, Cin=64, Cout=64, k=3, xf=True),
     "wgrad_kernel<float, 2, 4, 9, true, false, false>"),
    ("conv", BF, dict(N=16, H=16, W=16, Cin=512, Cout=512, k=3, xf=True, stats=True),
     "conv_pc_kernel<bf16_t, 2, 1, 9>"),
    ("conv", BF, dict(N=16, H=64, W=64, Cin=128, Cout=128, k=3, xf=True, stats=True),
     "conv_igemm_kernel<bf16_t, 4, 4, 2, true>"),
    ("conv", BF, dict(N=16, H=512, W=512, Cin=16, Cout=16, k=3, xf=True, stats=True),
     "conv_thin_kernel<bf16_t, 8, 1, 2, 2, true, false, false, 0>"),
    ("conv", BF, dict(N=16, H=32, W=52, Cin=256, Cout=16, k=3, dil=3, bias=True, stats=True),
     "conv_igemm_kernel<bf16_t, 1, 1, 1, false>"),
    ("conv", F16, dict(N=30, H=64, W=104, Cin=128, Cout=128, k=3, bias=True, addend=True, act=3),
     "conv_igemm_kernel<f16_t, 4, 4, 2, true>"),
    ("phases", BF, dict(N=16, H=256, W=256, Cin=32, Cout=16, k=4),
     "conv_thin_kernel<bf16_t, 4, 1, 2, 4, false, false, false, 0>"),
    ("phases", BF, dict(N=16, H=128, W=128, Cin=64, Cout=32, k=3, addend=True),
     "conv_igemm_kernel<bf16_t, 4, 2, 2, false>"),
]
_DTS = {BF: torch.bfloat16, F16: torch.float16, F32: torch.float32}


def _fast_id(c):
    op, dt, kw, _ = c
    return "%s-%s-%s" % (op, dt, "-".join("%s%s" % (k, v) for k, v in kw.items() if v is not False))


@pytest.mark.parametrize("case", FAST_CASES, ids=[_fast_id(c) for c in FAST_CASES])
def test_real_shape_case_matches_the_fp64_reference(case):
    op, dt, kw, kernel = case
    make = {"conv": _conv_case, "phases": _phases_case, "wgrad": _wgrad_case}[op]
    rec = make(_DTS[dt], kernel=None if _SWITCHED else kernel, **kw)
    orig = {"conv": ops.conv, "phases": ops.conv_phases, "wgrad": ops.wgrad}
    res, kern, nsplit, _ = replay(rec, orig)
    assert res.startswith(("exact", "bounded")), (res, kern, nsplit)

