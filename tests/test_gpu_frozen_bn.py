"""Fine-tuning with frozen BatchNorm (GPU): a BatchNorm2d in eval mode normalises with its running statistics, leaves them
alone, and back-propagates g_c = scale*g_y, dgamma = sum g_y*xhat, dbeta = sum g_y -- per module, as nn.BatchNorm2d does.

Expected values: torch.autograd through the CPU oracle (oracle/uresnet_oracle.py) with eval-mode BatchNorm, in fp64 and fp32,
on running statistics that normalise (tests/golden/uresnet_ip16_frozen_2x1x64x64.npz: calibrated by the reference model's own
train-mode passes; tests/golden/aspp_ip16_norm_1x3x64x96.npz for ASPP_ResNet), and the reference's own eval-mode
forward + backward recorded in the first fixture.  Bounds are those of the train-mode tests (test_gpu_uresnet.py,
test_gpu_aspp.py, test_gpu_ops.py), named at each use.
"""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import uresnet_oracle as O
from ubresnet_amd import synthetic

if torch.cuda.is_available():
    from ubresnet_amd import ops
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.models.ASPP_ResNet import ASPP_ResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    from test_gpu_uresnet import _grad_row, _grad_verdict, _rel

torch.set_num_threads(min(16, os.cpu_count() or 1))
DEV = "cuda"
STAT_KEYS = ("running_mean", "running_var", "num_batches_tracked")


def _frozen_sd(golden_dir):
    """seeded weights of the train fixture with the frozen fixture's (normalising) running statistics"""
    g = np.load(os.path.join(golden_dir, "uresnet_ip16_frozen_2x1x64x64.npz"))
    sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), int(g["meta"][5]))
    return g, O.state_dict_with_bn_stats(sd, g["bn_keys"], g["bn_stats"])


def _model(sd):
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(sd)
    return m.to(DEV)


def _f64(sd):
    return OrderedDict((k, v.double() if v.is_floating_point() else v) for k, v in sd.items())


def _oracle(fwd, sd, x, lab, wgt):
    """(loss, grads, logp, new running statistics) of pixelwise_nll(fwd(params, x, new_stats)) on the CPU"""
    p = OrderedDict((k, v.clone().requires_grad_(True) if O.is_param_key(k) else v) for k, v in sd.items())
    ns = {}
    logp = fwd(p, x, ns)
    loss = O.pixelwise_nll(logp, lab, wgt)
    names = [k for k in p if O.is_param_key(k)]
    return loss.detach(), OrderedDict(zip(names, torch.autograd.grad(loss, [p[k] for k in names]))), logp.detach(), ns


def _eval_fwd(forward):
    return lambda p, x, ns: forward(p, x, False, None)


def _step(m, xt, lt, wt):
    m.zero_grad(set_to_none=True)
    out = m(xt.to(DEV))
    loss = PixelWiseNLLLoss()(out, lt.to(DEV), wt.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), loss.item(), OrderedDict((n, p.grad.detach().clone()) for n, p in m.named_parameters())


def _stats(m):
    return OrderedDict((k, v.detach().clone()) for k, v in m.state_dict().items() if k.endswith(STAT_KEYS))


def _judge(grads, g32, g64, cos_min=0.9999, l2_max=2e-2):
    rows, fails = [], []
    for n in g64:
        rows.append(_grad_row(n, grads[n].cpu().double(), g32[n].double(), g64[n]))
        fails += _grad_verdict(rows[-1], cos_min=cos_min, l2_max=l2_max)
    print("worst grad (max-abs rel, l2 rel, min cos):", max(r[1] for r in rows), max(r[3] for r in rows), min(r[5] for r in rows))
    return fails


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("tag", ["2x1x64x64", "1x1x96x128"])
def test_uresnet_all_frozen_fp32(golden_dir, tag):
    """model.eval() + backward(): log-probabilities per element within 1e-3|ref| + 1e-4 of the fp32 oracle, loss within 1e-4,
    every gradient by the rule of test_gpu_uresnet._grad_verdict against the fp64 oracle -- conv1.bias / conv10.bias included:
    in front of a frozen BatchNorm they are real gradients (norm above 1e-3 of their weight's).  Buffers bitwise unchanged."""
    g, sd = _frozen_sd(golden_dir)
    B, H, W = [int(v) for v in tag.replace("x1x", "x", 1).split("x")]
    x, lab, wgt = synthetic.make_batch(B, H, W, int(g["meta"][4]))
    xt, lt, wt = torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(wgt)
    l32, g32, p32, _ = _oracle(_eval_fwd(O.uresnet_forward), sd, xt, lt, wt)
    l64, g64, _, _ = _oracle(_eval_fwd(O.uresnet_forward), _f64(sd), xt.double(), lt, wt.double())
    for b in ("conv1", "conv10"):        # the oracle itself: these biases are not noise in front of a frozen BatchNorm
        assert float(g64[b + ".bias"].norm()) > 1e-3 * float(g64[b + ".weight"].norm()), b
    m = _model(sd)
    m.eval()
    before = _stats(m)
    out, loss, grads = _step(m, xt, lt, wt)
    d = (out.cpu() - p32).abs()
    print("frozen", tag, "logp worst excess %.3e" % float((d - 1e-3 * p32.abs()).max()), "loss", loss, "oracle", float(l32))
    assert bool((d <= 1e-3 * p32.abs() + 1e-4).all()), "log-probabilities: worst per-element excess %.3e" % float((d - 1e-3 * p32.abs()).max())
    assert abs(loss - float(l32)) <= 1e-4 * abs(float(l32))
    fails = _judge(grads, g32, g64)
    assert not fails, "; ".join(fails[:8])
    for b in ("conv1", "conv10"):
        assert float(grads[b + ".bias"].double().norm()) > 1e-3 * float(grads[b + ".weight"].double().norm()), b
    for k, v in _stats(m).items():
        assert torch.equal(v, before[k]), "%s changed in a frozen step" % k
    if tag == "2x1x64x64":               # the reference's own eval-mode step (5e-2 on each norm, as the train test)
        assert bool(((out.cpu() - torch.from_numpy(g["logp_eval"])).abs() <= 1e-3 * p32.abs() + 1e-4).all())
        assert abs(loss - float(g["loss"])) <= 1e-4 * abs(float(g["loss"]))
        for n, ref_norm in zip([str(v) for v in g["grad_names"]], g["grad_norms"]):
            norm = float(grads[n].double().norm())
            assert abs(norm - ref_norm) <= 5e-2 * ref_norm + 1e-6, "grad norm %s: %g vs reference %g" % (n, norm, ref_norm)


# ------------------------------------------------------------------------------------------ 2
def test_per_module_eval_equals_model_eval(golden_dir):
    """model.train() with every BatchNorm2d in eval mode is the same computation as model.eval(): bitwise"""
    g, sd = _frozen_sd(golden_dir)
    x, lab, wgt = synthetic.make_batch(2, 64, 64, 1000)
    xt, lt, wt = torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(wgt)
    ma, mb = _model(sd), _model(sd)
    ma.eval()
    mb.train()
    for bn in mb.modules():
        if isinstance(bn, nn.BatchNorm2d):
            bn.eval()
    before = _stats(mb)
    oa, la, ga = _step(ma, xt, lt, wt)
    ob, lb, gb = _step(mb, xt, lt, wt)
    assert torch.equal(oa, ob), "log-probabilities differ"
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    for k, v in _stats(mb).items():
        assert torch.equal(v, before[k]), "%s overwritten although its module is in eval mode" % k


# ------------------------------------------------------------------------------------------ 3
def _bn(sd, pre, x, train_of, ns):
    return O._bn(sd, pre, x, train_of(pre), ns if train_of(pre) else None)


def _block(sd, pre, x, stride, train_of, ns):
    out = F.relu(_bn(sd, pre + ".bn1", O._conv(sd, pre + ".conv1", x, stride, 1), train_of, ns))
    out = F.relu(_bn(sd, pre + ".bn2", O._conv(sd, pre + ".conv2", out, 1, 1), train_of, ns))
    sc = _bn(sd, pre + ".bnpass", O._conv(sd, pre + ".bypass", x, stride, 0), train_of, ns) if (pre + ".bypass.weight") in sd else x
    return F.relu(out + sc)


def _double(sd, pre, x, stride, train_of, ns):
    return _block(sd, pre + ".res2", _block(sd, pre + ".res1", x, stride, train_of, ns), 1, train_of, ns)


def _dec(sd, pre, x, skip, train_of, ns):
    up = F.conv_transpose2d(x, sd[pre + ".deconv.weight"], None, 2, 1)
    return _double(sd, pre + ".res", torch.cat([up, skip], 1), 1, train_of, ns)


def _uresnet_mixed(train_of):
    """the oracle's UResNet (oracle.uresnet_forward) with a train / frozen flag per BatchNorm site"""
    def fwd(sd, x, ns):
        x0 = F.relu(_bn(sd, "bn1", O._conv(sd, "conv1", x, 1, 3), train_of, ns))
        e = [F.max_pool2d(x0, 3, 2, 1)]
        for i, s in enumerate((1, 2, 2, 2, 2)):
            e.append(_double(sd, "enc_layer%d" % (i + 1), e[-1], s, train_of, ns))
        y = e[5]
        for lvl, skip in ((5, e[4]), (4, e[3]), (3, e[2]), (2, e[1]), (1, x0)):
            y = _dec(sd, "dec_layer%d" % lvl, y, skip, train_of, ns)
        y = F.relu(_bn(sd, "bn10", O._conv(sd, "conv10", y, 1, 3), train_of, ns))
        return F.log_softmax(O._conv(sd, "conv11", y, 1, 3), dim=1)
    return fwd


MIXED = {
    "encoder_frozen": lambda pre: not (pre == "bn1" or pre.startswith("enc_layer")),
    "one_bnpass_frozen": lambda pre: pre != "enc_layer2.res1.bnpass",       # a tail with sites in different modes: two-pass fallback
    "one_bn2_frozen": lambda pre: pre != "dec_layer3.res.res1.bn2",
}


@pytest.mark.parametrize("case", sorted(MIXED))
def test_mixed_modes_match_oracle(golden_dir, case):
    train_of = MIXED[case]
    g, sd = _frozen_sd(golden_dir)
    x, lab, wgt = synthetic.make_batch(2, 64, 64, 1000)
    xt, lt, wt = torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(wgt)
    fwd = _uresnet_mixed(train_of)
    l32, g32, p32, ns = _oracle(fwd, sd, xt, lt, wt)
    l64, g64, _, _ = _oracle(fwd, _f64(sd), xt.double(), lt, wt.double())
    m = _model(sd)
    m.train()
    for name, mod in m.named_modules():
        if isinstance(mod, nn.BatchNorm2d) and not train_of(name):
            mod.eval()
    before = _stats(m)
    out, loss, grads = _step(m, xt, lt, wt)
    d = (out.cpu() - p32).abs()
    assert bool((d <= 1e-3 * p32.abs() + 1e-4).all()), "log-probabilities: worst per-element excess %.3e" % float((d - 1e-3 * p32.abs()).max())
    assert abs(loss - float(l32)) <= 1e-4 * abs(float(l32))
    # a conv bias in front of a train-mode BatchNorm stays analytically zero (the train tests' 1e-5)
    zero = [b for b, bn in (("conv1.bias", "bn1"), ("conv10.bias", "bn10")) if train_of(bn)]
    for b in zero:
        assert grads[b].abs().max().item() <= 1e-5, b
    fails = _judge(OrderedDict((n, v) for n, v in grads.items() if n not in zero), g32, OrderedDict((n, v) for n, v in g64.items() if n not in zero))
    assert not fails, "; ".join(fails[:8])
    after = _stats(m)
    for k in after:
        pre = k.rsplit(".", 1)[0]
        if not train_of(pre):
            assert torch.equal(after[k], before[k]), "%s of a frozen site changed" % k
        elif k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(before[k]) + 1, k
        else:
            assert _rel(after[k].cpu(), ns[k]) <= 1e-4, k       # as test_train_step_matches_reference_fixture_and_oracle


# ------------------------------------------------------------------------------------------ 4
def test_aspp_all_frozen(golden_dir):
    g = np.load(os.path.join(golden_dir, "aspp_ip16_norm_1x3x64x96.npz"))
    B, C, H, W, seed0, wseed = [int(v) for v in g["meta"]][:6]
    sd = O.state_dict_with_bn_stats(O.seeded_state_dict(O.aspp_resnet_schema(3, C, 16), wseed), g["bn_keys"], g["bn_stats"])
    x, lab, wgt = synthetic.make_batch(B, H, W, seed0, planes=C)
    xt, lt, wt = torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(wgt)
    l32, g32, p32, _ = _oracle(_eval_fwd(O.aspp_resnet_forward), sd, xt, lt, wt)
    l64, g64, _, _ = _oracle(_eval_fwd(O.aspp_resnet_forward), _f64(sd), xt.double(), lt, wt.double())
    m = ASPP_ResNet(num_classes=3, in_channels=C, inplanes=16, showsizes=False)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    before = _stats(m)
    out, loss, grads = _step(m, xt, lt, wt)
    d = (out.cpu() - p32).abs()
    assert bool((d <= 1e-3 * p32.abs() + 1e-4).all()), "log-probabilities: worst per-element excess %.3e" % float((d - 1e-3 * p32.abs()).max())
    assert abs(loss - float(l32)) <= 1e-4 * abs(float(l32))
    fails = _judge(grads, g32, g64, cos_min=0.999, l2_max=5e-2)       # the gates of test_aspp_train_step (same max-pool ties)
    assert not fails, "; ".join(fails[:8])
    for k, v in _stats(m).items():
        assert torch.equal(v, before[k]), k


# ------------------------------------------------------------------------------------------ 5
def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _close(got, ref, rel, what):
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e" % (what, err, scale)


# block tails of the ip16 network on 512x512 images: (side, channels) per level
TAIL_SHAPES = [(512, 16), (256, 32), (128, 64), (64, 128), (32, 256), (16, 512)]


@pytest.mark.parametrize("dt,N", [(torch.bfloat16, 16), (torch.float32, 2)])
@pytest.mark.parametrize("side,C", TAIL_SHAPES)
def test_one_pass_kernels_equal_two_pass(dt, N, side, C):
    """ubr_block_tail_bwd_frozen / ubr_bn_bwd_frozen against the two-pass kernels with k1 = k2 = 0: data gradients bit for bit
    (the same arithmetic per element), dgamma / dbeta within 4*tol(dt) of the two-pass sums (the bound of test_block_tail /
    test_bn_backward in test_gpu_ops.py: 2e-5 fp32, 1.2e-2 bf16, times 4, of the vector's largest entry)."""
    rtol = 4 * (2e-5 if dt == torch.float32 else 1.2e-2)
    gen = torch.Generator(device=DEV).manual_seed(1000 + side + C)
    cpu_ = 4 if dt == torch.float32 else 8
    shape = (N, side, side, C)
    npix = N * side * side
    T = lambda: torch.randn(shape, generator=gen, device=DEV).to(dt)
    V = lambda lo, hi: torch.rand(C, generator=gen, device=DEV) * (hi - lo) + lo
    go, go2, c2, cb = T(), T(), T(), T()
    mask = torch.randint(0, 256, (npix * (C // cpu_),), generator=gen, device=DEV, dtype=torch.uint8)
    s2, t2, m2, i2 = V(0.5, 1.5), V(-0.3, 0.3), V(-0.3, 0.3), V(0.7, 1.4)
    sb, mb, ib = V(0.5, 1.5), V(-0.3, 0.3), V(0.7, 1.4)
    zero = torch.zeros(C, device=DEV)
    stat = lambda: torch.zeros(32 * 2 * C, dtype=torch.float64, device=DEV)
    vec = lambda: torch.full((C,), float("nan"), device=DEV)
    for byp in (False, True):
        for second in (go2, None):
            r2, rb = stat(), stat()
            ops.block_tail_bwd_reduce(go, second, None, c2, s2, t2, m2, i2, cb if byp else None, mb if byp else None, ib if byp else None,
                                      r2, rb if byp else None, relu_mask=mask)
            ref_c2, ref_sc = torch.empty_like(c2), torch.empty_like(c2)
            ops.block_tail_bwd_apply(go, second, None, c2, s2, t2, m2, i2, zero, zero, cb if byp else None, sb if byp else None,
                                     mb if byp else None, ib if byp else None, zero if byp else None, zero if byp else None,
                                     ref_c2, ref_sc, relu_mask=mask)
            e = [vec() for _ in range(4)]
            k = torch.empty(2 * C, device=DEV)
            ops.bn_bwd_finalize(r2, npix, C, e[0], e[1], False, k[:C], k[C:])
            if byp:
                ops.bn_bwd_finalize(rb, npix, C, e[2], e[3], False, k[:C], k[C:])
            for lazy in ((False, True) if not byp else (False,)):
                f2, fb = stat(), stat()
                g_c2 = torch.full_like(c2, float("nan"))
                g_sc = None if lazy else torch.full_like(c2, float("nan"))
                ops.block_tail_bwd_frozen(go, second, mask, c2, s2, t2, m2, i2, f2, cb if byp else None, sb if byp else None,
                                          mb if byp else None, ib if byp else None, fb if byp else None, g_c2, g_sc)
                f = [vec() for _ in range(4)]
                kz = torch.full((2 * C,), float("nan"), device=DEV)
                ops.bn_bwd_finalize_frozen(f2, C, f[0], f[1], kz[:C], kz[C:])
                if byp:
                    ops.bn_bwd_finalize_frozen(fb, C, f[2], f[3])
                torch.cuda.synchronize()
                what = "tail %s C=%d byp=%d go2=%d lazy=%d" % (dt, C, byp, second is not None, lazy)
                assert torch.equal(_bits(g_c2), _bits(ref_c2)), what + ": g_c2"
                if not lazy:
                    assert torch.equal(_bits(g_sc), _bits(ref_sc)), what + ": g_sc"
                assert float(kz.abs().max()) == 0.0, what + ": k1 / k2 not zeroed"
                assert float(f2.view(32, -1)[8:].abs().max()) == 0.0, what + ": stripes beyond UBR_RED_SLOTS used"
                for got, ref, nm in list(zip(f, e, ("dgamma2", "dbeta2", "dgamma_b", "dbeta_b")))[:4 if byp else 2]:
                    _close(got, ref, rtol, what + ": " + nm)
    # single site
    for relu in (True, False):
        for second in (go2, None):
            r = stat()
            ops.bn_bwd_reduce(go, second, c2, s2, t2, m2, i2, relu, r)
            dg, db, k = vec(), vec(), torch.empty(2 * C, device=DEV)
            ops.bn_bwd_finalize(r, npix, C, dg, db, False, k[:C], k[C:])
            ref = torch.empty_like(c2)
            ops.bn_bwd_apply(go, second, c2, s2, t2, m2, i2, relu, zero, zero, ref)
            fr, gc, gp = stat(), torch.full_like(c2, float("nan")), torch.full_like(c2, float("nan"))
            ops.bn_bwd_frozen(go, second, c2, s2, t2, m2, i2, relu, fr, gc)
            ops.bn_bwd_frozen(go, second, c2, s2, t2, m2, i2, relu, None, gp)      # pure apply (sums formed by a conv epilogue)
            fg, fb_ = vec(), vec()
            ops.bn_bwd_finalize_frozen(fr, C, fg, fb_)
            torch.cuda.synchronize()
            what = "bn %s C=%d relu=%d ga2=%d" % (dt, C, relu, second is not None)
            assert torch.equal(_bits(gc), _bits(ref)) and torch.equal(_bits(gp), _bits(ref)), what + ": g_c"
            _close(fg, dg, rtol, what + ": dgamma")
            _close(fb_, db, rtol, what + ": dbeta")


# ------------------------------------------------------------------------------------------ 6
def _set_mode(m, frozen):
    m.eval() if frozen else m.train()


def test_modes_do_not_leak(golden_dir):
    """train step, frozen step, train step on ONE model at one shape: each bitwise the step a freshly built model takes from the
    same state (a launch tape or site vectors of the other mode would show)"""
    g, sd = _frozen_sd(golden_dir)
    x, lab, wgt = synthetic.make_batch(2, 64, 64, 1000)
    xt, lt, wt = torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(wgt)
    m = _model(sd)
    for i, frozen in enumerate((False, True, False, True)):
        state = OrderedDict((k, v.detach().clone()) for k, v in m.state_dict().items())
        fresh = _model(state)
        _set_mode(m, frozen)
        _set_mode(fresh, frozen)
        oa, la, ga = _step(m, xt, lt, wt)
        ob, lb, gb = _step(fresh, xt, lt, wt)
        assert torch.equal(oa, ob), "step %d (frozen=%s): log-probabilities differ from a fresh model's" % (i, frozen)
        for n in ga:
            assert torch.equal(ga[n], gb[n]), "step %d (frozen=%s): gradient of %s differs from a fresh model's" % (i, frozen, n)
        for (k, a), b in zip(_stats(m).items(), _stats(fresh).values()):
            assert torch.equal(a, b), "step %d: %s" % (i, k)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_frozen_backward_repeats_and_two_stream_equals_single_stream(golden_dir, dt, monkeypatch):
    """frozen steps in a row (the later ones replayed from the launch tape) are bitwise equal; UBR_WGRAD_STREAM=0 and 1 too
    (as test_two_stream_backward_equals_single_stream for train mode)"""
    g, sd = _frozen_sd(golden_dir)
    x, lab, wgt = synthetic.make_batch(2, 128, 128, 1000)
    xt, lt, wt = torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(wgt)
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("UBR_WGRAD_STREAM", mode)
        m = _model(sd)
        m.eval()
        m.compute_dtype = dt
        runs = [_step(m, xt, lt, wt) for _ in range(3)]
        for o, l, gr in runs[1:]:
            assert torch.equal(o, runs[0][0])
            for n in gr:
                assert torch.equal(gr[n], runs[0][2][n]), "stream mode %s: gradient of %s differs run to run" % (mode, n)
        res[mode] = runs[0]
    assert torch.equal(res["0"][0], res["1"][0])
    for n in res["0"][2]:
        assert torch.equal(res["0"][2][n], res["1"][2][n]), "gradient of %s: two-stream schedule differs from the single-stream one" % n


# ------------------------------------------------------------------------------------------ 7
def test_bf16_frozen_step_tracks_fp32(golden_dir):
    g, sd = _frozen_sd(golden_dir)
    x, lab, wgt = synthetic.make_batch(2, 128, 128, 1000)
    xt, lt, wt = torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(wgt)
    m = _model(sd)
    m.eval()
    _, l32, g32 = _step(m, xt, lt, wt)
    mb = _model(sd)
    mb.eval()
    mb.compute_dtype = torch.bfloat16
    _, l16, g16 = _step(mb, xt, lt, wt)
    print("frozen loss fp32 %.6f bf16 %.6f" % (l32, l16))
    assert abs(l16 - l32) <= 3e-2 * abs(l32)          # the bound of test_bf16_tracks_fp32
    assert all(bool(torch.isfinite(v).all()) for v in g16.values())


# ------------------------------------------------------------------------------------------ 8
def test_frozen_flat_adam_trajectory_matches_oracle(golden_dir):
    """five FlatAdam steps with every BatchNorm frozen track the CPU oracle's eval-mode trajectory (5e-3 per loss, the bound
    of test_training_trajectory_matches_oracle); the running statistics stay what they were"""
    g, sd = _frozen_sd(golden_dir)
    x, lab, wgt = synthetic.make_batch(2, 64, 64, 1000)
    xt, lt, wt = torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(wgt)
    m = _model(sd)
    m.eval()
    before = _stats(m)
    crit = PixelWiseNLLLoss()
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
    xd, ld, wd = xt.to(DEV), lt.to(DEV), wt.to(DEV)
    hip = []
    for _ in range(5):
        loss = crit(m(xd), ld, wd)
        opt.zero_grad()
        loss.backward()
        opt.step()
        hip.append(loss.item())
    p = OrderedDict((k, (v.clone().requires_grad_(True) if O.is_param_key(k) else v.clone())) for k, v in sd.items())
    oopt = torch.optim.Adam([v for k, v in p.items() if O.is_param_key(k)], lr=1e-3, weight_decay=1e-4)
    ref = []
    for _ in range(5):
        loss = O.pixelwise_nll(O.uresnet_forward(p, xt, False, None), lt, wt)
        oopt.zero_grad()
        loss.backward()
        oopt.step()
        ref.append(loss.item())
    print("frozen loss trajectories hip", hip, "oracle", ref)
    assert ref[-1] < ref[0]
    for a, b in zip(hip, ref):
        assert abs(a - b) <= 5e-3 * abs(b), "loss trajectory diverges: %s vs %s" % (hip, ref)
    for k, v in _stats(m).items():
        assert torch.equal(v, before[k]), k
