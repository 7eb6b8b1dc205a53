"""The gradient-ready contract of the backward schedule, checked without a collective (single process).

Engine._stage_notifier (Python-scheduled passes) and plan.backward (replayed launch tapes) report ranges flat[lo:hi] of the
flat gradient buffer to model._grad_ready_hook while backward is still running, and GradAllReducer all-reduces them in
place at once.  tests/grad_ready_probe.py::FinalityProbe takes the reducer's place, waits for exactly what the reducer
waits for, and copies each range instead of exchanging it.  Every case asserts

  (a) the ranges tile the buffer in order, none empty, at least 12 of them (head, 5 decoder levels, 5 encoder levels, stem);
  (b) every copy equals the buffer's final content bit for bit: nothing was written after it was reported;
  (c) the final buffer equals, bit for bit, the one of the same pass with no hook installed.

The gradient buffer of the probed pass is filled with NaN before backward writes it (torch.empty and a replayed plan's
persistent buffer would otherwise show a too-early copy the previous, plausible, gradient), and the unprobed pass of (c) is
not poisoned: (c) therefore also says that every element is written by every pass and none is read before it is written.

Shapes: the smallest the networks accept with all five levels (H and W multiples of 32); UResNet 2x1x64x64, ASPP_ResNet
1x3x64x96.  Mixed BatchNorm mode: stem and encoder BatchNorms (for ASPP_ResNet the ASPP branch BatchNorms too) in eval mode
on the normalising running statistics of the frozen-BatchNorm fixtures, decoder and head in train mode -- the frozen sites'
dgamma / dbeta are then deferred to the end of their stage (Engine._fin_flush)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import uresnet_oracle as O
from ubresnet_amd import synthetic
from grad_ready_probe import FinalityProbe, freeze_encoder

if torch.cuda.is_available():
    from ubresnet_amd import plan
    from ubresnet_amd.engine import Engine
    from ubresnet_amd.models.ASPP_ResNet import ASPP_ResNet
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN = float("nan")
_SD = {}


def _state_dict(net):
    """seeded weights, with the running statistics of the frozen-BatchNorm fixture of that network (they normalise)"""
    if net not in _SD:
        if net == "uresnet":
            g = np.load(os.path.join(GOLDEN, "uresnet_ip16_frozen_2x1x64x64.npz"))
            sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), int(g["meta"][5]))
        else:
            g = np.load(os.path.join(GOLDEN, "aspp_ip16_norm_1x3x64x96.npz"))
            sd = O.seeded_state_dict(O.aspp_resnet_schema(3, 3, 16), int(g["meta"][5]))
        _SD[net] = O.state_dict_with_bn_stats(sd, g["bn_keys"], g["bn_stats"])
    return _SD[net]


def _model(net, dt, mixed, cls=None):
    if net == "uresnet":
        m = (cls or UResNet)(3, 1, 16)
    else:
        m = (cls or ASPP_ResNet)(3, 3, 16, showsizes=False)
    m.load_state_dict(_state_dict(net))
    m = m.cuda().train()
    if mixed:
        assert len(freeze_encoder(m)) >= 26
    m.compute_dtype = dt
    return m


def _batch(net, step):
    if net == "uresnet":
        x, lab, wgt = synthetic.make_batch(2, 64, 64, 1000 + 10 * step)
    else:
        x, lab, wgt = synthetic.make_batch(1, 64, 96, 1000 + 10 * step, planes=3)
    return torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(wgt).cuda()


def _bwd_plan(eng):
    for p in eng._planned.values():
        if p.bwd is not None:
            return p
    return None


def _poison_new_buffers(mp):
    """every parameter view of a newly allocated gradient buffer starts as NaN (the views, not the padding _grad_views zeroes)"""
    orig = Engine._grad_views

    def poisoned(self, dev):
        flat, views = orig(self, dev)
        for v in views.values():
            v.fill_(NAN)
        return flat, views
    mp.setattr(Engine, "_grad_views", poisoned)


def _passes(net, dt, mixed, steps, probed, monkeypatch, reference=None):
    """`steps` train passes (no optimizer: the weights stay, the input changes) -> ([final flat buffer per pass], [ranges per
    pass], engine).  probed: poison the gradient buffer before every backward, watch the pass with a FinalityProbe and check
    (a), (b) and -- against reference[i], the flat buffer of pass i of a plain run -- (c) after it"""
    crit = PixelWiseNLLLoss()
    flats, ranges = [], []
    with monkeypatch.context() as mp:
        if probed:
            _poison_new_buffers(mp)
        m = _model(net, dt, mixed)
        probe = FinalityProbe(m) if probed else None
        for i in range(steps):
            x, lab, wgt = _batch(net, i)
            m.zero_grad(set_to_none=True)
            loss = crit(m(x), lab, wgt)
            eng = m.__dict__["_ubr_engine"]
            if probed:
                p = _bwd_plan(eng)
                if p is not None:           # this backward will be replayed into the plan's persistent buffer
                    for v in p.views.values():
                        v.fill_(NAN)
                probe.reset()
            loss.backward()
            torch.cuda.synchronize()
            if probed:
                ranges.append(probe.check(eng, None if reference is None else reference[i]))
            flats.append(m.__dict__["_ubr_flat_grad"].clone())
    return flats, ranges, eng


def _report(tag, eng, ranges):
    last = ranges[-1][-1]
    print("grad-ready %s: %d ranges per pass, last (exposed) range %d bytes of %d" % (tag, len(ranges[-1]), 4 * (last[1] - last[0]), 4 * eng.grad_numel))


def _check_leg(net, dt, mixed, planned, monkeypatch):
    monkeypatch.setattr(plan, "ENABLED", planned)
    steps = 4 if planned else 1
    ref, _, _ = _passes(net, dt, mixed, steps, False, monkeypatch)
    assert all(torch.isfinite(f).all() for f in ref), "the plain pass's gradient is not finite"
    _, ranges, eng = _passes(net, dt, mixed, steps, True, monkeypatch, reference=ref)
    replayed = any(p.bwd is not None and p.uses >= 3 for p in eng._planned.values())
    assert replayed == planned, "launch plan %s" % ("was not replayed" if planned else "was used although disabled")
    assert all(r == ranges[0] for r in ranges), "replayed passes report other ranges than the recording pass"
    return eng, ranges


@pytest.mark.parametrize("mixed", [False, True], ids=["train", "mixed"])
@pytest.mark.parametrize("planned", [False, True], ids=["python", "replayed"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("net", ["uresnet", "aspp"])
def test_reported_ranges_are_final(net, dt, planned, mixed, monkeypatch):
    eng, ranges = _check_leg(net, dt, mixed, planned, monkeypatch)
    if planned:         # two streams produce the gradients: every stage carries a mark of each
        assert all(m1 is not None for _, _, _, m1 in _bwd_plan(eng).bwd.stages)
    _report("%s %s %s %s" % (net, str(dt).split(".")[1], "replayed" if planned else "python", "mixed" if mixed else "train"), eng, ranges)


@pytest.mark.parametrize("planned", [False, True], ids=["python", "replayed"])
@pytest.mark.parametrize("net", ["uresnet", "aspp"])
def test_reported_ranges_are_final_single_stream(net, planned, monkeypatch):
    """UBR_WGRAD_STREAM=0: weight gradients and their slab sums on the compute stream, no side-stream event or mark"""
    monkeypatch.setenv("UBR_WGRAD_STREAM", "0")
    eng, ranges = _check_leg(net, torch.float32, False, planned, monkeypatch)
    if planned:
        assert all(m1 is None for _, _, _, m1 in _bwd_plan(eng).bwd.stages)
    _report("%s fp32 %s train single-stream" % (net, "replayed" if planned else "python"), eng, ranges)


def test_hook_is_ignored_while_accumulating(monkeypatch):
    """a backward pass that finds .grad tensors adds into them: it must not report ranges (the reducer would exchange a buffer
    that .grad no longer aliases, autograd_fn._NetFn.backward), it announces itself through _grad_accum_pending once, and
    .grad is the sum of the two passes (tolerance of test_gpu_dp.py::test_grad_accumulates_like_autograd)"""
    crit = PixelWiseNLLLoss()
    single = []
    for i in range(2):
        m = _model("uresnet", torch.float32, False)
        x, lab, wgt = _batch("uresnet", i)
        crit(m(x), lab, wgt).backward()
        single.append({n: p.grad.clone() for n, p in m.named_parameters()})
    m = _model("uresnet", torch.float32, False)
    probe = FinalityProbe(m)
    pending = []
    m._grad_accum_pending = lambda: pending.append(1)
    x, lab, wgt = _batch("uresnet", 0)
    crit(m(x), lab, wgt).backward()
    torch.cuda.synchronize()
    probe.check(m.__dict__["_ubr_engine"])
    assert probe.calls >= 12 and not pending
    probe.reset()
    x, lab, wgt = _batch("uresnet", 1)
    crit(m(x), lab, wgt).backward()             # no zero_grad: gradients accumulate
    torch.cuda.synchronize()
    assert probe.calls == 0, "the hook was called %d times by an accumulating pass" % probe.calls
    assert len(pending) == 1, "_grad_accum_pending was called %d times" % len(pending)
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad, single[0][n] + single[1][n], rtol=1e-5, atol=1e-7), n


def test_probe_catches_a_parameter_reported_too_early(monkeypatch):
    """the finality check bites: with conv1.weight (written by the last launches of backward) moved to the front of the
    completion order, its slot is part of the head's range and is still poison when that range is reported.  Same kernels,
    same valid memory; only the layout of the flat buffer differs"""
    class Permuted(UResNet):
        def _grad_completion_order(self):
            order = UResNet._grad_completion_order(self)
            late = [e for e in order if e[0] == "conv1.weight"]
            return late + [e for e in order if e[0] != "conv1.weight"]

    monkeypatch.setattr(plan, "ENABLED", False)
    crit = PixelWiseNLLLoss()
    with monkeypatch.context() as mp:
        _poison_new_buffers(mp)
        m = _model("uresnet", torch.float32, False, Permuted)
        probe = FinalityProbe(m)
        x, lab, wgt = _batch("uresnet", 0)
        crit(m(x), lab, wgt).backward()
        torch.cuda.synchronize()
    eng = m.__dict__["_ubr_engine"]
    assert eng.grad_order[0][0] == "conv1.weight"
    with pytest.raises(AssertionError, match=r"stage 0 reported .* in parameter conv1\.weight"):
        probe.check(eng)
    # the gradient itself is complete and finite: only the promise about WHEN was broken
    assert torch.isfinite(m.__dict__["_ubr_flat_grad"]).all()
    # and the real order passes on the same pass
    _, ranges, _ = _passes("uresnet", torch.float32, False, 1, True, monkeypatch)
    assert len(ranges[0]) >= 12
