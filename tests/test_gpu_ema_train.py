"""ParamEMA (ubresnet_amd/ema.py over libubresnet_ema.so) through UResNet(inplanes 16) at 1 x 1 x 64 x 64 fp32 and the real
backward: six guarded steps with an update each against tests/ema_ref.py applied to parameter snapshots, bit for bit, the third
gradient poisoned; the same sequence captured in a graph; evaluation inside applied() against a fresh model that was loaded from
averaged_state_dict(), through the replayed launch plan; what applied() leaves behind; buffers="share"; the state_dict round
trip; deploy.load_model(ema=True); the epoch loops."""
import numpy as np
import pytest
import torch

import ema_ref as R
import kref
import oracle.uresnet_oracle as O
from ubresnet_amd import synthetic

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import deploy
    from ubresnet_amd.autograd_fn import _engine
    from ubresnet_amd.ema import ParamEMA
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam, FlatSGD
    from ubresnet_amd.staging import BatchStager
    from ubresnet_amd.training import epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

B_, H_, W_ = 1, 64, 64
HYP = dict(lr=1e-3, weight_decay=1e-4, max_grad_norm=1e30, skip_nonfinite=True)
DECAY, WARMUP = 0.999, 10
NSTEPS, POISON = 6, 2              # the gradient of the third step is poisoned


def _model():
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
    return m.cuda().train()


def _batch(i):
    return tuple(torch.from_numpy(a).cuda() for a in synthetic.make_batch(B_, H_, W_, 1000 + B_ * i))


def _backward(m, opt, crit, i, poison=False):
    x, lab, wgt = _batch(i)
    loss = crit.forward(m.forward(x), lab, wgt)
    opt.zero_grad()
    loss.backward()
    if poison:
        m.__dict__["_ubr_flat_grad"][opt._layout[0][2] + 1] = float("nan")


def _stats(m):
    return {n: b.detach().clone() for n, b in m.named_buffers() if b.is_floating_point()}


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def run():
    """six guarded Adam steps with an update after each; per step: clones of the gradient, the parameters, the moments, the
    running statistics, the shadow and the statistics' shadow; and the numpy replay of both shadows"""
    m = _model()
    opt = FlatAdam(m, **HYP)
    ema = ParamEMA(opt, decay=DECAY, warmup=WARMUP, buffers="average")
    crit = PixelWiseNLLLoss()
    ref_shadow = opt.flat.cpu().numpy().copy()
    ref_stats = {n: b.cpu().numpy().copy() for n, b in _stats(m).items()}
    ref, snaps = R.Ctl(), []
    for i in range(NSTEPS):
        _backward(m, opt, crit, i, poison=(i == POISON))
        grad = m.__dict__["_ubr_flat_grad"].clone()
        opt.step()
        ema.update()
        snap = dict(grad=grad, flat=opt.flat.clone(), exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone(), stats=_stats(m),
                    shadow=ema.shadow.clone(), shadow_stats=ema.stats.clone())
        if ref.advance(0 if i == POISON else 1, DECAY, WARMUP):
            ref_shadow = R.update(ref_shadow, snap["flat"].cpu().numpy(), ref.w)
            ref_stats = {n: R.update(v, snap["stats"][n].cpu().numpy(), ref.w) for n, v in ref_stats.items()}
        snap["ref_shadow"], snap["ref_stats"], snap["w"] = ref_shadow, ref_stats, float(ref.w)
        snaps.append(snap)
    torch.cuda.synchronize()
    crit.flush()
    return dict(m=m, opt=opt, ema=ema, crit=crit, snaps=snaps, ref=ref, counts=ema.counts(), skipped=opt.guard.read()["skipped"])


def test_the_shadow_is_the_replay_of_the_parameter_snapshots(run):
    ema, snaps = run["ema"], run["snaps"]
    for i, s in enumerate(snaps):
        kref.assert_bits(s["shadow"], torch.from_numpy(s["ref_shadow"]), what="step %d: shadow" % (i + 1))
        for name, b, off in ema._stats:
            kref.assert_bits(s["shadow_stats"][off:off + b.numel()].view(b.shape), torch.from_numpy(s["ref_stats"][name]),
                             what="step %d: shadow of %s" % (i + 1, name))
    assert len(ema._stats) == 104 and len(ema._params) == 165
    # the weights of the warm-up: 1 - (1 + u) / (10 + u) for u = 0, 1, (held), 2, 3, 4
    assert [s["w"] for s in snaps] == [float(np.float32(1.0 - (1.0 + u) / (10 + u))) for u in (0, 1, 1, 2, 3, 4)]
    assert not _bits_equal(snaps[-1]["shadow"], snaps[-1]["flat"]) and not _bits_equal(snaps[0]["shadow"], snaps[1]["shadow"])


def test_a_skipped_step_moves_nothing_and_is_counted_as_held(run):
    before, bad, after = run["snaps"][POISON - 1], run["snaps"][POISON], run["snaps"][POISON + 1]
    assert bool(torch.isnan(bad["grad"]).any())
    for key in ("flat", "exp_avg", "exp_avg_sq", "shadow", "shadow_stats"):
        assert _bits_equal(bad[key], before[key]), "the skipped step changed %s" % key
        assert not _bits_equal(after[key], bad[key]), "the step after it did not change %s" % key
    assert any(not _bits_equal(bad["stats"][n], before["stats"][n]) for n in bad["stats"])     # the forward did update the statistics
    assert run["counts"] == (NSTEPS - 1, 1) == (run["ref"].updates, run["ref"].held) and run["skipped"] == 1
    assert all(bool(torch.isfinite(run["snaps"][-1][k]).all()) for k in ("flat", "shadow", "shadow_stats"))


def test_a_captured_step_and_update_replay_to_the_same_bytes(run):
    """norm, step, advance, update: one linear capture, replayed over the eager run's gradients, the poisoned one included"""
    snaps = run["snaps"]
    m = _model()
    opt = FlatAdam(m, **HYP)
    ema = ParamEMA(opt, decay=DECAY, warmup=WARMUP, buffers="share")
    crit = PixelWiseNLLLoss()
    _backward(m, opt, crit, 0)                                  # the .grad tensors become views of the flat gradient buffer
    flat_grad = m.__dict__["_ubr_flat_grad"]
    assert opt._flat_grad() is flat_grad
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
        ema.update()
    torch.cuda.synchronize()
    assert _bits_equal(ema.shadow, opt.flat) and ema.updates == 0          # the capture ran nothing
    for i, s in enumerate(snaps):
        flat_grad.copy_(s["grad"])
        graph.replay()
        torch.cuda.synchronize()
        for key, got in (("flat", opt.flat), ("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq), ("shadow", ema.shadow)):
            kref.assert_bits(got, s[key], what="replay %d: %s" % (i + 1, key))
    assert (ema.updates, ema.held) == (NSTEPS - 1, 1)
    crit.flush()


def _plans(m):
    eng = _engine(m, "uresnet")
    return {k: (p.fwd, p.bwd) for k, p in eng._planned.items()}


def test_applied_evaluates_the_averaged_model_and_leaves_everything_as_it_was(run):
    m, opt, ema, crit = run["m"], run["opt"], run["ema"], run["crit"]
    x = _batch(50)[0]
    avg = ema.averaged_state_dict()
    assert set(avg) == set(m.state_dict()) and all(avg[k].data_ptr() != v.data_ptr() for k, v in m.state_dict().items())
    live_sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert all(torch.equal(avg[k], live_sd[k]) for k in avg if k.endswith("num_batches_tracked"))
    fresh = UResNet(num_classes=3, input_channels=1, inplanes=16)
    fresh.load_state_dict(avg)
    fresh = fresh.cuda().eval()
    ptrs = [p.data_ptr() for p in m.parameters()] + [b.data_ptr() for b in m.buffers()]
    flat0, shadow0, stats0 = opt.flat.clone(), ema.shadow.clone(), ema.stats.clone()
    with torch.no_grad():
        want = [fresh(x), fresh(x)][1]                           # the second call replays the fresh model's plan
        m.eval()
        live_out = m(x).clone()
        with ema.applied():
            assert _bits_equal(opt.flat, shadow0) and _bits_equal(ema.shadow, flat0)
            with pytest.raises(RuntimeError, match="swapped"):
                ema.update()
            with pytest.raises(RuntimeError, match="swapped"):
                with ema.applied():
                    pass
            warm = m(x).clone()
            plans = _plans(m)
            got = m(x)                                           # the replay of the plan the live weights recorded
            assert _plans(m) == plans
            torch.cuda.synchronize()
            kref.assert_bits(got, want, what="forward inside applied() against a fresh model with averaged_state_dict()")
            kref.assert_bits(warm, want, what="first forward inside applied()")
        m.train()
    assert not _bits_equal(live_out, want)
    # after exit: the bytes and the addresses are what they were
    assert _bits_equal(opt.flat, flat0) and _bits_equal(ema.shadow, shadow0) and _bits_equal(ema.stats, stats0)
    for k, v in m.state_dict().items():
        assert torch.equal(v.view(torch.uint8) if v.is_floating_point() else v, live_sd[k].view(torch.uint8) if v.is_floating_point() else live_sd[k]), k
    assert ptrs == [p.data_ptr() for p in m.parameters()] + [b.data_ptr() for b in m.buffers()]
    # an exception inside the block swaps back too
    with pytest.raises(ZeroDivisionError):
        with ema.applied():
            1 / 0
    torch.cuda.synchronize()
    assert _bits_equal(opt.flat, flat0) and not ema._swapped
    # the next train step replays its plans: none is recorded
    plans = _plans(m)
    train_keys = [k for k in plans if k[2]]
    assert train_keys and all(plans[k][0] is not None and plans[k][1] is not None for k in train_keys)
    uses = {k: _engine(m, "uresnet")._planned[k].uses for k in train_keys}
    _backward(m, opt, crit, NSTEPS)
    opt.step()
    ema.update()
    torch.cuda.synchronize()
    after = _plans(m)
    assert set(after) == set(plans) and all(after[k][0] is plans[k][0] and after[k][1] is plans[k][1] for k in plans), "a plan was recorded again"
    assert sum(_engine(m, "uresnet")._planned[k].uses - uses[k] for k in train_keys) == 1
    assert ema.updates == NSTEPS and not _bits_equal(opt.flat, flat0)
    crit.flush()


def test_state_dict_round_trip_continues_bit_for_bit(run):
    m, opt, ema, crit = run["m"], run["opt"], run["ema"], run["crit"]
    sd = ema.state_dict()
    assert sorted(sd) == ["buffers", "decay", "shadow", "stats", "updates", "warmup"]
    assert (sd["decay"], sd["warmup"], sd["buffers"], sd["updates"]) == (DECAY, WARMUP, "average", ema.updates)
    msd = m.state_dict()
    assert set(sd["shadow"]) == {n for n, _ in m.named_parameters()} and set(sd["stats"]) == {n for n in msd if n.endswith(("running_mean", "running_var"))}
    assert all(sd["shadow"][n].shape == msd[n].shape for n in sd["shadow"])
    m2 = _model()
    m2.load_state_dict({k: v.detach().clone() for k, v in msd.items()})
    opt2 = FlatAdam(m2, **HYP)
    opt2.load_state_dict(opt.state_dict())
    ema2 = ParamEMA(opt2, decay=0.5, warmup=0, buffers="average")
    ema2.load_state_dict(sd)
    assert (ema2.decay, ema2.warmup, ema2.updates, ema2.held) == (DECAY, WARMUP, ema.updates, 0)
    kref.assert_bits(ema2.shadow, ema.shadow, what="shadow through the state_dict")
    kref.assert_bits(ema2.stats, ema.stats, what="statistics' shadow through the state_dict")
    u = ema.updates
    _backward(m, opt, crit, NSTEPS + 1)
    for p, q in zip(m.parameters(), m2.parameters()):
        q.grad = p.grad.detach().clone()
    with torch.no_grad():
        for b, q in zip(m.buffers(), m2.buffers()):
            q.copy_(b)                                              # the statistics this forward left
    for o, e in ((opt, ema), (opt2, ema2)):
        o.step()
        e.update()
    torch.cuda.synchronize()
    kref.assert_bits(opt2.flat, opt.flat, what="parameters after the step")
    kref.assert_bits(ema2.shadow, ema.shadow, what="shadow after the next update")
    kref.assert_bits(ema2.stats, ema.stats, what="statistics' shadow after the next update")
    assert ema2.updates == ema.updates == u + 1
    h, h2 = ema.head(), ema2.head()
    assert (h.w, h.d) == (h2.w, h2.d) == tuple(float(v) for v in R.schedule(DECAY, WARMUP, u))           # the warm-up went on, not over
    # reset: the live weights again, the count from zero
    ema2.reset()
    assert _bits_equal(ema2.shadow, opt2.flat) and ema2.counts() == (0, 0)
    crit.flush()


def test_deploy_loads_the_averaged_weights(run, tmp_path):
    m, ema = run["m"], run["ema"]
    avg = ema.averaged_state_dict()
    path = str(tmp_path / "ckpt.tar")
    torch.save({"iter": 7, "state_dict": m.state_dict(), "ema": ema.state_dict()}, path)
    loaded = deploy.load_model(path, "cuda", num_classes=3, ema=True)
    assert not loaded.training
    for k, v in loaded.state_dict().items():
        assert torch.equal(v, avg[k]), k
    live = deploy.load_model(path, "cuda", num_classes=3)
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in live.state_dict().items())
    assert any(not torch.equal(v, avg[k]) for k, v in live.state_dict().items())
    bare = str(tmp_path / "bare.tar")
    torch.save({"iter": 7, "state_dict": m.state_dict()}, bare)
    with pytest.raises(KeyError, match="ema"):
        deploy.load_model(bare, "cuda", num_classes=3, ema=True)
    # copy_to_model is the same thing in place, one way
    m3 = _model()
    m3.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    e3 = ParamEMA(FlatSGD(m3, lr=1e-2, momentum=0.9), decay=DECAY, buffers="average")
    assert e3.opt.guard is None
    e3.load_state_dict(ema.state_dict())
    e3.copy_to_model()
    for k, v in m3.state_dict().items():
        assert torch.equal(v, avg[k]), k


def test_share_leaves_the_running_statistics_alone():
    m = _model()
    opt = FlatAdam(m, lr=1e-3)
    ema = ParamEMA(opt, decay=0.9, buffers="share")
    assert ema.stats is None and ema.state_dict()["stats"] == {} and opt.guard is None
    crit = PixelWiseNLLLoss()
    for i in range(2):
        _backward(m, opt, crit, i)
        opt.step()
        before = _stats(m)
        ema.update()
        torch.cuda.synchronize()
        assert all(_bits_equal(b, before[n]) for n, b in _stats(m).items())
    assert ema.counts() == (2, 0)                                   # no guard: every update is applied
    flat0 = opt.flat.clone()
    with ema.applied():
        torch.cuda.synchronize()
        assert all(_bits_equal(b, before[n]) for n, b in _stats(m).items()) and not _bits_equal(opt.flat, flat0)
    torch.cuda.synchronize()
    assert all(_bits_equal(b, before[n]) for n, b in _stats(m).items()) and _bits_equal(opt.flat, flat0)
    avg = ema.averaged_state_dict()
    assert all(torch.equal(avg[n], b) for n, b in before.items())
    crit.flush()


def test_epoch_train_updates_and_validate_evaluates_the_average():
    m = _model()
    opt = FlatAdam(m, **HYP)
    ema = ParamEMA(opt, decay=DECAY, warmup=WARMUP)
    ld = synthetic.SyntheticLArCVDataset(height=H_, width=W_, tag="train", nentries=16)
    ld.start(B_)
    lines, vlines = [], []
    with BatchStager(ld, B_, H_, W_, tag="train", timeout=20.0) as st:
        out = epoch.train(st, m, PixelWiseNLLLoss(), opt, 4, iiter=0, nclasses=3, print_freq=1, log=lines.append, ema=ema)
        torch.cuda.synchronize()
        flat0, shadow0, stats0 = opt.flat.clone(), ema.shadow.clone(), _stats(m)
        acc = epoch.validate(st, m, PixelWiseNLLLoss(), 2, iiter=0, nclasses=3, print_freq=1, log=vlines.append, ema=ema)
        torch.cuda.synchronize()
        assert _bits_equal(opt.flat, flat0) and _bits_equal(ema.shadow, shadow0) and not ema._swapped
        assert all(_bits_equal(b, stats0[n]) for n, b in _stats(m).items())
        plain = epoch.validate(st, m, PixelWiseNLLLoss(), 1, iiter=0, nclasses=3, print_freq=1, log=vlines.append)
    assert len(out) == 2 and len(lines) == 5 and isinstance(acc, float) and isinstance(plain, float)
    assert ["EMA %d/0" % (i + 1) in l for i, l in enumerate(lines[:4])] == [True] * 4 and "EMA 4/0" in lines[4], lines
    assert not any("EMA" in l for l in vlines)
    assert ema.counts() == (4, 0) and not _bits_equal(shadow0, flat0)
