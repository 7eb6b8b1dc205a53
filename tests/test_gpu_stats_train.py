"""StatsGuard (ubresnet_amd/bnguard.py over libubresnet_stats.so) through UResNet(inplanes 16) at 1 x 1 x 64 x 64 and the real
train step, guarded FlatAdam, seeded synthetic batches g1, g2 and bad (= g2 with one NaN pixel):

1. the gap as it stands: without a StatsGuard, g1, bad leaves a non-finite running_mean while every parameter is finite;
2. with one, g1, bad, g2 ends bit-equal to g1, g2 -- parameters, both Adam moments, every BatchNorm buffer, the applied count --
   in fp32 and in bf16.  (This leans on the replayed pass being bitwise reproducible, which tools/reprocheck.py asserts; if the
   two runs ever differ, first establish whether g1, g2 differs from g1, g2.);
3. clean steps only: the guard changes nothing;
4. epoch.train(accumulate=2, stats_guard=sg) over g1, g1, g2, bad rolls the statistics back over the whole cycle;
5. a ParamEMA(buffers="average") beside it never sees the poisoned statistics;
6. a plain, unguarded FlatAdam: the scan alone restores;
7. resync() after load_state_dict, and the constructor's refusal of statistics that are already NaN."""
import pytest
import torch

import oracle.uresnet_oracle as O
from ubresnet_amd import synthetic

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd.bnguard import StatsGuard
    from ubresnet_amd.ema import ParamEMA
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training import epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

B_, H_, W_ = 1, 64, 64
HYP = dict(lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
STEM = "bn1.running_mean"


def _model(dtype=torch.float32):
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
    m = m.cuda().train()
    if dtype != torch.float32:
        m.compute_dtype = dtype
    return m


@pytest.fixture(scope="module")
def batches():
    g1 = tuple(torch.from_numpy(a).cuda() for a in synthetic.make_batch(B_, H_, W_, 1000))
    g2 = tuple(torch.from_numpy(a).cuda() for a in synthetic.make_batch(B_, H_, W_, 2000))
    x = g2[0].clone()
    x[0, 0, 31, 17] = float("nan")
    return dict(g1=g1, g2=g2, bad=(x, g2[1], g2[2]))


def _step(m, opt, crit, batch, sg=None, ema=None):
    x, lab, wgt = batch
    loss = crit.forward(m.forward(x), lab, wgt)
    opt.zero_grad()
    loss.backward()
    opt.step()
    if sg is not None:
        sg.resolve()
    if ema is not None:
        ema.update()


def _bits(t):
    return t.detach().reshape(-1).view(torch.int32) if t.is_floating_point() else t.detach().reshape(-1)


def _buffers(m):
    return {n: b.detach().clone() for n, b in m.named_buffers()}


def _state(m, opt):
    """everything a train step leaves behind, cloned"""
    torch.cuda.synchronize()
    s = {"flat": opt.flat.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone()}
    s.update({"buffer " + n: b for n, b in _buffers(m).items()})
    return s, (opt.guard.read()["applied"] if opt.guard is not None else opt.steps)


def _assert_same(a, b, what):
    (sa, na), (sb, nb) = a, b
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(_bits(sa[k]), _bits(sb[k])), "%s: %s differs" % (what, k)
    assert na == nb, "%s: applied steps %r vs %r" % (what, na, nb)


def _finite_stats(m):
    return all(bool(torch.isfinite(b).all()) for b in m.buffers() if b.is_floating_point())


def _run(seq, batches, dtype=torch.float32, guard=True, hyp=HYP, ema=False):
    m = _model(dtype)
    opt = FlatAdam(m, **hyp)
    sg = StatsGuard(m, optimizer=opt) if guard else None
    e = ParamEMA(opt, decay=0.9, buffers="average") if ema else None
    crit = PixelWiseNLLLoss()
    for name in seq:
        _step(m, opt, crit, batches[name], sg, e)
    torch.cuda.synchronize()
    crit.flush()
    return m, opt, sg, e


@pytest.fixture(scope="module")
def clean_fp32(batches):
    """g1, g2 without a StatsGuard: what legs 2 and 3 compare with"""
    m, opt, _, _ = _run(["g1", "g2"], batches, guard=False)
    return _state(m, opt)


def test_1_the_gap_as_it_stands(batches):
    m, opt, _, _ = _run(["g1", "bad"], batches, guard=False)
    nonfinite = [n for n, b in m.named_buffers() if n.endswith("running_mean") and not bool(torch.isfinite(b).all())]
    assert nonfinite, "the premise no longer holds: a NaN input pixel left every running_mean finite"
    assert STEM in nonfinite
    assert bool(torch.isfinite(opt.flat).all()), "a guarded optimizer let the bad step into the parameters"
    assert opt.guard.read()["skipped"] == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_2_a_bad_batch_costs_one_step_and_nothing_else(batches, clean_fp32, dtype):
    ma, oa, sg, _ = _run(["g1", "bad", "g2"], batches, dtype)
    a = _state(ma, oa)
    if dtype == torch.float32:
        b = clean_fp32
    else:
        mb, ob, _, _ = _run(["g1", "g2"], batches, dtype, guard=False)
        b = _state(mb, ob)
    _assert_same(a, b, "g1, bad, g2 with a StatsGuard against g1, g2")
    assert a[1] == 2 and "buffer bn1.num_batches_tracked" in a[0] and int(a[0]["buffer bn1.num_batches_tracked"]) == 2
    r = sg.read()
    assert r["restored"] == 1 and r["kept"] == 2 and r["restored_for_stats"] == 0 and r["bad_rows"] == 0
    assert STEM in r["bad_sites"] and r["bad_sites_last"] == []
    assert all(n.endswith(("running_mean", "running_var")) for n in r["bad_sites"])
    assert _finite_stats(ma) and sg.row().cpu().tolist() == [1, 0]


def test_3_clean_steps_are_left_alone(batches, clean_fp32):
    m, opt, sg, _ = _run(["g1", "g2"], batches)
    _assert_same(_state(m, opt), clean_fp32, "g1, g2 with a StatsGuard against without")
    r = sg.read()
    assert (r["kept"], r["restored"], r["restored_for_stats"], r["bad_rows"], r["bad_sites"]) == (2, 0, 0, 0, [])
    # the shadow is the live buffers at a step boundary: that is why there is no state_dict
    for (name, b, _, count), off in zip(sg._rows, sg._offs):
        assert torch.equal(sg.shadow[off:off + count], b.detach().reshape(-1).view(torch.int32)), name
    assert sg.names == [k for k in m.state_dict() if k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked")]
    assert len(sg.names) == 3 * 52


class _Feed(object):
    """a stager as far as epoch.train looks"""

    def __init__(self, items):
        self.items = list(items)

    def next(self):
        return self.items.pop(0)


def test_4_epoch_train_rolls_back_a_whole_accumulation_cycle(batches):
    ref, lines_ref = _model(), []
    epoch.train(_Feed([batches["g1"], batches["g1"]]), ref, PixelWiseNLLLoss(), FlatAdam(ref, **HYP), 2, print_freq=1, log=lines_ref.append,
                accumulate=2)
    m, lines = _model(), []
    opt = FlatAdam(m, **HYP)
    sg = StatsGuard(m, optimizer=opt)
    out = epoch.train(_Feed([batches[k] for k in ("g1", "g1", "g2", "bad")]), m, PixelWiseNLLLoss(), opt, 4, print_freq=1, log=lines.append,
                      accumulate=2, stats_guard=sg)
    torch.cuda.synchronize()
    want, got = _buffers(ref), _buffers(m)
    for n in want:
        assert torch.equal(_bits(got[n]), _bits(want[n])), "%s is not what it was after g1, g1" % n
    assert int(got["bn1.num_batches_tracked"]) == 2 and len(out) == 2
    # (the first line is logged before the first optimizer step of the epoch: like GradNorm, the figure appears with its first row)
    assert len(lines) == 5 and lines[-1].endswith("BNRestored 1") and lines[3].endswith("BNRestored 1"), lines
    assert lines[1].endswith("BNRestored 0") and lines[2].endswith("BNRestored 0") and "BNRestored" not in lines[0], lines
    assert not any("BNRestored" in l for l in lines_ref)
    r = sg.read()
    assert (r["kept"], r["restored"]) == (1, 1) and STEM in r["bad_sites"]
    assert opt.guard.read()["skipped"] == 1


def test_5_the_average_never_sees_the_poisoned_statistics(batches):
    m, opt, sg, ema = _run(["g1", "bad", "g2"], batches, ema=True)
    assert ema.stats is not None and bool(torch.isfinite(ema.stats).all()) and bool(torch.isfinite(ema.shadow).all())
    assert ema.held == 1 and ema.updates == 2 and _finite_stats(m)
    # resolve() over the average's values is a usage error
    with ema.applied():
        with pytest.raises(RuntimeError, match="swapped into the model"):
            sg.resolve()
    sg.resolve()
    torch.cuda.synchronize()
    assert sg.read()["kept"] == 3


def test_6_an_unguarded_optimizer_the_scan_alone_restores(batches):
    m, opt, sg, _ = _run(["g1"], batches, hyp=dict(lr=1e-3))
    assert opt.guard is None
    after_g1 = _buffers(m)
    _step(m, opt, PixelWiseNLLLoss(), batches["bad"], sg)
    torch.cuda.synchronize()
    r = sg.read()
    assert (r["kept"], r["restored"], r["restored_for_stats"], r["bad_rows"]) == (1, 1, 1, len(r["bad_sites_last"])) and r["bad_rows"] >= 1
    assert STEM in r["bad_sites"]
    got = _buffers(m)
    for n in after_g1:
        assert torch.equal(_bits(got[n]), _bits(after_g1[n])), n
    # check_nonfinite=False on an unguarded optimizer never restores: the statistics stay poisoned
    m2 = _model()
    opt2 = FlatAdam(m2, lr=1e-3)
    sg2 = StatsGuard(m2, optimizer=opt2, check_nonfinite=False)
    _step(m2, opt2, PixelWiseNLLLoss(), batches["bad"], sg2)
    torch.cuda.synchronize()
    assert sg2.read()["kept"] == 1 and not _finite_stats(m2)


def test_7_resync_and_the_refusal_of_poisoned_statistics(batches):
    m, opt, sg, _ = _run(["g1"], batches)
    other = {k: (v.detach().clone() + 1.0 if k.endswith(("running_mean", "running_var")) else v.detach().clone()) for k, v in m.state_dict().items()}
    m.load_state_dict(other)
    sg.resync()
    crit = PixelWiseNLLLoss()
    _step(m, opt, crit, batches["bad"], sg)
    torch.cuda.synchronize()
    got = m.state_dict()
    for k in other:
        assert torch.equal(_bits(got[k]), _bits(other[k])), "%s did not return to the loaded statistics" % k
    assert sg.read()["restored"] == 1 and STEM in sg.read()["bad_sites"]
    # a buffer whose storage was replaced is found again, and its shadow follows it
    m.bn1.running_mean = m.bn1.running_mean.detach().clone() + 2.0
    moved = m.bn1.running_mean.clone()
    sg.resolve()                                             # flag: the last step was skipped -> restore, from the new storage's values
    torch.cuda.synchronize()
    assert torch.equal(_bits(m.bn1.running_mean), _bits(moved))
    # poison from outside a train step: resync() and the constructor refuse, by name
    with torch.no_grad():
        m.bn1.running_var[3] = float("inf")
    with pytest.raises(ValueError, match="bn1.running_var"):
        sg.resync()
    with pytest.raises(ValueError, match="already non-finite at bn1.running_var"):
        StatsGuard(m, optimizer=opt)
    crit.flush()
