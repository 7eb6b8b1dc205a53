"""FlatAdam / FlatSGD with parameter groups and frozen parameters (ubresnet_amd/optim.py over libubresnet_group.so), through
UResNet(inplanes 16) at 1 x 1 x 64 x 64 and the real backward: one group == the plain optimizer bit for bit; two groups with a
frozen stem against torch.optim on the same groups and gradients, within the bound tests/test_gpu_optim.py applies to the
ungrouped optimizers (2e-5 of a tensor's largest magnitude); unfreezing and per-parameter step counts; state_dict interchange
with torch.optim; a learning-rate schedule; the guarded grouped optimizer and the epoch loop's log."""
import copy

import pytest
import torch

import kref
import oracle.uresnet_oracle as O
from ubresnet_amd import synthetic

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import optim
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam, FlatSGD
    from ubresnet_amd.staging import BatchStager
    from ubresnet_amd.training import epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

BOUND = 2e-5                       # tests/test_gpu_optim.py: worst |flat - torch| over a tensor's largest magnitude
B_, H_, W_ = 1, 64, 64
STEM = ("conv1.", "bn1.")           # with the dot: conv10, conv11 and bn10 are the head
ENC = ("conv1.", "bn1.", "enc_")


def _model():
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
    return m.cuda().train()


def _batch(i):
    return tuple(torch.from_numpy(a).cuda() for a in synthetic.make_batch(B_, H_, W_, 1000 + 7 * i))


def _maxrel(a, b):
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


def _worst(ma, mb):
    return max(_maxrel(p.detach(), q.detach()) for p, q in zip(ma.parameters(), mb.parameters()))


def _backward(m, i, crit):
    x, lab, wgt = _batch(i)
    for p in m.parameters():
        p.grad = None
    crit(m(x), lab, wgt).backward()


def _hand_over(ma, mb):
    """mb's parameters get clones of ma's gradients (None where ma has none)"""
    for p, q in zip(ma.parameters(), mb.parameters()):
        q.grad = None if p.grad is None else p.grad.detach().clone()


def _two_groups(m, **second):
    enc = [p for n, p in m.named_parameters() if n.startswith(ENC)]
    dec = [p for n, p in m.named_parameters() if not n.startswith(ENC)]
    return [{"params": enc, "lr": 1e-4, "weight_decay": 0.0}, dict({"params": dec}, **second)]


def _stem(m):
    return [(n, p) for n, p in m.named_parameters() if n.startswith(STEM)]


# ------------------------------------------------------------------------------------------------------------------------
# one group is the plain optimizer
# ------------------------------------------------------------------------------------------------------------------------
_SINGLE = {
    "adam": (lambda m, **kw: FlatAdam(m, lr=1e-3, weight_decay=1e-4, **kw), ("exp_avg", "exp_avg_sq")),
    "sgd": (lambda m, **kw: FlatSGD(m, lr=1e-2, momentum=0.9, weight_decay=1e-4, **kw), ("momentum_buffer",)),
    "adam-guarded": (lambda m, **kw: FlatAdam(m, lr=1e-3, weight_decay=1e-4, max_grad_norm=1e30, skip_nonfinite=True, **kw), ("exp_avg", "exp_avg_sq")),
    "sgd-guarded": (lambda m, **kw: FlatSGD(m, lr=1e-2, momentum=0.9, weight_decay=1e-4, max_grad_norm=1e30, skip_nonfinite=True, **kw), ("momentum_buffer",)),
}


@pytest.mark.parametrize("which", sorted(_SINGLE))
def test_a_single_group_is_the_plain_optimizer_bit_for_bit(which):
    make, buffers = _SINGLE[which]
    ma, mb = _model(), _model()
    oa = make(ma)
    ob = make(mb, groups=[{"params": list(mb.parameters())}])
    assert len(ob.param_groups) == 1 and ob.param_groups[0]["lr"] == oa.param_groups[0]["lr"]
    crit = PixelWiseNLLLoss()
    for i in range(3):
        _backward(ma, i, crit)
        _hand_over(ma, mb)
        oa.step()
        ob.step()
        torch.cuda.synchronize()
        kref.assert_bits(ob.flat, oa.flat, what="%s step %d: parameters" % (which, i + 1))
        for nm in buffers:
            kref.assert_bits(getattr(ob, nm), getattr(oa, nm), what="%s step %d: %s" % (which, i + 1, nm))
    assert not torch.equal(oa.flat, _model_flat_like(oa))
    if "guarded" in which:
        ra, rb = oa.guard.read(), ob.guard.read()
        assert (rb["applied"], rb["skipped"], rb["clipped_total"], rb["scale"]) == (3, 0, 0, 1.0) == (ra["applied"], ra["skipped"], ra["clipped_total"], ra["scale"])
        assert abs(rb["norm"] - ra["norm"]) <= 2.0 ** -22 * ra["norm"]       # two summation orders of one fp64 sum, rounded to fp32
    else:
        assert ob.guard is None
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sorted(sa["state"]) == sorted(sb["state"]) and sb["param_groups"][0]["params"] == sa["param_groups"][0]["params"]
    if "adam" in which:
        assert all(float(e["step"]) == 3.0 for e in sb["state"].values())


def _model_flat_like(opt):
    """the flat parameter buffer of a fresh model in opt's layout"""
    fresh = dict(_model().named_parameters())
    out = torch.zeros_like(opt.flat)
    for name, p, o in opt._layout:
        out[o:o + p.numel()].copy_(fresh[name].detach().reshape(-1))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# two groups, a frozen stem, unfreezing: one run per optimizer, shared by the tests below
# ------------------------------------------------------------------------------------------------------------------------
def _make(kind, m, flat, **kw):
    groups = _two_groups(m)
    if kind == "adam":
        return (FlatAdam(m, lr=1e-3, weight_decay=1e-4, groups=groups, **kw) if flat else torch.optim.Adam(groups, lr=1e-3, weight_decay=1e-4))
    return (FlatSGD(m, lr=1e-2, momentum=0.9, weight_decay=1e-4, groups=groups, **kw) if flat else torch.optim.SGD(groups, lr=1e-2, momentum=0.9, weight_decay=1e-4))


@pytest.fixture(scope="module", params=["adam", "sgd"])
def frozen_run(request):
    """3 steps; the stem (conv1, bn1) has requires_grad=False for the first two and is unfrozen before the third"""
    kind = request.param
    ma, mb = _model(), _model()
    for m in (ma, mb):
        for _, p in _stem(m):
            p.requires_grad_(False)
    oa, ob = _make(kind, ma, True), _make(kind, mb, False)
    initial = {n: p.detach().clone() for n, p in ma.named_parameters()}
    crit = PixelWiseNLLLoss()
    worst, frozen_same, had_grad = [], [], []
    for i in range(3):
        if i == 2:
            for m in (ma, mb):
                for _, p in _stem(m):
                    p.requires_grad_(True)
        _backward(ma, i, crit)
        had_grad.append([p.grad is not None for _, p in _stem(ma)])
        _hand_over(ma, mb)
        oa.step()                                   # no RuntimeError: the grouped optimizer takes a partially frozen model
        ob.step()
        torch.cuda.synchronize()
        worst.append(_worst(ma, mb))
        frozen_same.append(all(torch.equal(p.detach().view(torch.int32), initial[n].view(torch.int32)) for n, p in _stem(ma)))
    return dict(kind=kind, ma=ma, mb=mb, oa=oa, ob=ob, worst=worst, frozen_same=frozen_same, had_grad=had_grad, initial=initial)


def test_two_groups_with_a_frozen_stem_track_torch_optim(frozen_run):
    r = frozen_run
    assert r["had_grad"][0] == r["had_grad"][1] == [False] * len(_stem(r["ma"])) and all(r["had_grad"][2])
    assert r["frozen_same"][:2] == [True, True], "a frozen parameter changed"
    for i, w in enumerate(r["worst"]):
        assert w <= BOUND, "%s step %d: parameters drift from torch.optim by %.3e" % (r["kind"], i + 1, w)
    moved = [n for n, p in r["ma"].named_parameters() if not n.startswith(STEM) and not torch.equal(p.detach(), r["initial"][n])]
    assert len(moved) == len(list(r["ma"].parameters())) - len(_stem(r["ma"]))
    assert r["oa"].steps == 3
    assert [g["lr"] for g in r["oa"].param_groups] == [g["lr"] for g in r["ob"].param_groups]


def test_an_unfrozen_parameter_starts_at_step_one(frozen_run):
    r = frozen_run
    assert r["frozen_same"][2] is False, "the unfrozen stem did not move"
    sd = r["oa"].state_dict()
    index = r["oa"]._index
    stem_ids = sorted(index[id(p)] for _, p in _stem(r["ma"]))
    assert sorted(sd["state"]) == list(range(len(index)))
    if r["kind"] == "adam":
        for i, e in sd["state"].items():
            assert float(e["step"]) == (1.0 if i in stem_ids else 3.0), i
        ref = r["ob"].state_dict()["state"]
        assert all(float(ref[i]["step"]) == float(sd["state"][i]["step"]) for i in sd["state"])
    counts = r["oa"]._grouped.counts()
    seg = r["oa"]._segment_of()
    assert [int(counts[seg[i]]) for i in stem_ids] == [1] * len(stem_ids) and sorted(set(counts.tolist())) == [1, 3]


def test_state_dict_interchanges_with_torch_optim(frozen_run):
    r = frozen_run
    kind, sd = r["kind"], r["oa"].state_dict()
    keys = ("exp_avg", "exp_avg_sq") if kind == "adam" else ("momentum_buffer",)
    # torch.optim on the same grouping takes it ...
    fresh = _model()
    ot = _make(kind, fresh, False)
    ot.load_state_dict(copy.deepcopy(sd))
    back = ot.state_dict()
    assert [g["params"] for g in back["param_groups"]] == [g["params"] for g in sd["param_groups"]] and sorted(back["state"]) == sorted(sd["state"])
    assert [(g["lr"], g["weight_decay"]) for g in back["param_groups"]] == [(1e-4, 0.0), (1e-3 if kind == "adam" else 1e-2, 1e-4)]
    for i, e in sd["state"].items():
        for k in keys:
            assert torch.equal(back["state"][i][k].cpu(), e[k].cpu()), (i, k)
        if kind == "adam":
            assert float(back["state"][i]["step"]) == float(e["step"])
    # ... and torch.optim's loads into the flat optimizer: steps and moments come back equal
    ref = r["ob"].state_dict()
    m2 = _model()
    o2 = _make(kind, m2, True)
    o2.load_state_dict(copy.deepcopy(ref))
    sd2 = o2.state_dict()
    assert sorted(sd2["state"]) == sorted(ref["state"]) and [g["params"] for g in sd2["param_groups"]] == [g["params"] for g in ref["param_groups"]]
    for i, e in ref["state"].items():
        for k in keys:
            assert torch.equal(sd2["state"][i][k].cpu(), e[k].cpu()), (i, k)
        if kind == "adam":
            assert float(sd2["state"][i]["step"]) == float(e["step"])
    # and one more identical step from the loaded state agrees with torch's next step
    m2.load_state_dict(r["mb"].state_dict())
    crit = PixelWiseNLLLoss()
    _backward(m2, 3, crit)
    _hand_over(m2, r["mb"])
    o2.step()
    r["ob"].step()
    torch.cuda.synchronize()
    assert _worst(m2, r["mb"]) <= BOUND
    if kind == "adam":
        steps = sorted(set(float(e["step"]) for e in o2.state_dict()["state"].values()))
        assert steps == [2.0, 4.0]


def test_loading_a_state_without_entries_starts_from_zeros():
    """into an optimizer that has stepped: a parameter with no saved state restarts at step 1 on ZERO moments, as under torch"""
    m = _model()
    crit = PixelWiseNLLLoss()
    for kind, names in (("adam", ("exp_avg", "exp_avg_sq")), ("sgd", ("momentum_buffer",))):
        opt = _make(kind, m, True)
        _backward(m, 0, crit)
        opt.step()
        assert all(bool(getattr(opt, n).any()) for n in names)
        fresh = _make(kind, _model(), False).state_dict()           # torch.optim, never stepped: no state entries
        assert fresh["state"] == {}
        opt.load_state_dict(fresh)
        torch.cuda.synchronize()
        assert not any(bool(getattr(opt, n).any()) for n in names), "stale moments survive load_state_dict"
        assert opt.state_dict()["state"] == {} and int(opt._grouped.counts().max()) == 0


# ------------------------------------------------------------------------------------------------------------------------
# learning-rate schedule
# ------------------------------------------------------------------------------------------------------------------------
def test_a_step_lr_schedule_scales_the_next_update():
    def groups(m):
        g = _two_groups(m, lr=1e-2, weight_decay=0.0)
        g[0]["lr"] = 1e-1
        return g
    ma, mb = _model(), _model()
    oa = FlatSGD(ma, lr=1.0, groups=groups(ma))
    ob = torch.optim.SGD(groups(mb), lr=1.0)
    sa = torch.optim.lr_scheduler.StepLR(oa, step_size=1, gamma=0.1)
    sb = torch.optim.lr_scheduler.StepLR(ob, step_size=1, gamma=0.1)
    crit = PixelWiseNLLLoss()
    _backward(ma, 0, crit)
    grads = [p.grad.detach().clone() for p in ma.parameters()]
    flats = [oa.flat.clone()]
    for i in range(2):                              # the same gradient twice: no momentum, no decay, so update = lr * gradient
        for p, q, g in zip(ma.parameters(), mb.parameters(), grads):
            p.grad, q.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
        sa.step()
        sb.step()
        torch.cuda.synchronize()
        flats.append(oa.flat.clone())
        assert _worst(ma, mb) <= BOUND
        assert [g["lr"] for g in oa.param_groups] == [g["lr"] for g in ob.param_groups]
    assert [g["lr"] for g in oa.param_groups] == pytest.approx([1e-3, 1e-4])
    # per element: the stored parameter rounds each update by at most half an ulp of the parameter, so where the first update
    # is at least 100 ulps the ratio of the two is 0.1 within (0.5 + 0.05) / 100, the products lr * g within 2^-23 more
    d1, d2 = (flats[1] - flats[0]).double(), (flats[2] - flats[1]).double()
    ulp = 2.0 ** -23 * torch.maximum(torch.maximum(flats[0].abs(), flats[1].abs()), flats[2].abs()).double()
    clear = (d1.abs() >= 100 * ulp) & (d1 != 0)          # (padding floats: zero parameter, zero update)
    print("lr schedule: %d of %d elements with an update of 100 ulps or more" % (int(clear.sum()), d1.numel()))
    assert int(clear.sum()) > 1000
    worst = float((d2[clear] / d1[clear] - 0.1).abs().max())
    print("lr schedule: worst |second / first - 0.1| = %.3e" % worst)
    assert worst <= 6e-3, "the second update is not a tenth of the first: off by %.3e" % worst


# ------------------------------------------------------------------------------------------------------------------------
# the guarded grouped optimizer
# ------------------------------------------------------------------------------------------------------------------------
def _frozen_pair():
    ma, mb = _model(), _model()
    for m in (ma, mb):
        for _, p in _stem(m):
            p.requires_grad_(False)
    return ma, mb


def test_the_guard_clips_by_the_norm_of_the_active_parameters():
    ma, mb = _frozen_pair()
    crit = PixelWiseNLLLoss()
    _backward(ma, 0, crit)
    active = [p for p in ma.parameters() if p.grad is not None]
    norm64 = float(torch.sqrt(sum(p.grad.double().square().sum() for p in active)))
    # stale bytes of the frozen stem in the flat gradient buffer: poisoned, they must not reach the norm
    flat = ma.__dict__["_ubr_flat_grad"]
    probe = FlatAdam(ma, lr=1e-3, groups=_two_groups(ma), max_grad_norm=1e30, skip_nonfinite=True)
    for (name, p, o) in probe._layout:
        if name.startswith(STEM):
            flat[o:o + p.numel()] = float("nan")
    half = norm64 / 2
    oa = FlatAdam(ma, lr=1e-3, weight_decay=1e-4, groups=_two_groups(ma), max_grad_norm=half, skip_nonfinite=True)
    ob = torch.optim.Adam(_two_groups(mb), lr=1e-3, weight_decay=1e-4)
    _hand_over(ma, mb)
    torch.nn.utils.clip_grad_norm_([q for q in mb.parameters() if q.grad is not None], half)
    before = oa.flat.clone()
    oa.step()
    ob.step()
    torch.cuda.synchronize()
    r = oa.guard.read()
    assert abs(r["norm"] - norm64) <= 2.0 ** -22 * norm64 and abs(r["scale"] - 0.5) < 1e-5
    assert (r["applied"], r["skipped"], r["clipped_total"]) == (1, 0, 1)
    assert _worst(ma, mb) <= BOUND
    assert not torch.equal(oa.flat, before)
    assert oa.guard.row().tolist() == [r["norm"], r["scale"], 1.0]


def test_a_nan_gradient_step_is_skipped_and_no_count_advances():
    ma, _ = _frozen_pair()
    crit = PixelWiseNLLLoss()
    oa = FlatAdam(ma, lr=1e-3, weight_decay=1e-4, groups=_two_groups(ma), skip_nonfinite=True)
    snaps = []
    for i in range(3):
        _backward(ma, i, crit)
        if i == 1:
            ma.conv10.weight.grad.view(-1)[3] = float("nan")
        oa.step()
        snaps.append((oa.flat.clone(), oa.exp_avg.clone(), oa.exp_avg_sq.clone()))
    torch.cuda.synchronize()
    for a, b in zip(snaps[1], snaps[0]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the skipped step changed something"
    assert not torch.equal(snaps[2][0], snaps[1][0]) and all(bool(torch.isfinite(t).all()) for t in snaps[2])
    r = oa.guard.read()
    assert (r["applied"], r["skipped"]) == (2, 1) and oa.steps == 3
    sd = oa.state_dict()
    stem_ids = [oa._index[id(p)] for _, p in _stem(ma)]
    assert all(i not in sd["state"] for i in stem_ids), "a parameter that never stepped has a state entry"
    assert sorted(set(float(e["step"]) for e in sd["state"].values())) == [2.0]


def test_epoch_train_logs_the_norm_and_the_skips_of_a_grouped_optimizer():
    m = _model()
    for _, p in _stem(m):
        p.requires_grad_(False)
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4, groups=_two_groups(m), max_grad_norm=1e30, skip_nonfinite=True)
    ld = synthetic.SyntheticLArCVDataset(height=H_, width=W_, tag="train", nentries=16)
    ld.start(B_)
    lines = []
    with BatchStager(ld, B_, H_, W_, tag="train", timeout=20.0) as st:
        out = epoch.train(st, m, PixelWiseNLLLoss(), opt, 4, iiter=0, nclasses=3, print_freq=1, log=lines.append)
    assert len(out) == 2 and len(lines) == 5
    assert all("GradNorm" in l and "Skipped 0" in l for l in lines), lines
    r = opt.guard.read()
    assert r["applied"] == 4 and r["skipped"] == 0 and ("GradNorm %.3e" % r["norm"]) in lines[3]
    counts = opt._grouped.counts()
    assert sorted(set(counts.tolist())) == [0, 4]
