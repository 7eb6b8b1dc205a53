"""GradAccumulator (ubresnet_amd/accum.py over libubresnet_accum.so) through UResNet(inplanes 16) at 1 x 1 x 64 x 64, fp32 and
bf16, and the real backward: the flat gradient after a cycle against tests/accum_ref.py applied to clones of the micro-batch
gradients, bit for bit; every micro-batch a replayed pass; three guarded Adam steps against the mean built by hand; a poisoned
micro-batch; a grouped optimizer with a frozen parameter; every=1; the error without zero_grad(); epoch.train(accumulate=2); one
rank under a forced GradAllReducer in a child process."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import accum_ref as R
import kref
import oracle.uresnet_oracle as O
from ubresnet_amd import synthetic

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from ubresnet_amd import accum
    from ubresnet_amd.accum import GradAccumulator
    from ubresnet_amd.autograd_fn import _engine
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.staging import BatchStager
    from ubresnet_amd.training import epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

B_, H_, W_ = 1, 64, 64
HYP = dict(lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
DTYPES = ["fp32", "bf16"]


def _model(dtype="fp32"):
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
    m = m.cuda().train()
    if dtype == "bf16":
        m.compute_dtype = torch.bfloat16
    return m


def _batch(i):
    return tuple(torch.from_numpy(a).cuda() for a in synthetic.make_batch(B_, H_, W_, 1000 + B_ * i))


def _backward(m, crit, i):
    """one micro-batch onto .grad tensors that are None -> the flat gradient buffer"""
    assert all(p.grad is None for p in m.parameters())
    x, lab, wgt = _batch(i)
    crit.forward(m.forward(x), lab, wgt).backward()
    return m.__dict__["_ubr_flat_grad"]


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _train_plans(m):
    return [p for k, p in _engine(m, "uresnet")._planned.items() if k[2] and k[4]]


# ------------------------------------------------------------------------------------------------------------------------
# one cycle
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_cycle_leaves_the_replay_of_the_micro_gradients_in_the_flat_buffer(dtype):
    m, crit = _model(dtype), PixelWiseNLLLoss()
    acc = GradAccumulator(m, every=2)
    assert (acc.every, acc.average, acc.pending) == (2, True, 0) and acc.buffer.numel() == _engine(m, "uresnet").grad_numel
    with pytest.raises(RuntimeError, match="no backward has run"):
        acc.add()
    clones = []
    for i in range(2):
        flat = _backward(m, crit, i)
        clones.append(flat.clone())
        last = acc.add()
        assert last == (i == 1) and acc.pending == (1 if i == 0 else 0)
        if not last:
            m.zero_grad()
    torch.cuda.synchronize()
    flat = m.__dict__["_ubr_flat_grad"]
    want = R.cycle([c.cpu().numpy() for c in clones], R.scale_of(2))
    kref.assert_bits(flat, torch.from_numpy(want), what="%s: the flat gradient after the cycle, padding included" % dtype)
    assert not _bits_equal(clones[0], clones[1]) and not _bits_equal(flat, clones[1]) and bool(torch.isfinite(flat).all())
    eng = _engine(m, "uresnet")
    base = flat.data_ptr()
    for name, p in eng.grad_order:
        assert p.grad is not None and p.grad.data_ptr() == base + 4 * eng.grad_offsets[name] and p.grad.shape == p.shape, name
    kref.assert_bits(acc.buffer, clones[0], what="the accumulator after the cycle: the first micro-batch, untouched by the last call")
    crit.flush()


def test_after_a_warm_up_cycle_every_backward_is_a_replay():
    m, crit = _model("bf16"), PixelWiseNLLLoss()
    acc = GradAccumulator(m, every=2)
    for i in range(2):                                       # the warm-up cycle records the forward and the backward tape
        _backward(m, crit, i)
        acc.add()
        m.zero_grad()
    plans = _train_plans(m)
    assert len(plans) == 1 and plans[0].fwd is not None and plans[0].bwd is not None
    plan, uses, bwd = plans[0], plans[0].uses, plans[0].bwd
    for i in range(2, 4):
        flat = _backward(m, crit, i)
        assert flat is plan.flat and m._ubr_flat_grad is plan.flat, "an eager pass handed out a fresh buffer"
        assert m.__dict__["_ubr_grad_accumulated"] is False
        acc.add()
        m.zero_grad()
    torch.cuda.synchronize()
    assert _train_plans(m) == [plan] and plan.bwd is bwd and plan.uses == uses + 2
    crit.flush()


# ------------------------------------------------------------------------------------------------------------------------
# optimizer steps
# ------------------------------------------------------------------------------------------------------------------------
def _steps(make_opt, through, dtype="fp32", nsteps=3, every=2, poison=None, first=0):
    """`nsteps` optimizer steps of `every` micro-batches each.  through="acc": GradAccumulator; "hand": the mean is built from the
    cloned micro-gradients with accum_ref on the host and copied into the flat buffer before step(); "plain" (every == 1): no
    accumulator at all.  poison=(step, micro): a NaN is planted in that micro-batch's gradient.  -> per step clones of the
    parameters and both moments, and the model and optimizer"""
    m, crit = _model(dtype), PixelWiseNLLLoss()
    opt = make_opt(m)
    acc = GradAccumulator(m, every=every) if through == "acc" else None
    snaps = []
    for s in range(nsteps):
        clones = []
        for k in range(every):
            opt.zero_grad()
            flat = _backward(m, crit, first + s * every + k)
            if poison == (s, k):
                flat[opt._layout[0][2] + 1] = float("nan")
            if acc is not None:
                assert acc.add() == (k == every - 1)
            else:
                clones.append(flat.clone())
        if through == "hand":
            mean = R.cycle([c.cpu().numpy() for c in clones], R.scale_of(every))
            m.__dict__["_ubr_flat_grad"].copy_(torch.from_numpy(mean))
        opt.step()
        snaps.append(dict(flat=opt.flat.clone(), exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone()))
    torch.cuda.synchronize()
    crit.flush()
    return snaps, m, opt


def _same(a, b, what):
    assert len(a) == len(b)
    for s, (x, y) in enumerate(zip(a, b)):
        for key in ("flat", "exp_avg", "exp_avg_sq"):
            kref.assert_bits(x[key], y[key], what="%s: step %d: %s" % (what, s + 1, key))


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_guarded_steps_equal_the_mean_built_by_hand(dtype):
    mk = lambda m: FlatAdam(m, **HYP)
    got, m, opt = _steps(mk, "acc", dtype)
    want, _, opt2 = _steps(mk, "hand", dtype)
    _same(got, want, dtype)
    assert opt.steps == opt2.steps == 3 and opt.guard.read()["skipped"] == 0
    assert not _bits_equal(got[0]["flat"], got[1]["flat"]) and not _bits_equal(got[1]["flat"], got[2]["flat"])
    assert bool(torch.isfinite(got[-1]["flat"]).all())


def test_a_poisoned_micro_batch_skips_that_step_and_the_next_cycle_applies():
    mk = lambda m: FlatAdam(m, **HYP)
    got, m, opt = _steps(mk, "acc", nsteps=3, poison=(1, 0))               # the FIRST micro-batch of the second step: it goes through ubc_set
    for key in ("flat", "exp_avg", "exp_avg_sq"):
        assert _bits_equal(got[1][key], got[0][key]), "the skipped step changed %s" % key
        assert not _bits_equal(got[2][key], got[1][key]), "the step after it did not change %s" % key
    r = opt.guard.read()
    assert (opt.steps, r["skipped"], r["applied"]) == (3, 1, 2) and bool(torch.isfinite(got[2]["flat"]).all())
    late, _, opt2 = _steps(mk, "acc", nsteps=2, poison=(1, 1))             # the LAST micro-batch: it goes through ubc_finish
    assert _bits_equal(late[1]["flat"], late[0]["flat"]) and opt2.guard.read()["skipped"] == 1
    _same(late[:1], got[:1], "the first step of both runs")


def test_a_grouped_optimizer_with_a_frozen_parameter_ignores_the_stale_bytes():
    def mk(m):
        frozen = m.conv10.weight
        frozen.requires_grad_(False)
        rest = [p for p in m.parameters() if p is not frozen]
        return FlatAdam(m, groups=[{"params": rest[:40], "lr": 1e-4}, {"params": rest[40:]}], **HYP)
    got, m, opt = _steps(mk, "acc")
    want, m2, _ = _steps(mk, "hand")
    _same(got, want, "grouped, conv10.weight frozen")
    assert m.conv10.weight.grad is None and opt.steps == 3 and opt.guard.read()["skipped"] == 0
    o = dict((name, off) for name, _, off in opt._layout)["conv10.weight"]
    n = m.conv10.weight.numel()
    fresh = _model()
    assert _bits_equal(opt.flat[o:o + n], fresh.conv10.weight.detach().reshape(-1)), "the frozen parameter moved"
    assert not bool(opt.exp_avg[o:o + n].any())
    assert bool(m.__dict__["_ubr_flat_grad"][o:o + n].any()), "the backward left no bytes at the frozen parameter: nothing stale was summed"


def test_every_1_launches_nothing_and_is_the_run_without_an_accumulator(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GradAccumulator(every=1) launched a kernel")
    for name in ("set_", "add", "finish"):
        monkeypatch.setattr(accum.A, name, boom)
    mk = lambda m: FlatAdam(m, **HYP)
    got, m, _ = _steps(mk, "acc", nsteps=2, every=1)
    want, _, _ = _steps(mk, "plain", nsteps=2, every=1)
    _same(got, want, "every=1")
    acc = GradAccumulator(m, every=1)
    assert acc.buffer is None and acc.add() is True and acc.pending == 0


def test_add_raises_after_a_backward_onto_existing_gradients():
    m, crit = _model(), PixelWiseNLLLoss()
    acc = GradAccumulator(m, every=3)
    _backward(m, crit, 0)
    assert acc.add() is False
    x, lab, wgt = _batch(1)
    crit.forward(m.forward(x), lab, wgt).backward()                         # no zero_grad(): the legacy accumulating pass
    with pytest.raises(RuntimeError, match="missing zero_grad"):
        acc.add()
    assert acc.pending == 1
    m.zero_grad()
    acc.reset()
    assert acc.pending == 0
    _backward(m, crit, 2)
    assert acc.add() is False and acc.pending == 1                          # a plain pass again: accepted
    # a .grad that was replaced by a tensor of the caller's is the other documented cause
    m.conv10.weight.grad = m.conv10.weight.grad.clone()
    with pytest.raises(RuntimeError, match="conv10.weight is not the view of the flat gradient buffer"):
        acc.add()
    m2 = _model()
    a2 = GradAccumulator(m2, every=2)
    m2.__dict__["_ubr_flat_grad"] = torch.zeros(a2.buffer.numel() + 4, device="cuda")     # another network's layout
    with pytest.raises(RuntimeError, match="the flat gradient buffer is"):
        a2.add()
    crit.flush()


# ------------------------------------------------------------------------------------------------------------------------
# the epoch loop
# ------------------------------------------------------------------------------------------------------------------------
def _stager():
    ld = synthetic.SyntheticLArCVDataset(height=H_, width=W_, tag="train", nentries=16)
    ld.start(B_)
    return BatchStager(ld, B_, H_, W_, tag="train", timeout=20.0)


def _untimed(lines):
    """log lines without the host times (Batch / Data), which differ from run to run"""
    return [re.sub(r"Batch [0-9.]+( \([0-9.]+\))?\s+Data [0-9.]+( \([0-9.]+\))?", "Batch - Data -", l) for l in lines]


def test_epoch_train_with_accumulate_2_steps_every_second_batch():
    m = _model()
    opt = FlatAdam(m, **HYP)
    lines = []
    with _stager() as st:
        out = epoch.train(st, m, PixelWiseNLLLoss(), opt, 4, iiter=0, nclasses=3, print_freq=1, log=lines.append, accumulate=2)
    torch.cuda.synchronize()
    want, _, opt2 = _steps(lambda mm: FlatAdam(mm, **HYP), "acc", nsteps=2)             # the hand-written loop over the same 4 batches
    assert opt.steps == 2 == opt2.steps
    for key, t in (("flat", opt.flat), ("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq)):
        kref.assert_bits(t, want[-1][key], what="epoch.train(accumulate=2): %s" % key)
    assert len(out) == 2 and len(lines) == 5
    assert "GradNorm" not in lines[0] and "Skipped" not in lines[0]                    # no step yet after the first batch
    assert all("Skipped 0" in l for l in lines[1:]), lines                             # a batch without a step is not a skipped step
    norms = [re.search(r"GradNorm (\S+) \((\S+)\)", l).groups() for l in lines[1:]]
    assert float(norms[0][0]) > 0 and norms[0] == norms[1] and norms[2] == norms[3] and norms[2] != norms[0]   # the meters move on the second and fourth batch only


def test_epoch_train_with_accumulate_1_is_the_call_without_the_argument():
    runs = []
    for kw in (dict(), dict(accumulate=1)):
        m = _model()
        opt = FlatAdam(m, **HYP)
        lines = []
        with _stager() as st:
            out = epoch.train(st, m, PixelWiseNLLLoss(), opt, 4, iiter=2, nclasses=3, print_freq=2, log=lines.append, **kw)
        torch.cuda.synchronize()
        runs.append((out, _untimed(lines), opt.flat.clone(), opt.steps))
    (out0, lines0, flat0, steps0), (out1, lines1, flat1, steps1) = runs
    assert out0 == out1 and lines0 == lines1 and steps0 == steps1 == 4 and _bits_equal(flat0, flat1)
    assert len(lines0) == 3 and "Batch - Data -" in lines0[0] and "Skipped 0" in lines0[-1]


# ------------------------------------------------------------------------------------------------------------------------
# data parallel: one rank, the reducer forced
# ------------------------------------------------------------------------------------------------------------------------
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(port, q):
    """two steps of two micro-batches, with a GradAllReducer that exchanges every micro-batch bucket by bucket although there is
    one rank (UBR_FORCE_REDUCER=1) and without one: an average over one rank is the identity, so the parameters are bit-equal"""
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), UBR_FORCE_REDUCER="1")
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    from ubresnet_amd.dist import GradAllReducer
    res = {}
    for with_reducer in (True, False):
        m, crit = _model("bf16"), PixelWiseNLLLoss()
        opt = FlatAdam(m, **HYP)
        red = GradAllReducer(m, bucket_bytes=1 << 20) if with_reducer else None
        acc = GradAccumulator(m, every=2)
        forced = red is not None and red.force
        for i in range(4):
            opt.zero_grad()
            _backward(m, crit, i)
            if red is not None:
                red.finish()
            if acc.add():
                opt.step()
        torch.cuda.synchronize()
        crit.flush()
        plans = _train_plans(m)
        res[with_reducer] = (opt.flat.clone(), opt.exp_avg.clone(), opt.steps, forced, len(plans) == 1 and plans[0].uses == 4)
    a, b = res[True], res[False]
    ok = bool(_bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1]) and a[2] == b[2] == 2 and a[3] and not b[3] and a[4] and b[4]
              and torch.isfinite(a[0]).all().item())
    q.put((ok, a[2], b[2], a[3], a[4], b[4]))
    dist.destroy_process_group()


def test_one_rank_under_a_forced_reducer_equals_the_run_without_one():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_worker, args=(_free_port(), q))
    p.start()
    res = q.get(timeout=600)
    p.join(timeout=60)
    assert res[0] is True, res
