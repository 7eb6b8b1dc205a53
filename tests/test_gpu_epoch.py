"""ubresnet_amd.training.epoch on the device: train() against a plain loop that stops the host at every step, validate()
against the plain eval loop, and a resume from a checkpoint that carries live FlatAdam state."""
import pytest
import torch

import oracle.uresnet_oracle as O
from ubresnet_amd import synthetic

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import deploy, metrics
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.staging import BatchStager
    from ubresnet_amd.training import epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

B, H, W = 2, 64, 64


def _model():
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
    return m.cuda()


def _stager(**kw):
    ld = synthetic.SyntheticLArCVDataset(height=H, width=W, tag="train", nentries=64)
    ld.start(B)
    return BatchStager(ld, B, H, W, tag="train", timeout=20.0, **kw)


def _batch(i):
    return tuple(torch.from_numpy(a).cuda() for a in synthetic.make_batch(B, H, W, 1000 + B * i))


def _tensors(m, opt=None):
    out = {"param:" + n: p.detach().clone() for n, p in m.named_parameters()}
    out.update({"buffer:" + n: v.detach().clone() for n, v in m.named_buffers()})
    if opt is not None:
        out.update({"exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(), "steps": torch.tensor(opt.steps)})
    return out


def _differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(a[k], b[k])]


@pytest.fixture(scope="module")
def plain_run():
    """12 train steps the reference's way: loss.item() and accuracy() at every step"""
    m = _model().train()
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
    crit = PixelWiseNLLLoss()
    losses, accs = [], []
    for i in range(12):
        x, lab, wgt = _batch(i)
        pred = m.forward(x)
        loss = crit.forward(pred, lab, wgt)
        opt.zero_grad()
        loss.backward()
        opt.step()
        accs.append(metrics.accuracy(pred.detach(), lab))
        losses.append(loss.item())
    crit.flush()
    return dict(model=m, losses=losses, accs=accs, end=_tensors(m, opt))


def test_train_returns_what_the_plain_loop_computes(plain_run):
    m = _model()
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
    lines = []
    with _stager() as st:
        loss_avg, acc1_avg = epoch.train(st, m, PixelWiseNLLLoss(), opt, 12, iiter=3, nclasses=3, print_freq=5, log=lines.append)
    torch.cuda.synchronize()
    losses, accs = plain_run["losses"], plain_run["accs"]
    assert loss_avg == sum(losses) / 12 and acc1_avg == sum(a[1] for a in accs) / 12
    assert m.training and _differing(_tensors(m, opt), plain_run["end"]) == []
    assert len(lines) == 4 and lines[0].startswith("Train Iter: [3][0/12]") and lines[2].startswith("Train Iter: [3][10/12]")
    assert lines[-1].startswith("Train Iter [3] Ave:")


def test_the_loss_falls(plain_run):
    losses = plain_run["losses"]
    assert sum(losses[-3:]) / 3 < sum(losses[:3]) / 3, losses


def test_validate_returns_what_the_plain_eval_loop_computes(plain_run):
    m = plain_run["model"]
    before = _tensors(m)
    for p in m.parameters():
        p.grad = None
    with _stager() as st:
        st.skip(12)
        got = epoch.validate(st, m, PixelWiseNLLLoss(), 4, iiter=1, nclasses=3, print_freq=2, log=lambda s: None)
    assert isinstance(got, float) and not m.training
    assert all(p.grad is None for p in m.parameters()), "validate left a gradient"
    assert _differing(_tensors(m), before) == [], "validate touched a parameter or a running statistic"
    m.eval()
    tot = []
    with torch.no_grad():
        for i in range(12, 16):
            x, lab, wgt = _batch(i)
            tot.append(metrics.accuracy(m.forward(x), lab)[-1])
    assert got == sum(tot) / 4 and 0.0 < got <= 100.0
    m.train()


def _steps(m, opt, st, n):
    crit = PixelWiseNLLLoss()
    for _ in range(n):
        x, lab, wgt = st.next()
        loss = crit.forward(m.forward(x), lab, wgt)
        opt.zero_grad()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    crit.flush()


def test_resume_from_a_checkpoint_with_live_adam_state(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ma = _model().train()
    oa = FlatAdam(ma, lr=1e-3, weight_decay=1e-4)
    with _stager() as st:
        _steps(ma, oa, st, 3)
        name = deploy.save_checkpoint({"iter": 3, "epoch": 0, "state_dict": ma.state_dict(), "best_prec1": 0.0,
                                       "optimizer": oa.state_dict()}, False, 3)
        assert name == "checkpoint.3th.tar"
        _steps(ma, oa, st, 3)
    mb = _model().train()
    ob = FlatAdam(mb, lr=5e-2)                               # other hyper-parameters: the checkpoint's must win
    ckpt = torch.load(tmp_path / name, map_location="cpu", weights_only=True)
    assert ckpt["iter"] == 3 and sorted(ckpt) == ["best_prec1", "epoch", "iter", "optimizer", "state_dict"]
    mb.load_state_dict(ckpt["state_dict"])
    ob.load_state_dict(ckpt["optimizer"])
    with _stager() as st:
        st.skip(ckpt["iter"])
        _steps(mb, ob, st, 3)
    assert oa.steps == ob.steps == 6
    assert _differing(_tensors(mb, ob), _tensors(ma, oa)) == []
