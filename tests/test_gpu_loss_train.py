"""PixelWiseFocalLoss (ubresnet_amd/training/pixelwise_focalloss.py over libubresnet_loss.so) through UResNet(inplanes 16) at
2 x 1 x 64 x 64 and the real train step, seeded synthetic batches:

1. a step with PixelWiseFocalLoss(gamma=0) leaves all 165 gradients bit-equal to the same step with PixelWiseNLLLoss;
2. a step with gamma=2, normalize="weights": the gradient w.r.t. the log-probabilities against tests/loss_ref.py within its bound,
   a finite non-zero gradient norm, and the same bits from run to run;
3. epoch.train and epoch.validate over 4 batches with the focal criterion, a guarded FlatAdam and PixelWeights: finite meters;
4. a batch with a label out of range raises from flush();
5. read() against the reference's per-class means; double backward raises."""
import math

import numpy as np
import pytest
import torch

import loss_ref as R
import oracle.uresnet_oracle as O
from ubresnet_amd import synthetic

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.pixel_weights import PixelWeights
    from ubresnet_amd.training import PixelWiseFocalLoss, epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

B_, H_, W_ = 2, 64, 64


def _model():
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
    return m.cuda().train()


@pytest.fixture(scope="module")
def batch():
    return tuple(torch.from_numpy(a).cuda() for a in synthetic.make_batch(B_, H_, W_, 1000))


def _grads(crit, batch):
    m = _model()
    x, lab, wgt = batch
    loss = crit.forward(m.forward(x), lab, wgt)
    loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}, float(loss.detach())


def test_1_gamma_0_trains_as_the_nll_loss_bit_for_bit(batch):
    want, loss_want = _grads(PixelWiseNLLLoss(), batch)
    got, loss_got = _grads(PixelWiseFocalLoss(gamma=0.0), batch)
    assert len(want) == len(got) == 165
    for n in want:
        assert torch.equal(got[n].view(torch.int32), want[n].view(torch.int32)), "%s differs" % n
    assert abs(loss_got - loss_want) <= float(np.spacing(np.float32(abs(loss_want))))
    PixelWiseFocalLoss.flush()


def test_2_a_focal_step_over_weighted_means(batch):
    x, lab, wgt = batch
    crit = PixelWiseFocalLoss(weight=torch.tensor([0.5, 2.0, 4.0]), gamma=2.0, normalize="weights")
    m = _model()
    logp = m.forward(x).detach().clone().requires_grad_(True)
    loss = crit(logp, lab, wgt)
    loss.backward()
    torch.cuda.synchronize()
    f = R.forward(logp.detach().cpu().numpy(), lab.cpu().numpy(), wgt.cpu().numpy(), np.float32([0.5, 2.0, 4.0]), -100, 2.0, "weights")
    want, lim, hot = R.backward(1.0, f, 2.0, 3)
    g = logp.grad.cpu().numpy()
    ratio = float((np.abs(g.astype(np.float64) - want)[hot] / lim[hot]).max())
    print("gamma 2, weights: worst gradient error / bound %.3f; loss %.9g (reference %.9g)" % (ratio, float(loss), f["loss"]))
    assert ratio <= 1.0 and not g[~hot].any() and not np.signbit(g[~hot]).any()
    # the weight sum is a sum of fp32 products in fp64, as the reference forms it; the mean is one fp64 product rounded to fp32
    r = crit.read()
    assert r["valid"] == f["valid"] and abs(r["denom"] - f["denom"]) <= 1e-12 * f["denom"] and r["per_class_pixels"] == f["class_pixels"]
    assert abs(float(loss) - f["loss"]) <= f["lim_sum"] / f["denom"] + 2.0 ** -24 * abs(f["loss"])
    # the whole step: a finite, non-zero gradient norm, and the same bits from run to run
    a, la = _grads(crit, batch)
    b, lb = _grads(crit, batch)
    norm = math.sqrt(sum(float(v.double().pow(2).sum()) for v in a.values()))
    assert math.isfinite(norm) and norm > 0.0 and la == lb
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), "%s differs from run to run" % n
    crit.flush()


class _Feed(object):
    """a stager as far as the epoch loops look"""

    def __init__(self, items):
        self.items = list(items)

    def next(self):
        return self.items.pop(0)


def test_3_the_epoch_loops_take_the_criterion_as_it_is():
    pw = PixelWeights(num_classes=3, radius=1, gain=2.0)
    items = []
    for seed in (1000, 2000, 3000, 4000):
        x, lab, _ = (torch.from_numpy(a).cuda() for a in synthetic.make_batch(B_, H_, W_, seed))
        items.append((x, lab, pw(lab)))
    m = _model()
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    crit = PixelWiseFocalLoss(gamma=2.0, normalize="weights")
    lines = []
    loss, acc = epoch.train(_Feed(items), m, crit, opt, 4, print_freq=2, log=lines.append)
    assert math.isfinite(loss) and loss > 0.0 and math.isfinite(acc)
    assert opt.guard.read()["applied"] == 4 and all(bool(torch.isfinite(p).all()) for p in m.parameters())
    total = epoch.validate(_Feed(items), m, crit, 4, print_freq=2, log=lines.append)
    assert math.isfinite(total) and 0.0 <= total <= 100.0
    assert any(l.startswith("Train Iter") for l in lines) and any(l.startswith("Test:Result*") for l in lines)
    r = crit.read()
    assert r["valid"] == B_ * H_ * W_ and math.isfinite(r["loss"]) and sum(r["per_class_pixels"]) == r["valid"]


def test_4_a_label_out_of_range_raises_from_flush(batch):
    x, lab, wgt = batch
    lab = lab.clone()
    lab[1, 5, 7] = 3
    crit = PixelWiseFocalLoss(gamma=2.0)
    logp = _model().forward(x).detach().requires_grad_(True)
    loss = crit(logp, lab, wgt)                               # a loss with a gradient: the count is reported later
    with pytest.raises(RuntimeError, match=r"1 target label\(s\) outside \[0, 3\)"):
        crit.flush()
    assert math.isfinite(float(loss)) and crit.read()["valid"] == B_ * H_ * W_ - 1
    crit.flush()                                              # reported once
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r"outside \[0, 3\)"):
            crit(logp.detach(), lab, wgt)                     # without a gradient: at once


def test_5_read_and_double_backward(batch):
    x, lab, wgt = batch
    lab = lab.clone()
    lab[0, :4] = -100
    crit = PixelWiseFocalLoss(gamma=0.5, normalize="valid")
    logp = _model().forward(x).detach().requires_grad_(True)
    loss = crit(logp, lab, wgt)
    r = crit.read()
    f = R.forward(logp.detach().cpu().numpy(), lab.cpu().numpy(), wgt.cpu().numpy(), None, -100, 0.5, "valid")
    assert r["valid"] == f["valid"] == B_ * H_ * W_ - 4 * W_ and r["denom"] == float(f["valid"]) and r["per_class_pixels"] == f["class_pixels"]
    assert r["loss"] == float(loss) and abs(r["loss"] - f["loss"]) <= f["lim_sum"] / f["denom"] + 2.0 ** -24 * abs(f["loss"])
    for got, want, n in zip(r["per_class_loss"], f["per_class_loss"], f["class_pixels"]):
        assert n > 0 and abs(got - want) <= f["lim_sum"] / n
    # a class without a pixel has no mean
    only0 = torch.zeros_like(lab)
    crit(logp.detach(), only0, wgt)
    r0 = crit.read()
    assert r0["per_class_pixels"] == [B_ * H_ * W_, 0, 0] and math.isnan(r0["per_class_loss"][1]) and math.isnan(r0["per_class_loss"][2])
    # double backward raises
    (g,) = torch.autograd.grad(loss, logp, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward is not implemented"):
        g.sum().backward()
    crit.flush()
