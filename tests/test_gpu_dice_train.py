"""PixelWiseDiceLoss and WeightedSumLoss (ubresnet_amd/training/pixelwise_diceloss.py over libubresnet_dice.so) on the device:

1. the module at 2 x 3 x 64 x 64 with class and pixel weights against the fp64 composite (tests/dice_ref.py) within its bound;
2. forward + backward captured with torch.cuda.graph and replayed on new inputs of the same shape: the bits of the eager calls;
3. WeightedSumLoss of NLL + Dice through one guarded FlatAdam step of the 2 x 1 x 64 x 64 UResNet: the loss is the sum of the
   parts, the gradients are finite, read() is consistent (TP + FN per class is the weighted pixel sum of the class);
4. one NaN pixel in the criterion's input makes the guard skip the step;
5. double backward raises;
6. epoch.train runs three batches with the combined criterion."""
import math

import numpy as np
import pytest
import torch

import dice_ref as R
import oracle.uresnet_oracle as O
from ubresnet_amd import synthetic

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training import PixelWiseDiceLoss, WeightedSumLoss, epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

B_, H_, W_ = 2, 64, 64


def _model():
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
    return m.cuda().train()


@pytest.fixture(scope="module")
def batch():
    return tuple(torch.from_numpy(a).cuda() for a in synthetic.make_batch(B_, H_, W_, 1000))


def _logp(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(3.0 * torch.randn(B_, 3, H_, W_, generator=g), dim=1).cuda()


def test_1_the_module_against_the_fp64_composite(batch):
    _, lab, _ = batch
    lab = lab.clone()
    lab[0, :4] = -100
    g = torch.Generator().manual_seed(5)
    wgt = (torch.rand(B_, H_, W_, generator=g) + 0.25).cuda()
    cw = torch.tensor([0.5, 2.0, 4.0])
    for alpha, beta, eps in ((0.5, 0.5, 1.0), (0.3, 0.7, 1e-6)):
        crit = PixelWiseDiceLoss(weight=cw, alpha=alpha, beta=beta, eps=eps)
        logp = _logp(11).requires_grad_(True)
        loss = crit(logp, lab, wgt)
        (2.0 * loss).backward()
        torch.cuda.synchronize()
        f = R.forward(logp.detach().cpu().numpy(), lab.cpu().numpy(), wgt.cpu().numpy(), cw.numpy(), -100, alpha, beta, eps, True)
        want, lim, ok = R.backward(2.0, f)
        hot = np.broadcast_to(ok[:, None], want.shape)
        got = logp.grad.cpu().numpy()
        ratio = float((np.abs(got.astype(np.float64) - want)[hot] / lim[hot]).max())
        print("alpha %g beta %g eps %g: worst gradient error / bound %.3f; loss %.9g (reference %.9g, bound %.3g)"
              % (alpha, beta, eps, ratio, float(loss.detach()), f["loss"], f["lim_loss"]))
        assert ratio <= 1.0 and not got.view(np.uint32)[~hot].any() and np.count_nonzero(got) > 0.9 * 3 * f["valid"]
        assert abs(float(loss) - f["loss"]) <= f["lim_loss"] and 0.0 < float(loss) < 1.0
        r = crit.read()
        assert r["valid"] == f["valid"] == B_ * H_ * W_ - 4 * W_ and r["pixels"] == f["pixels"] and r["loss"] == float(loss)
        for c in range(3):
            assert abs(r["tp"][c] - f["tp"][c]) <= f["d_tp"][c] and abs(r["fp"][c] - f["fp"][c]) <= f["d_fp"][c]
            assert abs(r["fn"][c] - f["fn"][c]) <= f["d_fn"][c] and abs(r["index"][c] - f["T"][c]) <= f["lim_T"][c]
            assert abs(r["soft_iou"][c] - f["tp"][c] / (f["tp"][c] + f["fp"][c] + f["fn"][c])) <= 1e-5
    crit.flush()


def test_2_a_captured_pair_replays_on_new_inputs(batch):
    _, lab, wgt = batch
    crit = PixelWiseDiceLoss(weight=torch.tensor([1.0, 2.0, 0.5]), alpha=0.3, beta=0.7).cuda()      # (class weights on the device: no copy in the capture)
    x, t, w = _logp(1).requires_grad_(True), lab.clone(), wgt.clone()
    for _ in range(2):                                             # warm up off the capture: the workspace and the library exist
        crit(x, t, w).backward()
        x.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = crit(x, t, w)
        (g,) = torch.autograd.grad(loss, x)
    for seed, roll in ((2, 3), (3, 17)):
        new_x, new_t = _logp(seed), torch.roll(lab, roll, dims=2)
        new_t[1, :2] = -100
        with torch.no_grad():
            x.copy_(new_x)
        t.copy_(new_t)
        w.copy_(torch.roll(wgt, roll, dims=1))
        graph.replay()
        torch.cuda.synchronize()
        eager_x = new_x.clone().requires_grad_(True)
        eager = PixelWiseDiceLoss(weight=torch.tensor([1.0, 2.0, 0.5]), alpha=0.3, beta=0.7).cuda()
        eager_loss = eager(eager_x, t.clone(), w.clone())
        eager_loss.backward()
        torch.cuda.synchronize()
        assert torch.equal(loss.view(torch.int32), eager_loss.detach().view(torch.int32)) and float(loss) > 0.0, seed
        assert torch.equal(g.view(torch.int32), eager_x.grad.view(torch.int32)) and bool(g.any()), seed
    crit.flush()


def _step(batch, poison=False):
    x, lab, wgt = batch
    m = _model()
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    nll, dice = PixelWiseNLLLoss(), PixelWiseDiceLoss()
    crit = WeightedSumLoss([(1.0, nll), (0.5, dice)])
    before = [p.detach().clone() for p in m.parameters()]
    logp = m.forward(x)
    if poison:
        # one NaN log-probability, in a channel that is not its pixel's target: the NLL part does not look at it, the region loss does
        mask = torch.zeros_like(logp)
        mask[1, (int(lab[1, 7, 9]) + 1) % 3, 7, 9] = float("nan")
        logp = logp + mask
    loss = crit.forward(logp, lab, wgt)
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return m, opt, crit, nll, dice, logp, loss, before


def test_3_nll_plus_dice_through_a_guarded_step(batch):
    x, lab, wgt = batch
    m, opt, crit, nll, dice, logp, loss, before = _step(batch)
    with torch.no_grad():
        parts = (float(nll(logp.detach(), lab, wgt)), float(dice(logp.detach(), lab, wgt)))
    want = np.float32(parts[0]) + np.float32(0.5) * np.float32(parts[1])
    assert abs(float(loss) - float(want)) <= 2.0 * float(np.spacing(np.float32(abs(want)))), (float(loss), parts)
    assert parts[0] > 0.0 and 0.0 < parts[1] < 1.0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert any(bool(p.grad.any()) for p in m.parameters())
    guard = opt.guard.read()
    assert guard["applied"] == 1 and guard["skipped"] == 0 and math.isfinite(guard["norm"]) and guard["norm"] > 0.0
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    (w_nll, r_nll), (w_dice, r) = crit.read()
    assert (w_nll, w_dice) == (1.0, 0.5) and r_nll is None and r["loss"] == parts[1]
    f = R.forward(logp.detach().cpu().numpy(), lab.cpu().numpy(), wgt.cpu().numpy(), None, -100)
    assert r["valid"] == B_ * H_ * W_ == sum(r["pixels"]) and r["pixels"] == f["pixels"]
    for c in range(3):
        # TP + FN of a class is the weighted pixel sum of the class: p + (1 - p) = 1 at every pixel, within the bound of the two sums
        assert abs(r["tp"][c] + r["fn"][c] - f["weighted_pixels"][c]) <= f["d_tp"][c] + f["d_fn"][c] + 2.0 ** -50 * f["weighted_pixels"][c], c
        assert 0.0 <= r["soft_iou"][c] <= r["index"][c] <= 1.0
    crit.flush()


def test_4_one_nan_input_pixel_makes_the_guard_skip(batch):
    m, opt, crit, nll, dice, logp, loss, before = _step(batch, poison=True)
    guard = opt.guard.read()
    x, lab, wgt = batch
    with torch.no_grad():
        assert math.isfinite(float(nll(logp.detach(), lab, wgt))) and math.isnan(float(dice(logp.detach(), lab, wgt)))
    assert not math.isfinite(float(loss)) and guard["applied"] == 0 and guard["skipped"] == 1
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    crit.flush()


def test_5_double_backward_raises(batch):
    _, lab, wgt = batch
    logp = _logp(4).requires_grad_(True)
    loss = PixelWiseDiceLoss()(logp, lab, wgt)
    (g,) = torch.autograd.grad(loss, logp, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward is not implemented"):
        g.sum().backward()
    PixelWiseDiceLoss.flush()


class _Feed(object):
    """a stager as far as the epoch loops look"""

    def __init__(self, items):
        self.items = list(items)

    def next(self):
        return self.items.pop(0)


def test_6_epoch_train_takes_the_combined_criterion():
    items = [tuple(torch.from_numpy(a).cuda() for a in synthetic.make_batch(B_, H_, W_, seed)) for seed in (1000, 2000, 3000)]
    m = _model()
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    dice = PixelWiseDiceLoss(alpha=0.3, beta=0.7)
    crit = WeightedSumLoss([(1.0, PixelWiseNLLLoss()), (0.5, dice)])
    lines = []
    loss, acc = epoch.train(_Feed(items), m, crit, opt, 3, print_freq=1, log=lines.append)
    assert math.isfinite(loss) and loss > 0.0 and math.isfinite(acc)
    assert opt.guard.read()["applied"] == 3 and all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert any(l.startswith("Train Iter") for l in lines)
    r = dice.read()
    assert r["valid"] == B_ * H_ * W_ and 0.0 < r["loss"] < 1.0 and sum(r["pixels"]) == r["valid"]
