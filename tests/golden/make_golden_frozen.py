#!/usr/bin/env python
"""Frozen-BatchNorm fixture, made by the REFERENCE's own model code (same recipe and helpers as make_golden.py).

uresnet_ip16_frozen_2x1x64x64.npz: the reference UResNet(3 classes, 1 plane, inplanes 16) on the seeded weights of the
train fixture, its running statistics calibrated by its own train-mode passes (calibrate_running_stats), then ONE
``model.eval()`` forward + PixelWiseNLLLoss + backward: eval-mode log-probabilities, the loss, and per parameter tensor the
gradient's L2 norm and 16 sampled entries.  The calibrated statistics (bn_keys / bn_stats) are part of the fixture's
input.  Needs the reference checkout; nothing of its text is stored.

    python tests/golden/make_golden_frozen.py
    python tests/golden/make_golden_frozen.py --f64      # the same in float64 (same statistics), as *_f64.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG                      # noqa: E402
from make_golden import O                      # noqa: E402

B, C, H, W, SEED_X, SEED_W, SEED_CAL = 2, 1, 64, 64, 1000, 42, 1700


def main():
    if MG.F64:
        torch.set_default_dtype(torch.float64)     # the reference's modules are built in float64 (make_golden.py --f64)
    ub, _, pl, _ = MG.import_reference()
    sd = O.seeded_state_dict(O.uresnet_schema(3, C, 16, 16), SEED_W)
    if MG.F64:
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    bn_keys = [k for k in sd if k.endswith("running_mean") or k.endswith("running_var")]
    m = MG.make_differentiable(ub.UResNet(num_classes=3, input_channels=C, inplanes=16))
    m.load_state_dict(sd)
    MG.calibrate_running_stats(m, [MG.make_batch(B, H, W, SEED_CAL + 10 * i)[0] for i in range(2)])
    MG.keep_committed_stats(m, "uresnet_ip16_frozen_2x1x64x64.npz", bn_keys)
    stats = np.concatenate([m.state_dict()[k].numpy().reshape(-1) for k in bn_keys]).astype(np.float32)
    x, lab, wgt = MG.make_batch(B, H, W, SEED_X)
    crit = pl.PixelWiseNLLLoss()
    crit.size_average = True   # the version shim of make_golden.py
    m.eval()
    m.zero_grad()
    out = m.forward(torch.from_numpy(x))
    loss = crit.forward(out, torch.from_numpy(lab), torch.from_numpy(wgt))
    loss.backward()
    after = np.concatenate([m.state_dict()[k].numpy().reshape(-1) for k in bn_keys]).astype(np.float32)
    assert np.array_equal(after, stats), "eval-mode pass touched the running statistics"
    names, norms, samples = MG.grad_summary(m)
    np.savez_compressed(
        MG.out_path("uresnet_ip16_frozen_2x1x64x64.npz"),
        meta=np.array([B, C, H, W, SEED_X, SEED_W]), bn_keys=np.array(bn_keys), bn_stats=stats,
        logp_eval=out.detach().numpy().astype(MG.FDT), loss=np.float64(loss.item()),
        grad_names=np.array(names), grad_norms=norms, **{"gs__" + k: v for k, v in samples.items()})
    print("frozen fixture: loss %.6f, absmax logp %.3f, |g conv1.bias| %.3e, |g conv10.bias| %.3e"
          % (loss.item(), out.abs().max().item(), norms[names.index("conv1.bias")], norms[names.index("conv10.bias")]))


if __name__ == "__main__":
    main()
