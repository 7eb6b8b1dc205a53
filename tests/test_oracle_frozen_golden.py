"""Pin the CPU oracle's EVAL-mode (frozen BatchNorm) forward and gradients to the reference's own code.

Fixture: tests/golden/uresnet_ip16_frozen_2x1x64x64_f64.npz, written by tests/golden/make_golden_frozen.py: the reference
UResNet in float64 on seeded weights and calibrated running statistics, one ``model.eval()`` forward + PixelWiseNLLLoss +
backward.  Bounds as in test_oracle_golden.py for the train fixture: loss 1e-6 relative, per-tensor gradient norms and sampled
entries 1e-5.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from oracle import uresnet_oracle as O
from ubresnet_amd import synthetic

torch.set_num_threads(min(8, os.cpu_count() or 1))


def test_uresnet_eval_mode_forward_and_grads(golden_dir):
    g = np.load(os.path.join(golden_dir, "uresnet_ip16_frozen_2x1x64x64_f64.npz"), allow_pickle=False)
    g32 = np.load(os.path.join(golden_dir, "uresnet_ip16_frozen_2x1x64x64.npz"), allow_pickle=False)
    assert np.array_equal(g["bn_stats"], g32["bn_stats"]) and [str(k) for k in g["bn_keys"]] == [str(k) for k in g32["bn_keys"]]
    B, C, H, W, seed0, wseed = [int(v) for v in g["meta"]]
    sd = O.state_dict_with_bn_stats(O.seeded_state_dict(O.uresnet_schema(3, C, 16, 16), wseed), g["bn_keys"], g["bn_stats"])
    p = OrderedDict((k, (v.double().requires_grad_(True) if O.is_param_key(k) else (v.double() if v.is_floating_point() else v)))
                    for k, v in sd.items())
    x, lab, wgt = synthetic.make_batch(B, H, W, seed0)
    logp = O.uresnet_forward(p, torch.from_numpy(x).double(), False, None)
    loss = O.pixelwise_nll(logp, torch.from_numpy(lab), torch.from_numpy(wgt).double())
    names = [k for k in p if O.is_param_key(k)]
    grads = OrderedDict(zip(names, torch.autograd.grad(loss, [p[k] for k in names])))
    assert np.abs(logp.detach().numpy() - g["logp_eval"]).max() <= 1e-6 * max(1.0, np.abs(g["logp_eval"]).max())
    assert np.abs(g["logp_eval"]).max() < 100.0          # the statistics normalise (seeded ones give 1e5)
    assert abs(float(loss) - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    assert [str(n) for n in g["grad_names"]] == names
    for n, ref_norm in zip(names, g["grad_norms"]):
        gv = grads[n].reshape(-1).numpy()
        norm = np.sqrt((gv.astype(np.float64) ** 2).sum())
        assert abs(norm - ref_norm) <= 1e-5 * ref_norm + 1e-7, n
        rs = np.random.RandomState(7)
        idx = np.sort(rs.choice(gv.shape[0], size=min(16, gv.shape[0]), replace=False))
        assert np.abs(gv[idx] - g["gs__" + n]).max() <= 1e-5 * (np.abs(gv).max() + 1e-12) + 1e-7, n
    # in front of a frozen BatchNorm these biases get real gradients (in front of a train-mode one they are analytically zero)
    for b in ("conv1", "conv10"):
        assert float(grads[b + ".bias"].norm()) > 1e-3 * float(grads[b + ".weight"].norm()), b
