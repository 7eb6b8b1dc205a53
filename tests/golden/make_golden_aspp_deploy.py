"""Deployment fixture of ASPP_ResNet: the reference's own eval forward on one whole-view tile.

Runs only where the reference checkout is present (same import recipe as make_golden.py, whose helpers are imported; nothing
of the reference is copied).  The reference's ASPP_ResNet(num_classes=3, in_channels=3, inplanes=16) with weights seed 44
runs in eval mode on synthetic.make_batch(1, 512, 832, 1000, planes=3), the tile of deploy/run_ubresnet_wholeview.py:38-39
with the three planes stacked as channels (BASELINE configs[3]).  Its running statistics are an INPUT: the calibrated
statistics committed in aspp_ip16_norm_1x3x64x96.npz (bn_keys, bn_stats), never recalibrated here.

        python tests/golden/make_golden_aspp_deploy.py             # aspp_ip16_norm_1x3x512x832_summary.npz
        python tests/golden/make_golden_aspp_deploy.py --f64       # the reference in float64, as *_f64.npz (not committed: no
                                                                   # test pins the oracle to this fixture)

Fields as in uresnet_ip16_nc4_norm_1x1x512x832_summary.npz: sample_idx, sample_logp_eval, argmax, argmax_sha256,
class_counts, margin_hist, packed safe_0p02 / safe_0p2 (top-2 margin above 0.02 / 0.2 nat), bn_keys, bn_stats, absmax, meta.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G          # noqa: E402  (import recipe, seeded inputs, sampling; its main() does not run on import)

H, W, SEED_X, SEED_W = 512, 832, 1000, 44
STATS = "aspp_ip16_norm_1x3x64x96.npz"


def main():
    torch.manual_seed(0)
    if G.F64:
        torch.set_default_dtype(torch.float64)
    _, aspp, _, _ = G.import_reference()
    sda = G.O.seeded_state_dict(G.O.aspp_resnet_schema(3, 3, 16), SEED_W)
    bn_keys = [k for k in sda if k.endswith("running_mean") or k.endswith("running_var")]
    m = aspp.ASPP_ResNet(num_classes=3, in_channels=3, inplanes=16, showsizes=False)
    m.load_state_dict(sda)
    assert os.path.exists(os.path.join(HERE, STATS)), "the committed statistics %s are an input of this fixture" % STATS
    G.keep_committed_stats(m, STATS, bn_keys)
    m.eval()
    after = m.state_dict()
    x = G.make_batch(1, H, W, SEED_X, planes=3)[0]
    with torch.no_grad():
        out = m.forward(torch.from_numpy(x))
    assert bool(torch.isfinite(out).all())
    stats = np.concatenate([after[k].numpy().reshape(-1) for k in bn_keys]).astype(np.float32)
    am = out.max(1)[1].numpy().astype(np.uint8)
    top2 = torch.topk(out, 2, dim=1)[0]
    margin = (top2[:, 0] - top2[:, 1]).numpy().reshape(-1)
    idx = G.sample_indices(out.numel(), 4096, 13)
    np.savez_compressed(
        G.out_path("aspp_ip16_norm_1x3x512x832_summary.npz"),
        sample_idx=idx, sample_logp_eval=out.numpy().reshape(-1)[idx],
        argmax=am, argmax_sha256=np.array(hashlib.sha256(am.tobytes()).hexdigest()),
        class_counts=np.bincount(am.reshape(-1), minlength=3),
        safe_0p02=np.packbits(margin > 0.02), safe_0p2=np.packbits(margin > 0.2),
        margin_hist=np.histogram(margin, bins=[0, 1e-4, 1e-3, 1e-2, 1e-1, 1, 10, 1e9])[0],
        bn_keys=np.array(bn_keys), bn_stats=stats, meta=np.array([1, 3, H, W, SEED_X, SEED_W]),
        absmax=np.float32(out.abs().max().item()))
    print("aspp deploy fixture: absmax logp %.3f" % out.abs().max().item(), "class counts", np.bincount(am.reshape(-1), minlength=3),
          "margin <= 0.2: %.4f, <= 0.02: %.4f" % (float((margin <= 0.2).mean()), float((margin <= 0.02).mean())))


if __name__ == "__main__":
    main()
