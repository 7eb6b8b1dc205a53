"""Pin the CPU oracle (oracle/uresnet_oracle.py) to fixtures produced by the reference's own code.

Fixtures: tests/golden/*.npz, written by tests/golden/make_golden.py from an in-memory import
of /root/reference.  Tolerances: forward <= 1e-6 abs on log-probs
(both sides are PyTorch-CPU; the only difference is op dispatch order), gradients
<= 1e-5 relative on per-tensor L2 norms and sampled entries.  Everything is compared in
float64 (tests/golden/*_f64.npz, the reference's code run in float64, against the oracle in
float64): in fp32 the same code differs from CPU to CPU by ~1e-6 relative (convolution kernels
sum in another order), which is the size of these bounds; in float64 by ~1e-14.
"""
import hashlib
from collections import OrderedDict
import os

import numpy as np
import pytest
import torch

from oracle import uresnet_oracle as O
from ubresnet_amd import synthetic

torch.set_num_threads(min(8, os.cpu_count() or 1))


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _f64(sd):
    return OrderedDict((k, v.double() if v.is_floating_point() else v) for k, v in sd.items())


def _batch64(*args, **kw):
    x, lab, wgt = synthetic.make_batch(*args, **kw)
    return torch.from_numpy(x).double(), torch.from_numpy(lab), torch.from_numpy(wgt).double()


def test_schema_matches_reference_keys(golden_dir):
    for fn, schema in (("state_dict_keys_uresnet_ip16.txt", O.uresnet_schema(3, 1, 16, 16)),
                       ("state_dict_keys_aspp_ip16.txt", O.aspp_resnet_schema(3, 3, 16))):
        lines = open(os.path.join(golden_dir, fn)).read().split("\n")[:-1]
        keys = [l.split(" ")[0] for l in lines]
        assert keys == list(schema.keys())
    sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
    nparam = sum(v.numel() for k, v in sd.items() if O.is_param_key(k))
    assert nparam == 18100931
    assert sum(1 for k in sd if O.is_param_key(k)) == 165
    sda = O.seeded_state_dict(O.aspp_resnet_schema(3, 3, 16), 44)
    assert sum(v.numel() for k, v in sda.items() if O.is_param_key(k)) == 31577251


@pytest.mark.parametrize("tag", ["2x1x64x64", "1x1x96x128"])
def test_uresnet_forward_and_grads(golden_dir, tag):
    g = _load(golden_dir, "uresnet_ip16_%s_f64.npz" % tag)
    B, C, H, W, seed0, wseed = [int(v) for v in g["meta"]]
    sd = _f64(O.seeded_state_dict(O.uresnet_schema(3, C, 16, 16), wseed))
    xt, lt, wt = _batch64(B, H, W, seed0)
    with torch.no_grad():
        ev = O.uresnet_forward(sd, xt, train=False)
    assert np.abs(ev.numpy() - g["logp_eval"]).max() <= 1e-6 * max(1.0, np.abs(g["logp_eval"]).max())
    loss, grads, logp, ns = O.train_step_grads(O.uresnet_forward, sd, xt, lt, wt)
    assert np.abs(logp.numpy() - g["logp_train"]).max() <= 2e-6 * max(1.0, np.abs(g["logp_train"]).max())
    assert abs(float(loss) - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    names = [str(n) for n in g["grad_names"]]
    assert names == list(grads.keys())
    for n, ref_norm in zip(names, g["grad_norms"]):
        gv = grads[n].reshape(-1).numpy()
        norm = np.sqrt((gv.astype(np.float64) ** 2).sum())
        assert abs(norm - ref_norm) <= 1e-5 * ref_norm + 1e-7, n
        rs = np.random.RandomState(7)
        idx = np.sort(rs.choice(gv.shape[0], size=min(16, gv.shape[0]), replace=False))
        assert np.abs(gv[idx] - g["gs__" + n]).max() <= 1e-5 * (np.abs(gv).max() + 1e-12) + 1e-7, n
    for k in ("bn1", "bn10"):
        assert np.abs(ns[k + ".running_mean"].numpy() - g[k + "_running_mean"]).max() <= 1e-6
        assert np.abs(ns[k + ".running_var"].numpy() - g[k + "_running_var"]).max() <= 1e-5
    assert int(ns["bn1.num_batches_tracked"]) == int(g["nbt"])


def test_uresnet_four_classes_eval(golden_dir):
    g = _load(golden_dir, "uresnet_ip16_nc4_1x1x64x96_f64.npz")
    B, C, H, W, seed0, wseed = [int(v) for v in g["meta"]]
    sd = _f64(O.seeded_state_dict(O.uresnet_schema(4, C, 16, 16), wseed))
    x = _batch64(B, H, W, seed0)[0]
    with torch.no_grad():
        ev = O.uresnet_forward(sd, x, train=False)
    assert np.abs(ev.numpy() - g["logp_eval"]).max() <= 1e-6 * max(1.0, np.abs(g["logp_eval"]).max())


def test_aspp_forward_and_grads(golden_dir):
    g = _load(golden_dir, "aspp_ip16_1x3x64x96_f64.npz")
    B, C, H, W, seed0, wseed = [int(v) for v in g["meta"]]
    sd = _f64(O.seeded_state_dict(O.aspp_resnet_schema(3, C, 16), wseed))
    xt, lt, wt = _batch64(B, H, W, seed0, planes=C)
    with torch.no_grad():
        ev = O.aspp_resnet_forward(sd, xt, train=False)
    assert np.abs(ev.numpy() - g["logp_eval"]).max() <= 1e-6 * max(1.0, np.abs(g["logp_eval"]).max())
    loss, grads, logp, _ = O.train_step_grads(O.aspp_resnet_forward, sd, xt, lt, wt)
    assert abs(float(loss) - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    for n, ref_norm in zip([str(n) for n in g["grad_names"]], g["grad_norms"]):
        gv = grads[n].reshape(-1).numpy().astype(np.float64)
        assert abs(np.sqrt((gv ** 2).sum()) - ref_norm) <= 2e-5 * ref_norm + 1e-7, n


def test_blocks_and_loss(golden_dir):
    g = _load(golden_dir, "blocks_f64.npz")
    for name, (cin, cout, stride) in {"id": (8, 8, 1), "proj": (8, 16, 1), "down": (8, 16, 2)}.items():
        sd = _f64(O.seeded_state_dict(O._block_keys("b", cin, cout, stride), 50 + stride + cout))
        x = torch.from_numpy(g["block_%s_x" % name]).double()
        with torch.no_grad():
            tr = O.basic_block(sd, "b", x, stride, True, None)
            ev = O.basic_block(sd, "b", x, stride, False, None)
        assert np.abs(tr.numpy() - g["block_%s_train" % name]).max() <= 2e-6
        assert np.abs(ev.numpy() - g["block_%s_eval" % name]).max() <= 2e-6
    sd = _f64(O.seeded_state_dict(OrderedDict([("d.deconv.weight", (16, 8, 4, 4))] + list(O._double_keys("d.res", 16, 8, 1).items())), 60))
    with torch.no_grad():
        ev = O.conv_transpose_layer(sd, "d", torch.from_numpy(g["ctl_x"]).double(), torch.from_numpy(g["ctl_skip"]).double(), False, None)
        tr = O.conv_transpose_layer(sd, "d", torch.from_numpy(g["ctl_x"]).double(), torch.from_numpy(g["ctl_skip"]).double(), True, None)
    assert np.abs(ev.numpy() - g["ctl_eval"]).max() <= 2e-6
    assert np.abs(tr.numpy() - g["ctl_train"]).max() <= 2e-6
    loss = O.pixelwise_nll(torch.from_numpy(g["loss_logp"]), torch.from_numpy(g["loss_target"]), torch.from_numpy(g["loss_pw"]))
    assert abs(float(loss) - float(g["loss_value"])) <= 1e-6 * abs(float(g["loss_value"]))
    # closed form: mean(-logp[target]*w), ignored pixels contribute 0 but stay in the denominator
    lp, tg, pw = g["loss_logp"], g["loss_target"], g["loss_pw"]
    acc = 0.0
    for b in range(lp.shape[0]):
        for i in range(lp.shape[2]):
            for j in range(lp.shape[3]):
                if tg[b, i, j] != -100:
                    acc += -float(lp[b, tg[b, i, j], i, j]) * float(pw[b, i, j])
    assert abs(acc / tg.size - float(g["loss_value"])) <= 1e-5 * abs(float(g["loss_value"]))


def test_uresnet_512_summary(golden_dir):
    """BASELINE config-1 shape (B=2, 512x512): sampled log-probs, argmax hash off low-margin pixels."""
    g = _load(golden_dir, "uresnet_ip16_2x1x512x512_summary_f64.npz")
    B, C, H, W, seed0, wseed = [int(v) for v in g["meta"]]
    sd = _f64(O.seeded_state_dict(O.uresnet_schema(3, C, 16, 16), wseed))
    x = _batch64(B, H, W, seed0)[0]
    with torch.no_grad():
        ev = O.uresnet_forward(sd, x, train=False)
    flat = ev.numpy().reshape(-1)
    ref = g["sample_logp_eval"]
    assert np.abs(flat[g["sample_idx"]] - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max())
    am = ev.max(1)[1].numpy().astype(np.uint8)
    if len(g["low_margin_idx"]) == 0:
        assert hashlib.sha256(am.tobytes()).hexdigest() == str(g["argmax_sha256_eval"])
    assert np.abs(np.bincount(am.reshape(-1), minlength=3) - g["class_counts_eval"]).sum() <= 2 * len(g["low_margin_idx"])


def test_accuracy_and_confusion():
    rs = np.random.RandomState(3)
    out = torch.from_numpy(rs.standard_normal((2, 3, 8, 8)).astype(np.float32))
    tgt = torch.from_numpy(rs.randint(0, 3, (2, 8, 8)).astype(np.int64))
    acc = O.accuracy(out, tgt)
    cm = O.confusion_matrix(out, tgt)
    for c in range(3):
        n = cm[c].sum().item()
        assert abs(acc[c] - (100.0 * cm[c, c].item() / n if n else 0.0)) < 1e-9
    assert abs(acc[3] - 100.0 * cm.diag().sum().item() / cm.sum().item()) < 1e-9


@pytest.mark.parametrize("tag", ["1x1x64x96", "1x1x512x832_summary"])
def test_uresnet_nc4_normalised_eval(golden_dir, tag):
    """deployment-shaped fixtures: 4 classes (deploy/ubresnet_funcs.py:43), running statistics calibrated by the
    reference itself so that eval activations are O(1) (the fp16 inference parity tests build on these)"""
    g = _load(golden_dir, "uresnet_ip16_nc4_norm_%s_f64.npz" % tag)
    B, C, H, W, seed0, wseed = [int(v) for v in g["meta"]]
    sd = _f64(O.state_dict_with_bn_stats(O.seeded_state_dict(O.uresnet_schema(4, C, 16, 16), wseed), g["bn_keys"], g["bn_stats"]))
    x = _batch64(B, H, W, seed0)[0]
    with torch.no_grad():
        out = O.uresnet_forward(sd, x, train=False).numpy()
    assert float(np.abs(out).max()) < 100.0            # normalised: nowhere near the 1e5 of uncalibrated seeded statistics
    if "logp_eval" in g.files:
        assert np.abs(out - g["logp_eval"]).max() <= 2e-5
    else:
        assert np.abs(out.reshape(-1)[g["sample_idx"]] - g["sample_logp_eval"]).max() <= 1e-4
        am = out.argmax(1).astype(np.uint8)
        safe = np.unpackbits(g["safe_0p02"])[:am.size].astype(bool)
        assert np.array_equal(am.reshape(-1)[safe], g["argmax"].reshape(-1)[safe])
        if int(g["margin_hist"][:2].sum()) == 0:       # no pixel with a top-2 margin below 1e-3: the class map is pinned bit for bit
            assert hashlib.sha256(am.tobytes()).hexdigest() == str(g["argmax_sha256"])


def test_aspp_normalised_eval_and_ip32(golden_dir):
    """round-3 fixtures: the reference ASPP_ResNet in eval mode on reference-calibrated running statistics, and one train
    step of the inplanes=32 U-ResNet that training/train_ubresnet2018_wlarcv2.py:88 builds"""
    g = _load(golden_dir, "aspp_ip16_norm_1x3x64x96_f64.npz")
    B, C, H, W, seed0, wseed = [int(v) for v in g["meta"]]
    sd = _f64(O.state_dict_with_bn_stats(O.seeded_state_dict(O.aspp_resnet_schema(3, C, 16), wseed), g["bn_keys"], g["bn_stats"]))
    x = _batch64(B, H, W, seed0, planes=C)[0]
    with torch.no_grad():
        ev = O.aspp_resnet_forward(sd, x, train=False)
    assert np.abs(ev.numpy() - g["logp_eval"]).max() <= 2e-5          # log-probabilities are O(10) here
    g = _load(golden_dir, "uresnet_ip32_1x1x64x64_f64.npz")
    B, C, H, W, seed0, wseed = [int(v) for v in g["meta"]]
    sd = _f64(O.seeded_state_dict(O.uresnet_schema(3, C, 32, 16), wseed))
    xt, lt, wt = _batch64(B, H, W, seed0)
    with torch.no_grad():
        ev = O.uresnet_forward(sd, xt, train=False)
    assert np.abs(ev.numpy() - g["logp_eval"]).max() <= 1e-6 * max(1.0, np.abs(g["logp_eval"]).max())
    loss, grads, logp, _ = O.train_step_grads(O.uresnet_forward, sd, xt, lt, wt)
    assert np.abs(logp.numpy() - g["logp_train"]).max() <= 2e-6 * max(1.0, np.abs(g["logp_train"]).max())
    assert abs(float(loss) - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    for n, ref_norm in zip([str(n) for n in g["grad_names"]], g["grad_norms"]):
        gv = grads[n].reshape(-1).numpy().astype(np.float64)
        assert abs(np.sqrt((gv ** 2).sum()) - ref_norm) <= 2e-5 * ref_norm + 1e-7, n


def test_aspp_full_size_summary(golden_dir):
    """BASELINE configs[3] at its real size (1 x 3 x 512 x 832): the oracle against what the reference's own ASPP_ResNet produced"""
    g = _load(golden_dir, "aspp_ip16_1x3x512x832_summary_f64.npz")
    B, C, H, W, seed0, wseed = [int(v) for v in g["meta"]]
    sd = _f64(O.seeded_state_dict(O.aspp_resnet_schema(3, C, 16), wseed))
    xt, lt, wt = _batch64(B, H, W, seed0, planes=C)
    idx = g["sample_idx"]
    with torch.no_grad():
        ev = O.aspp_resnet_forward(sd, xt, train=False).numpy()
    ref = g["sample_logp_eval"]
    assert np.abs(ev.reshape(-1)[idx] - ref).max() <= 1e-5 * float(g["absmax_eval"])
    am = ev.argmax(1).astype(np.uint8)
    assert np.abs(np.bincount(am.reshape(-1), minlength=3) - g["class_counts_eval"]).sum() <= 2 * len(g["low_margin_idx_eval"]) + 2
    loss, grads, logp, _ = O.train_step_grads(O.aspp_resnet_forward, sd, xt, lt, wt)
    assert np.abs(logp.numpy().reshape(-1)[idx] - g["sample_logp_train"]).max() <= 2e-5 * max(1.0, float(g["absmax_train"]))
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    for n, ref_norm in zip([str(n) for n in g["grad_names"]], g["grad_norms"]):
        gv = grads[n].reshape(-1).numpy().astype(np.float64)
        assert abs(np.sqrt((gv ** 2).sum()) - ref_norm) <= 1e-3 * ref_norm + 1e-7, n
