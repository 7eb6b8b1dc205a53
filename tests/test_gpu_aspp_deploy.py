"""ASPP_ResNet deployment (GPU): the folded inference schedule (Engine.aspp_infer: BatchNorm folded into the packed weights,
ReLU / shortcut in the conv epilogues, one ubr_aspp_front launch per ASPP level) against the reference's own eval forward,
deploy.load_model(arch="aspp"), segment_crops, and the whole-view segmenter on stacked tiles (the three planes as channels):
crop / stitch bit-exact against torch slicing, hipGraph replay bit-exact against eager launches."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import uresnet_oracle as O
from ubresnet_amd import synthetic

if torch.cuda.is_available():
    from ubresnet_amd import deploy, engine, ops

SMALL = "aspp_ip16_norm_1x3x64x96.npz"
FULL = "aspp_ip16_norm_1x3x512x832_summary.npz"

# f16, 512 x 832, absolute bar on the sampled log-probabilities (|logp| up to 32.7): twice the largest sample error of the
# PARENT schedule (eval forward on the training schedule, UBR_INFER_FOLD=0: BatchNorm applied on load, nothing folded)
# against this fixture, measured on an MI355X: 0.160473 (fp32 on the same schedule: 1.24e-4).  That is already above the 0.1 the
# 64 x 96 fixture is held to: the bar at this size is 0.320946, and the class-map thresholds stay where they are.  Folding the
# scale into f16 weights adds one rounding per weight; the factor two covers it (the folded schedule measured 0.1031).
F16_FULL_PARENT_ERR = 0.160473
F16_FULL_BAR = 2 * F16_FULL_PARENT_ERR


def _state(g):
    B, C, H, W, seed0, wseed = [int(v) for v in g["meta"]]
    sd = O.state_dict_with_bn_stats(O.seeded_state_dict(O.aspp_resnet_schema(3, C, 16), wseed), g["bn_keys"], g["bn_stats"])
    x = torch.from_numpy(synthetic.make_batch(B, H, W, seed0, planes=C)[0]).cuda()
    return sd, x


def _model(g):
    sd, x = _state(g)
    return deploy.load_model(None, "cuda:0", num_classes=3, input_channels=3, state_dict=sd, arch="aspp"), x


def _forward(m, x, dt=None):
    m.compute_dtype = dt
    try:
        with torch.no_grad():
            return m(x)
    finally:
        m.compute_dtype = None


def _class_map_bars(am, g, ncls=3):
    """f16 bars of test_full_size_tile_matches_reference_summary on the pixels whose reference top-2 margin exceeds 0.2 nat"""
    ram = g["argmax"].reshape(-1)
    am = am.reshape(-1)
    safe = np.unpackbits(g["safe_0p2"])[:am.size].astype(bool)
    left_out = 1.0 - float(safe.mean())
    print("safe_0p2 leaves out %.4f of the pixels" % left_out)
    assert left_out <= 0.12
    agree = float((am[safe] == ram[safe]).mean())
    cm = np.bincount(ram[safe].astype(np.int64) * ncls + am[safe], minlength=ncls * ncls).reshape(ncls, ncls)
    iou = [cm[c, c] / max(1, cm[c].sum() + cm[:, c].sum() - cm[c, c]) for c in range(ncls)]
    print("agreement on safe_0p2 %.5f, IoU %s, agreement everywhere %.5f" % (agree, iou, float((am == ram).mean())))
    assert agree >= 0.9995
    assert min(iou) >= 0.99


# ----------------------------------------------------------------------------------------------------------------------
# schedule against the reference
# ----------------------------------------------------------------------------------------------------------------------
def test_folded_schedule_runs_and_matches_reference_fp32(golden_dir):
    g = np.load(os.path.join(golden_dir, SMALL))
    m, x = _model(g)
    calls = []
    orig = ops.aspp_front
    ops.aspp_front = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        out = _forward(m, x).cpu()
    finally:
        ops.aspp_front = orig
    assert len(calls) == 3, "eval under no_grad must take the folded schedule: one ubr_aspp_front per ASPP level"
    ref = torch.from_numpy(g["logp_eval"])
    d = (out - ref).abs()
    print("aspp folded fp32 64x96: max abs err %.3e, worst |a-b| - 1e-3|b| %.3e" % (float(d.max()), float((d - 1e-3 * ref.abs()).max())))
    assert bool((d <= 1e-3 * ref.abs() + 1e-4).all())
    assert float(torch.logsumexp(out, 1).abs().max()) <= 1e-3          # rows are log-probabilities


def test_folded_equals_training_schedule_in_eval_mode_fp32(golden_dir, monkeypatch):
    g = np.load(os.path.join(golden_dir, SMALL))
    m, x = _model(g)
    folded = _forward(m, x)
    monkeypatch.setattr(engine, "_INFER_FOLD", False)
    m.__dict__.pop("_ubr_engine", None)
    plain = _forward(m, x)
    d = float((folded - plain).abs().max())
    print("aspp folded vs UBR_INFER_FOLD=0, fp32: max abs difference %.3e" % d)
    assert d <= 2e-4


@pytest.mark.parametrize("dt,tol", [(torch.float16, 0.1), (torch.bfloat16, 1.0)], ids=["f16", "bf16"])
def test_folded_schedule_low_precision(golden_dir, dt, tol):
    g = np.load(os.path.join(golden_dir, SMALL))
    m, x = _model(g)
    out = _forward(m, x, dt).cpu()
    ref = torch.from_numpy(g["logp_eval"])
    err = float((out - ref).abs().max())
    print("aspp folded %s 64x96: max abs err %.4f" % (dt, err))
    assert err <= tol
    top2 = torch.topk(ref, 2, dim=1)[0]
    safe = (top2[:, 0] - top2[:, 1]) > 2 * tol
    assert torch.equal(out.argmax(1)[safe], ref.argmax(1)[safe])


def test_train_mode_and_grad_enabled_stay_on_the_training_schedule(golden_dir, monkeypatch):
    g = np.load(os.path.join(golden_dir, SMALL))
    m, x = _model(g)
    calls = []
    orig = ops.aspp_front
    monkeypatch.setattr(ops, "aspp_front", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    m(x)                                          # eval mode, gradients enabled
    assert not calls
    m.ASPP_layer_enc4.B3_bn.train()               # one BatchNorm in train mode
    with torch.no_grad():
        m(x)
    assert not calls
    m.eval()
    with torch.no_grad():
        m(x)
    assert len(calls) == 3


def test_full_size_fp32_matches_reference_summary(golden_dir):
    g = np.load(os.path.join(golden_dir, FULL))
    m, x = _model(g)
    out = _forward(m, x).cpu().numpy()
    ref = g["sample_logp_eval"]
    d = np.abs(out.reshape(-1)[g["sample_idx"]] - ref)
    print("aspp folded fp32 512x832: sample max abs err %.3e (|logp| max %.2f)" % (float(d.max()), float(np.abs(ref).max())))
    assert bool((d <= 1e-3 * np.abs(ref) + 1e-4).all())
    am = out.argmax(1).astype(np.uint8).reshape(-1)
    ram = g["argmax"].reshape(-1)
    safe = np.unpackbits(g["safe_0p02"])[:am.size].astype(bool)
    assert np.array_equal(am[safe], ram[safe])
    if int(g["margin_hist"][:2].sum()) == 0:
        assert hashlib.sha256(am.tobytes()).hexdigest() == str(g["argmax_sha256"])


def test_full_size_f16_matches_reference_summary(golden_dir):
    g = np.load(os.path.join(golden_dir, FULL))
    m, x = _model(g)
    out = _forward(m, x, torch.float16).cpu().numpy()
    ref = g["sample_logp_eval"]
    err = float(np.abs(out.reshape(-1)[g["sample_idx"]] - ref).max())
    print("aspp folded f16 512x832: sample max abs err %.4f (bar %.4f = 2 x parent schedule %.4f)" % (err, F16_FULL_BAR, F16_FULL_PARENT_ERR))
    _class_map_bars(out.argmax(1).astype(np.uint8), g)
    assert err <= F16_FULL_BAR


# ----------------------------------------------------------------------------------------------------------------------
# deployment surface
# ----------------------------------------------------------------------------------------------------------------------
def test_load_model_aspp_and_segment_crops(golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, SMALL))
    sd, x = _state(g)
    # a checkpoint as the reference writes it from a DataParallel model (training/train_ubresnet2018_wlarcv2.py:260-266)
    ck = {"iter": 7, "epoch": 0, "state_dict": {"module." + k: v for k, v in sd.items()}, "best_prec1": 0.0, "optimizer": {}}
    path = deploy.save_checkpoint(ck, False, -1, str(tmp_path / "checkpoint.pth.tar"))
    m = deploy.load_model(path, "cuda:0", num_classes=3, input_channels=3, arch="aspp")
    from ubresnet_amd.models.ASPP_ResNet import ASPP_ResNet
    assert isinstance(m, ASPP_ResNet) and not m.training
    out = deploy.segment_crops(m, torch.cat([x, x, x], 0), batch=2).cpu()
    ref = torch.from_numpy(g["logp_eval"])
    assert out.shape == (3,) + tuple(ref.shape[1:])
    for i in range(3):
        d = (out[i:i + 1] - ref).abs()
        assert bool((d <= 1e-3 * ref.abs() + 1e-4).all())


def test_segmenter_refuses_other_channel_counts(golden_dir):
    g = np.load(os.path.join(golden_dir, SMALL))
    m, _ = _model(g)
    with pytest.raises(ValueError):
        deploy.WholeViewSegmenter(m, 100, 200, planes=2, tile=(64, 96), batch=2)
    with pytest.raises(ValueError):
        deploy.WholeViewSegmenter(m, 100, 200, planes=3, tile=(64, 96), batch=22)     # 66 crop descriptors > UBR_MAX_TILES


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_stacked_whole_view_tiling(golden_dir, dtype):
    g = np.load(os.path.join(golden_dir, SMALL))
    m, _ = _model(g)
    P, rows, cols, th, tw = 3, 100, 200, 64, 96
    view = torch.zeros((P, 1, rows, cols), device="cuda")
    for p in range(P):
        view[p, 0] = torch.from_numpy(synthetic.make_crop(rows, cols, 7000 + p)[0]).cuda()
    seg = deploy.WholeViewSegmenter(m, rows, cols, planes=P, tile=(th, tw), batch=4, dtype=dtype, use_graph=True)
    assert seg.stacked and seg.tiles_per_event == 6
    out = seg(view)
    assert out.shape == (3, rows, cols) and torch.isfinite(out).all()
    assert torch.equal(out, seg(view))                    # graph replay is repeatable
    eager = deploy.WholeViewSegmenter(m, rows, cols, planes=P, tile=(th, tw), batch=4, dtype=dtype, use_graph=False)
    assert torch.equal(out, eager(view)), "hipGraph replay differs from eager launches"
    # restatement in torch: crop every stacked tile by slicing, run the model, copy the keep window
    want = torch.full_like(out, float("nan"))
    for (p, r0, c0, kr0, kr1, kc0, kc1) in seg.tiles:
        assert p == 0
        crop = torch.zeros((1, P, th, tw), device="cuda")
        hh, ww = min(th, rows - r0), min(tw, cols - c0)
        crop[0, :, :hh, :ww] = view[:, 0, r0:r0 + hh, c0:c0 + ww]
        sc = _forward(m, crop, dtype)[0]
        y1, x1 = min(kr1, rows - r0), min(kc1, cols - c0)
        want[:, r0 + kr0:r0 + y1, c0 + kc0:c0 + x1] = sc[:, kr0:y1, kc0:x1]
    assert not torch.isnan(want).any(), "keep windows must partition the view"
    assert torch.equal(out, want)


def test_stacked_segmenter_recaptures_on_replaced_storage(golden_dir):
    g = np.load(os.path.join(golden_dir, SMALL))
    m, _ = _model(g)
    P, rows, cols, th, tw = 3, 64, 96, 64, 96
    view = torch.zeros((P, 1, rows, cols), device="cuda")
    for p in range(P):
        view[p, 0] = torch.from_numpy(synthetic.make_crop(rows, cols, 7100 + p)[0]).cuda()
    seg = deploy.WholeViewSegmenter(m, rows, cols, planes=P, tile=(th, tw), batch=1, dtype=torch.float32, use_graph=True)
    a = seg(view)
    for p_ in m.parameters():                 # every parameter moves to new storage with the same values
        p_.data = p_.data.clone()
    b = seg(view)
    assert torch.equal(a, b)


def test_stacked_whole_view_full_size_event(golden_dir):
    """a 3 x 1008 x 3456 event with the planes stacked as channels: 10 tiles of 3 x 512 x 832, f16, one hipGraph replay"""
    g = np.load(os.path.join(golden_dir, FULL))
    m, x = _model(g)
    P, rows, cols, th, tw = 3, 1008, 3456, 512, 832
    view = torch.zeros((P, 1, rows, cols), device="cuda")
    for p in range(P):
        view[p, 0] = torch.from_numpy(synthetic.make_crop(rows, cols, 5000 + p)[0]).cuda()
    view[:, 0, :th, :tw] = x[0]                           # the tile at (0, 0) is the fixture's input
    seg = deploy.WholeViewSegmenter(m, rows, cols, planes=P, tile=(th, tw), batch=10, dtype=torch.float16, use_graph=True)
    assert seg.tiles_per_event == 10
    cover = torch.zeros((rows, cols), dtype=torch.int32)
    for (p, r0, c0, kr0, kr1, kc0, kc1) in seg.tiles:
        cover[r0 + kr0:min(r0 + kr1, rows), c0 + kc0:min(c0 + kc1, cols)] += 1
    assert int(cover.min()) == 1 and int(cover.max()) == 1, "keep windows must partition the view"
    out = seg(view)
    assert out.shape == (3, rows, cols) and torch.isfinite(out).all()
    assert torch.equal(out, seg(view))
    halves = deploy.WholeViewSegmenter(m, rows, cols, planes=P, tile=(th, tw), batch=5, dtype=torch.float16, use_graph=True)
    assert torch.equal(out, halves(view)), "one replay of 10 tiles differs from two replays of 5"
    del halves
    for i in (0, 3, 7, 9):                                # spot tiles: per-tile eager forward == the stitched keep window
        p, r0, c0, kr0, kr1, kc0, kc1 = seg.tiles[i]
        crop = torch.zeros((1, P, th, tw), device="cuda")
        hh, ww = min(th, rows - r0), min(tw, cols - c0)
        crop[0, :, :hh, :ww] = view[:, 0, r0:r0 + hh, c0:c0 + ww]
        sc = _forward(m, crop, torch.float16)[0]
        y1, x1 = min(kr1, rows - r0), min(kc1, cols - c0)
        assert torch.equal(out[:, r0 + kr0:r0 + y1, c0 + kc0:c0 + x1], sc[:, kr0:y1, kc0:x1]), "tile %d" % i
    # the fixture tile: the reference's class map inside the tile's keep window, f16 bars
    p, r0, c0, kr0, kr1, kc0, kc1 = seg.tiles[0]
    assert (r0, c0) == (0, 0)
    am = out[:, kr0:kr1, kc0:kc1].argmax(0).cpu().numpy()
    ram = g["argmax"].reshape(th, tw)[kr0:kr1, kc0:kc1]
    safe = np.unpackbits(g["safe_0p2"])[:th * tw].astype(bool).reshape(th, tw)[kr0:kr1, kc0:kc1]
    assert float((am[safe] == ram[safe]).mean()) >= 0.9995
    cm = np.bincount(ram[safe].astype(np.int64) * 3 + am[safe], minlength=9).reshape(3, 3)
    iou = [cm[c, c] / max(1, cm[c].sum() + cm[:, c].sum() - cm[c, c]) for c in range(3)]
    assert min(iou) >= 0.99, iou


# ----------------------------------------------------------------------------------------------------------------------
# launch count
# ----------------------------------------------------------------------------------------------------------------------
def _recorded_forward(m, x, dt):
    """forward through a fresh launch plan -> (launches on the tape, operator names, launches per operator call)"""
    from ubresnet_amd import autograd_fn, plan
    m.__dict__.pop("_ubr_engine", None)
    _forward(m, x, dt)
    rec, streams = plan.recorded_forward(autograd_fn._engine(m, "aspp"), x, dt)
    assert rec is not None, "the forward was not recorded"
    per = rec.launches_per_operator(streams)
    torch.cuda.synchronize()
    return rec.tape.size(), rec.operator_names(), per


def test_folded_forward_issues_fewer_launches_and_one_per_aspp_front(golden_dir, monkeypatch):
    g = np.load(os.path.join(golden_dir, SMALL))
    m, x = _model(g)
    n_fold, names, per = _recorded_forward(m, x, torch.float16)
    fronts = [i for i, n in enumerate(names) if n == "aspp_front"]
    assert len(fronts) == 3
    for i in fronts:
        assert per[i] == 1, "an ASPP level's front must be one launch"
        assert names[i + 1] == "conv" and per[i + 1] == 1, "ASPP_post (one 1x1 conv launch) must follow the front"
    assert "maxpool_fwd" not in names[fronts[0]:fronts[-1] + 2], "no separate pool launch between the ASPP levels"
    monkeypatch.setattr(engine, "_INFER_FOLD", False)
    n_plain, names_plain, _ = _recorded_forward(m, x, torch.float16)
    assert "aspp_front" not in names_plain
    print("launches on the forward tape: folded %d, UBR_INFER_FOLD=0 %d" % (n_fold, n_plain))
    assert n_fold < n_plain
