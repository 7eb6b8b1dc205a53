"""Temperature scaling through the deployment surface (GPU): WholeViewSegmenter(temperature=) and segment_crops(temperature=) with
the seeded UResNet of the oracle, fp32 compute, a 3 x 1 x 96 x 160 view, tiles of 64 x 96 and batch 4.  temperature=None against a
segmenter built without the argument; temperature=T against ubf_apply run by hand on the untempered tile scores, pasted through
the keep windows; per-plane temperatures; tta and blend against the same pipeline assembled from the existing calls; products
against the tempered scores; graph replay against eager launches; a Calibration fitted here as `temperature`;
epoch.validate(calibration=) -- everything bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import uresnet_oracle as O

if torch.cuda.is_available():
    from ubresnet_amd import _blend as VL
    from ubresnet_amd import _calib as F
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _tta as TL
    from ubresnet_amd import calibration as CB
    from ubresnet_amd import deploy

P, ROWS, COLS, TH, TW, BATCH = 3, 96, 160, 64, 96, 4
TEMPS = [0.5, 1.0, 2.5]
_CACHE = {}


def _uresnet():
    if "uresnet" not in _CACHE:
        sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
        _CACHE["uresnet"] = deploy.load_model(None, "cuda:0", num_classes=3, state_dict=sd)
    return _CACHE["uresnet"]


def _view():
    if "view" not in _CACHE:
        rs = np.random.RandomState(117)
        shape = (P, 1, ROWS, COLS)
        _CACHE["view"] = torch.from_numpy((rs.rand(*shape) * (rs.rand(*shape) > 0.9) * 100.0).astype(np.float32)).cuda()
    return _CACHE["view"]


def _segmenter(**kw):
    return deploy.WholeViewSegmenter(_uresnet(), ROWS, COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float32, **kw)


def _crops(tiles, view):
    crops = torch.zeros((len(tiles), 1, TH, TW), device="cuda")
    for t, (p, r0, c0, *_) in enumerate(tiles):
        hh, ww = min(TH, ROWS - r0), min(TW, COLS - c0)
        crops[t, 0, :hh, :ww] = view[p, 0, r0:r0 + hh, c0:c0 + ww]
    return crops


def _tile_scores(tiles, flips=(None,)):
    """the untempered per-tile forwards, made once per (tiling, view set): for every flip view the model's output in the
    segmenter's batches -> list over views of [ntiles, C, TH, TW] on the device"""
    key = ("tiles", tuple(tiles), tuple(flips))
    if key not in _CACHE:
        m, crops = _uresnet(), _crops(tiles, _view())
        m.compute_dtype = torch.float32
        try:
            outs = []
            for flip in flips:
                x = crops
                if flip:
                    x = torch.empty_like(crops)
                    TL.flip_planes(crops.data_ptr(), x.data_ptr(), crops.shape[0], TH, TW, flip, L.stream_ptr())
                with torch.no_grad():
                    outs.append(torch.cat([m(x[i:i + BATCH]) for i in range(0, len(tiles), BATCH)], 0).contiguous())
            _CACHE[key] = outs
        finally:
            m.compute_dtype = None
    return [o.clone() for o in _CACHE[key]]


def _apply_by_hand(scores, groups, temps):
    betas = torch.from_numpy(CB.TemperatureScale(temps).betas_for(groups)).cuda()
    n, C, H, W = scores.shape
    F.apply(scores.data_ptr(), scores.data_ptr(), betas.data_ptr(), n, C, H, W, L.stream_ptr())
    return scores


def _paste(tiles, logp):
    want = torch.full((P, 3, ROWS, COLS), float("nan"), device="cuda")
    for t, (p, r0, c0, kr0, kr1, kc0, kc1) in enumerate(tiles):
        r1, c1 = min(r0 + kr1, ROWS), min(c0 + kc1, COLS)
        want[p, :, r0 + kr0:r1, c0 + kc0:c1] = logp[t][:, kr0:r1 - r0, kc0:c1 - c0]
    assert not torch.isnan(want).any()
    return want


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_temperature_none_is_the_segmenter_without_the_argument():
    view = _view()
    for output in ("scores", "products", "pixels"):
        base, seg = _segmenter(output=output)(view), _segmenter(output=output, temperature=None)(view)
        if output == "scores":
            assert _same_bits(base, seg)
        elif output == "products":
            assert all(torch.equal(x, y) for x, y in zip(base, seg))
        else:
            assert all(np.array_equal(x, y) for x, y in zip(base.read(), seg.read())) and torch.equal(base.counts, seg.counts)
    m = _uresnet()
    m.compute_dtype = torch.float32
    try:
        crops = _crops(_segmenter().tiles[:5], view)
        assert _same_bits(deploy.segment_crops(m, crops, batch=BATCH), deploy.segment_crops(m, crops, batch=BATCH, temperature=None))
    finally:
        m.compute_dtype = None


@pytest.mark.parametrize("temps", [[1.7], TEMPS])
def test_scores_are_apply_by_hand_on_the_tile_scores_then_stitched(temps):
    seg = _segmenter(temperature=temps if len(temps) > 1 else temps[0])
    out = seg(_view())
    groups = [t[0] if len(temps) > 1 else 0 for t in seg.tiles]
    assert len(temps) == 1 or set(groups) == {0, 1, 2}
    want = _paste(seg.tiles, _apply_by_hand(_tile_scores(seg.tiles)[0], groups, temps))
    assert _same_bits(out, want)
    plain = _segmenter()(_view())
    assert not torch.equal(out, plain)
    if len(temps) > 1:
        # T = 1 on plane 1 moves nothing but the rounding of the renormalisation: u (2 |z| + |out| + 4 L + rS) of tests/calib_ref.py,
        # below 4 u max |x| + 1e-5 for these three classes; T = 0.5 on plane 0 doubles the distances
        lim = 4 * 2.0 ** -24 * float(plain[1].abs().max()) + 1e-5
        assert float((out[1] - plain[1]).abs().max()) <= lim and float((out[0] - plain[0]).abs().max()) > 1e-2
    assert _same_bits(seg(_view()), out), "replay is not repeatable"
    assert _same_bits(_segmenter(temperature=temps, use_graph=False)(_view()), out), "hipGraph replay differs from eager launches"
    # the pre-cropped loop: one temperature for every crop
    if len(temps) == 1:
        m = _uresnet()
        m.compute_dtype = torch.float32
        try:
            got = deploy.segment_crops(m, _crops(seg.tiles, _view()), batch=BATCH, temperature=temps[0])
        finally:
            m.compute_dtype = None
        assert _same_bits(got, _apply_by_hand(_tile_scores(seg.tiles)[0], groups, temps))


def test_with_tta_every_view_is_tempered_before_the_merge():
    seg = _segmenter(temperature=TEMPS, tta=("cols", "both"))
    out = seg(_view())
    flips = seg._flips
    assert len(flips) == 3 and flips[0] == 0
    groups = [t[0] for t in seg.tiles]
    views = [_apply_by_hand(v, groups, TEMPS) for v in _tile_scores(seg.tiles, flips)]
    merged = torch.empty_like(views[0])
    for k, (flip, v) in enumerate(zip(flips, views)):
        TL.merge_view(v.data_ptr(), merged.data_ptr(), merged.shape[0] * merged.shape[1], TH, TW, flip, k, len(flips), L.stream_ptr())
    assert _same_bits(out, _paste(seg.tiles, merged))
    assert not torch.equal(out, _segmenter(tta=("cols", "both"))(_view()))


def test_with_blend_the_tiles_are_tempered_before_they_vote():
    seg = _segmenter(temperature=TEMPS, margin=8, blend="linear")
    out = seg(_view())
    groups = [t[0] for t in seg.tiles]
    logp = _apply_by_hand(_tile_scores(seg.tiles)[0], groups, TEMPS)
    want = torch.empty((P, 3, ROWS, COLS), device="cuda")
    VL.blend_begin(want.data_ptr(), want.numel(), L.stream_ptr())
    for i in range(0, len(seg.tiles), BATCH):
        chunk = seg.tiles[i:i + BATCH]
        VL.blend_tiles(logp[i:].data_ptr(), 3, TH, TW, VL.desc3(chunk), len(chunk), seg._blend_lw[0][i:].data_ptr(),
                       seg._blend_lw[1][i:].data_ptr(), want.data_ptr(), P, ROWS, COLS, L.stream_ptr())
    assert _same_bits(out, want)
    assert not torch.equal(out, _segmenter(margin=8, blend="linear")(_view()))


def test_products_are_the_arg_max_and_the_top_probability_of_the_tempered_scores():
    view = _view()
    # the seeded, untrained network is thousands of nat sure of itself: temperatures that bring its top probability off 1.0
    hot = [2000.0, 1.0, 6000.0]
    scores = _segmenter(temperature=hot)(view)
    prod = _segmenter(temperature=hot, output="products")(view)
    lit = view[:, 0] > 10.0
    assert int(lit.sum()) > 100
    top, arg = scores.max(1)
    assert torch.equal(prod.label[lit].long(), arg[lit]) and bool((prod.label[~lit] == 255).all())
    conf = torch.exp(top).to(torch.float16)
    a, b = prod.confidence[lit].view(torch.int16).int(), conf[lit].view(torch.int16).int()
    print("confidence: %d of %d halves differ, by at most %d" % (int((a != b).sum()), a.numel(), int((a - b).abs().max())))
    assert torch.equal(a, b), "the confidence is not the top probability of the tempered scores rounded to half"
    assert bool((prod.confidence[~lit] == 0).all())
    plain = _segmenter(output="products")(view)
    assert not torch.equal(plain.confidence, prod.confidence)
    assert 0.3 < float(prod.confidence[0][lit[0]].float().mean()) < 0.999, "plane 0 is as sure as before"
    pix = _segmenter(temperature=hot, output="pixels")(view)
    idx, lab, conf_l = pix.read()
    assert len(idx) == int(lit.sum()) and np.array_equal(lab, prod.label[lit].cpu().numpy())
    # sparse input: the same products
    from ubresnet_amd import sparse
    sp = _segmenter(temperature=hot, output="products")(sparse.SparseEvent.from_dense(view))
    assert all(torch.equal(x, y) for x, y in zip(sp, prod))


def test_a_calibration_fitted_here_is_accepted_as_temperature():
    view = _view()
    seg = _segmenter()
    scores = seg(view)
    rs = np.random.RandomState(9)
    # labels drawn from the network's own probabilities at T0 per plane: the fit must move towards T0
    T0 = [0.6, 1.0, 2.0]
    p = torch.softmax(scores.double() / torch.tensor(T0, device="cuda", dtype=torch.float64).reshape(3, 1, 1, 1), 1).cpu().numpy()
    u = rs.rand(P, 1, ROWS, COLS)
    truth = torch.from_numpy((u > np.cumsum(p, 1)).sum(1).clip(0, 2).astype(np.uint8)).cuda()
    fit = CB.TemperatureFit(3, groups=P)
    fit.add(scores, truth, lit=view)
    cal = fit.read()
    lit = int((view > 10.0).sum())
    assert int(cal.counters[:, 0].sum()) == lit and not any(cal.empty)
    print("fitted temperatures", cal.temperatures, "drawn at", T0, "at_edge", cal.at_edge)
    tempered = _segmenter(temperature=cal)(view)
    by_list = _segmenter(temperature=cal.temperatures)(view)
    assert _same_bits(tempered, by_list) and _same_bits(tempered, _segmenter(temperature=cal.scale())(view))
    # the NLL of the tempered scores at T = 1 is the minimum: a second fit over them finds T = 1 within the grid's resolution
    again = CB.TemperatureFit(3, groups=P)
    again.add(tempered, truth, lit=view)
    for g, t in enumerate(again.read().temperatures):
        assert cal.at_edge[g] or abs(np.log(t)) < 0.02, (g, t)


def test_validate_fills_the_fit_and_returns_what_it_returned():
    from ubresnet_amd.training import epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    from ubresnet_amd import synthetic
    x, lab, wgt = synthetic.make_batch(2, 64, 64, 1000)
    batch = (torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(wgt).cuda())

    class _Stager:
        def next(self):
            return batch

    m = _uresnet()
    lines_a, lines_b = [], []
    base = epoch.validate(_Stager(), m, PixelWiseNLLLoss(), 2, nclasses=3, log=lines_a.append)
    fit = CB.TemperatureFit(3, groups=1)
    got = epoch.validate(_Stager(), m, PixelWiseNLLLoss(), 2, nclasses=3, log=lines_b.append, calibration=fit)
    assert got == base and fit.calls == 2 and len(lines_a) == len(lines_b)
    assert lines_a[-1] == lines_b[-1] and lines_a[-1].startswith("Test:Result*")              # the lines before carry wall-clock times
    cal = fit.read()
    assert int(cal.counters[0, 0]) == 2 * int((batch[0] > 10.0).sum()) and cal.table[0].any()
