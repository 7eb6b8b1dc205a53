"""Flip test-time augmentation through the deployment surface (GPU): segment_crops(tta=...) against the merge of tests/tta_ref.py
applied to plain calls of the same function on the flipped inputs, flip equivariance bit for bit, WholeViewSegmenter(tta=...)
against the stitch of segment_crops(tta=...) on the same crops (graph replay and eager, scores and event products, per-plane and
stacked tiles), tta off against a segmenter built without the argument, and the recapture after the model's storage moved.
Seeded models from the oracle, fp32 compute."""
import ctypes as C

import numpy as np
import pytest
import torch

import post_ref
import tta_ref as R

pytestmark = pytest.mark.gpu

from oracle import uresnet_oracle as O

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import deploy

P, ROWS, COLS, TH, TW = 3, 80, 144, 64, 96
_CACHE = {}


def _uresnet():
    if "uresnet" not in _CACHE:
        sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
        _CACHE["uresnet"] = deploy.load_model(None, "cuda:0", num_classes=3, state_dict=sd)
    return _CACHE["uresnet"]


def _aspp():
    if "aspp" not in _CACHE:
        sd = O.seeded_state_dict(O.aspp_resnet_schema(3, 3, 16), 42)
        _CACHE["aspp"] = deploy.load_model(None, "cuda:0", num_classes=3, input_channels=3, state_dict=sd, arch="aspp")
    return _CACHE["aspp"]


def _sparse(shape, seed, amp=100.0):
    """a tenth of the pixels carry charge, as on a wire plane; above the ADC threshold of the lit test where they do"""
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.rand(*shape) * (rs.rand(*shape) > 0.9) * amp).astype(np.float32)).cuda()


def _crops(model, x, tta=None, batch=2, **kw):
    """segment_crops at the compute type the segmenters below are built with"""
    model.compute_dtype = torch.float32
    try:
        return deploy.segment_crops(model, x, batch=batch, tta=tta, **kw)
    finally:
        model.compute_dtype = None


def _within(got, views, flips, what):
    """got [n,C,H,W] against tta_ref.merge of the plain outputs `views` (view k computed on the input flipped by flips[k])"""
    n, Cn, H, W = got.shape
    ref, lim = R.merge([v.cpu().numpy().reshape(n * Cn, H, W) for v in views], flips)
    g = got.cpu().numpy().astype(np.float64).reshape(n * Cn, H, W)
    assert np.isfinite(ref).all() and np.isfinite(g).all(), what
    ratio = np.abs(g - ref) / lim
    print("%s: worst error / bound %.3f" % (what, float(ratio.max())))
    i = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert float(ratio.max()) <= 1.0, "%s: at %s got %r, fp64 %r, bound %.3e" % (what, i, g[i], ref[i], lim[i])
    return ref


_DIMS = {1: [2], 2: [3], 3: [2, 3]}


def _tflip(x, flip):
    return torch.flip(x, _DIMS[flip]).contiguous() if flip else x


@pytest.mark.parametrize("tta", [("cols",), ("rows", "cols", "both")], ids=["cols", "all"])
def test_segment_crops_is_the_merge_of_plain_calls(tta):
    m = _uresnet()
    x = _sparse((3, 1, 64, 96), 11)
    flips = [0] + [{"rows": 1, "cols": 2, "both": 3}[t] for t in tta]
    got = _crops(m, x, tta)
    assert got.shape == (3, 3, 64, 96) and got.dtype == torch.float32
    views = [_crops(m, _tflip(x, f)) for f in flips]               # the same forward launches on the same bytes: only the merge differs
    ref = _within(got, views, flips, "segment_crops tta=%s" % (tta,))
    # the mean of the views' probabilities: a pixel's classes sum to the mean of the views' own sums (each 1 to fp32 rounding)
    sums = np.mean([np.exp(R.flip_planes(v.cpu().numpy().reshape(9, 64, 96), f).astype(np.float64)).reshape(3, 3, 64, 96).sum(1)
                    for v, f in zip(views, flips)], axis=0)
    assert np.abs(np.exp(ref).reshape(3, 3, 64, 96).sum(1) - sums).max() < 1e-12
    assert torch.equal(got, _crops(m, x, tta)), "not reproducible"
    assert torch.equal(got, _crops(m, x, tta, batch=3)), "the batch size shows in the result"


def test_two_views_are_flip_equivariant_bit_for_bit():
    m = _uresnet()
    x = _sparse((3, 1, 64, 96), 12)
    fx = _tflip(x, 2)
    a, b = _crops(m, x, ("cols",)), _crops(m, fx, ("cols",))
    assert torch.equal(b, torch.flip(a, [3])), "K = 2 and lae is symmetric: the mirror image must get the mirrored answer"
    pa, pb = _crops(m, x), _crops(m, fx)
    assert not torch.equal(pb, torch.flip(pa, [3])), "the network is flip-equivariant by itself: the check above shows nothing"


def _tile_crops(view, tiles, stacked):
    """the crops ubr_crop_tiles makes, by slicing: [ntiles, cin, TH, TW], zero beyond the view"""
    out = torch.zeros((len(tiles), P if stacked else 1, TH, TW), device="cuda")
    for t, (p, r0, c0, *_) in enumerate(tiles):
        hh, ww = min(TH, ROWS - r0), min(TW, COLS - c0)
        src = view[:, 0] if stacked else view[p:p + 1, 0]
        out[t, :, :hh, :ww] = src[:, r0:r0 + hh, c0:c0 + ww]
    return out


def _stitch(scores, tiles, oplanes):
    out = torch.full((oplanes, scores.shape[1], ROWS, COLS), float("nan"), device="cuda")
    desc = deploy._desc7(tiles)
    L.check(L.lib().ubr_stitch_tiles(scores.data_ptr(), scores.shape[1], TH, TW, desc, len(tiles), out.data_ptr(), oplanes, ROWS, COLS,
                                     L.stream_ptr()), "stitch_tiles")
    return out


@pytest.mark.parametrize("arch,batch", [("uresnet", 4), ("uresnet", 5), ("aspp", 4), ("aspp", 3)])
def test_whole_view_is_the_stitch_of_merged_crops(arch, batch):
    """batch 4 is the issue's; 5 (per-plane, 12 tiles) and 3 (stacked, 4 tiles) leave a short last chunk"""
    m = _uresnet() if arch == "uresnet" else _aspp()
    stacked = arch == "aspp"
    tta = ("rows", "cols")
    view = _sparse((P, 1, ROWS, COLS), 13)
    kw = dict(planes=P, tile=(TH, TW), batch=batch, dtype=torch.float32, tta=tta)
    seg = deploy.WholeViewSegmenter(m, ROWS, COLS, use_graph=True, **kw)
    assert seg.tiles_per_event == (4 if stacked else 12) and (seg.tiles_per_event % batch != 0) == (batch in (5, 3))
    out = seg(view)
    oplanes = 1 if stacked else P
    assert out.shape == ((3, ROWS, COLS) if stacked else (P, 3, ROWS, COLS)) and torch.isfinite(out).all()
    assert torch.equal(out, seg(view)), "replay is not repeatable"
    eager = deploy.WholeViewSegmenter(m, ROWS, COLS, use_graph=False, **kw)
    assert torch.equal(out, eager(view)), "hipGraph replay differs from eager launches"
    # the same crops in the same batches through segment_crops, then the unchanged stitch
    merged = _crops(m, _tile_crops(view, seg.tiles, stacked), tta, batch=batch)
    want = _stitch(merged, seg.tiles, oplanes)
    assert not torch.isnan(want).any()
    assert torch.equal(out.reshape(want.shape), want)
    plain = deploy.WholeViewSegmenter(m, ROWS, COLS, use_graph=True, **dict(kw, tta=None))(view)
    assert not torch.equal(out, plain), "the views changed nothing"
    # event products from the merged scores
    prod = deploy.WholeViewSegmenter(m, ROWS, COLS, use_graph=True, output="products", **kw)(view)
    ref = post_ref.reference(merged.cpu().numpy(), 3, TH, TW, seg.tiles, view[:, 0].cpu().numpy(), P if stacked else 1, 10.0,
                             np.zeros((oplanes, ROWS, COLS), np.uint8), np.zeros((oplanes, ROWS, COLS), np.uint16),
                             np.zeros((oplanes, 3), np.int64), 255, oplanes, ROWS, COLS)
    assert int(ref["lit"].sum()) > 100
    post_ref.accept(prod.label.cpu().numpy().reshape(oplanes, ROWS, COLS), prod.confidence.cpu().numpy().view(np.uint16).reshape(oplanes, ROWS, COLS),
                    prod.counts.cpu().numpy().reshape(oplanes, 3), ref, what="%s products, tta" % arch)
    crops_prod = _crops(m, _tile_crops(view, seg.tiles, stacked), tta, batch=batch, output="products")
    assert crops_prod.label.shape == (len(seg.tiles), TH, TW) and int(crops_prod.counts.sum()) > 0


def test_tta_off_is_the_segmenter_without_the_argument():
    m = _uresnet()
    view = _sparse((P, 1, ROWS, COLS), 14)
    kw = dict(planes=P, tile=(TH, TW), batch=4, dtype=torch.float32)
    base = deploy.WholeViewSegmenter(m, ROWS, COLS, **kw)(view)
    for off in (None, ()):
        seg = deploy.WholeViewSegmenter(m, ROWS, COLS, tta=off, **kw)
        assert torch.equal(seg(view), base) and seg._tta_side is None and seg._tta_merged is None
    x = _sparse((3, 1, 64, 96), 15)
    assert torch.equal(_crops(m, x, None), _crops(m, x, ())) and torch.equal(_crops(m, x), _crops(m, x, None))


def test_segmenter_with_tta_recaptures_on_replaced_storage():
    sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
    m = deploy.load_model(None, "cuda:0", num_classes=3, state_dict=sd)       # a model of its own: its storage is replaced below
    view = _sparse((P, 1, ROWS, COLS), 16)
    seg = deploy.WholeViewSegmenter(m, ROWS, COLS, planes=P, tile=(TH, TW), batch=4, dtype=torch.float32, tta=("both",))
    a = seg(view)
    side = seg._tta_side
    for p_ in m.parameters():                 # every parameter moves to new storage with the same values
        p_.data = p_.data.clone()
    b = seg(view)
    assert seg._tta_side is not side, "the side buffers are dropped with the captured graph"
    assert torch.equal(a, b)
    m.to("cuda:0")
    assert torch.equal(a, seg(view))
    with pytest.raises(RuntimeError):
        deploy.segment_crops(m, view[:, :, :64, :96].cpu(), tta=("cols",))     # tta needs the input on the device
