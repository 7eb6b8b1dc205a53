"""Overlap-tile inference through the deployment surface (GPU): WholeViewSegmenter(margin=, blend=) with seeded models from the
oracle, fp32 compute, a 3 x 1 x 96 x 160 view, tiles of 64 x 96 and batch 4 (and a 112 x 176 view, where a margin of 16 makes the
tiling denser).  margin=0, blend=None against a segmenter built without the arguments; margin=16 against the per-tile forwards
pasted through the keep windows, bit for bit; blend="linear" / "hann" against tests/blend_ref.py applied to the per-tile outputs
the model produced (within the derived bound; bit-equal where a single tile has weight); blend after the flip merge; event
products from the blended scores against tests/post_ref.py; the stacked ASPP_ResNet form."""
import numpy as np
import pytest
import torch

import blend_ref as R
import post_ref

pytestmark = pytest.mark.gpu

from oracle import uresnet_oracle as O

if torch.cuda.is_available():
    from ubresnet_amd import deploy

P, ROWS, COLS, TH, TW, BATCH = 3, 96, 160, 64, 96, 4
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


def _view(rows=ROWS, cols=COLS):
    key = ("view", rows, cols)
    if key not in _CACHE:
        _CACHE[key] = _sparse((P, 1, rows, cols), 21 + rows)
    return _CACHE[key]


def _segmenter(model, rows=ROWS, cols=COLS, **kw):
    return deploy.WholeViewSegmenter(model, rows, cols, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float32, **kw)


def _tile_outputs(model, view, tiles, stacked, tta=None):
    """the per-tile forwards, made once per (model, tiling): the crops ubr_crop_tiles makes, by slicing (zero beyond the view),
    through segment_crops in the segmenter's batches -> [ntiles, C, TH, TW] on the host"""
    key = ("tiles", stacked, tuple(tiles), tuple(view.shape), tta)
    if key not in _CACHE:
        rows, cols = view.shape[2:]
        crops = torch.zeros((len(tiles), P if stacked else 1, TH, TW), device="cuda")
        for t, (p, r0, c0, *_) in enumerate(tiles):
            hh, ww = min(TH, rows - r0), min(TW, cols - c0)
            src = view[:, 0] if stacked else view[p:p + 1, 0]
            crops[t, :, :hh, :ww] = src[:, r0:r0 + hh, c0:c0 + ww]
        model.compute_dtype = torch.float32
        try:
            _CACHE[key] = deploy.segment_crops(model, crops, batch=BATCH, tta=tta).cpu().numpy()
        finally:
            model.compute_dtype = None
    return _CACHE[key]


def _reference(seg, logp, rows=ROWS, cols=COLS):
    """blend_ref on the per-tile outputs, in the segmenter's chunks, with the tables the segmenter holds on the device (which are
    the reference's own within one rounding of the float64 logarithm) -> (ref, bound, lw_rows, lw_cols)"""
    lwr, lwc = (t.cpu().numpy() for t in seg._blend_lw)
    ro, co = R.margin_tiling(rows, cols, TH, TW, seg.margin)
    oplanes = 1 if seg.stacked else P
    desc = [t[:3] for t in seg.tiles]
    assert desc == R.view_desc(oplanes, ro, co)
    tr, tc = R.view_tables(oplanes, ro, co, TH, TW, rows, cols, seg.margin, seg.blend)
    for mine, ref in ((lwr, tr), (lwc, tc)):
        assert mine.dtype == np.float32 and mine.shape == ref.shape and np.array_equal(np.isneginf(mine), np.isneginf(ref))
        assert np.array_equal(mine.view(np.uint32)[ref == 0], ref.view(np.uint32)[ref == 0])          # +0 where a tile stands alone
        fin = np.isfinite(ref)
        assert (np.abs(mine[fin].astype(np.float64) - ref[fin]) <= np.spacing(np.abs(ref[fin]))).all()
    calls = [(logp[i:i + BATCH], desc[i:i + BATCH], lwr[i:i + BATCH], lwc[i:i + BATCH]) for i in range(0, len(desc), BATCH)]
    ref, lim, count = R.blend(np.full((oplanes, 3, rows, cols), -np.inf, np.float32), calls)
    assert (count >= 1).all() and (count >= 2).any() and (count == 4).any()
    return ref, lim, lwr, lwc


def _within(got, ref, lim, what):
    g = got.cpu().numpy().astype(np.float64).reshape(ref.shape)
    assert np.isfinite(ref).all() and np.isfinite(g).all(), what
    err = np.abs(g - ref)                                        # a bound of zero admits no error
    ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err == 0, 0.0, np.inf))
    print("%s: worst error / bound %.3f" % (what, float(ratio.max())))
    i = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert float(ratio.max()) <= 1.0, "%s: at %s got %r, fp64 %r, bound %.3e" % (what, i, g[i], ref[i], lim[i])


def test_the_defaults_are_the_segmenter_without_the_arguments():
    m, view = _uresnet(), _view()
    base = _segmenter(m)(view)
    seg = _segmenter(m, margin=0, blend=None)
    assert torch.equal(seg(view), base) and seg._blend_lw is None and seg._blend_out is None
    a = _segmenter(m, output="products")(view)
    b = _segmenter(m, output="products", margin=0, blend=None)(view)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("rows,cols,per_plane", [(ROWS, COLS, 4), (112, 176, 9)])
def test_margin_16_is_the_per_tile_forwards_pasted_through_the_keep_windows(rows, cols, per_plane):
    m, view = _uresnet(), _view(rows, cols)
    seg = _segmenter(m, rows, cols, margin=16)
    assert seg.tiles_per_event == P * per_plane and seg.tiles == deploy.view_tiles(rows, cols, P, TH, TW, False, 16)
    out = seg(view)
    logp = _tile_outputs(m, view, seg.tiles, False)
    want = np.full((P, 3, rows, cols), np.nan, np.float32)
    for t, (p, r0, c0, kr0, kr1, kc0, kc1) in enumerate(seg.tiles):
        assert (r0 == 0 or kr0 >= 16) and (r0 + TH >= rows or TH - kr1 >= 16) and (c0 == 0 or kc0 >= 16) and (c0 + TW >= cols or TW - kc1 >= 16)
        want[p, :, r0 + kr0:r0 + kr1, c0 + kc0:c0 + kc1] = logp[t][:, kr0:kr1, kc0:kc1]
    assert not np.isnan(want).any()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    prod = _segmenter(m, rows, cols, margin=16, output="products")(view)
    assert prod.label.shape == (P, rows, cols) and int(prod.counts.sum()) > 100


@pytest.mark.parametrize("kind", ["linear", "hann"])
def test_blend_is_the_reference_on_the_tile_outputs(kind):
    m, view = _uresnet(), _view()
    seg = _segmenter(m, margin=8, blend=kind)
    out = seg(view)
    assert out.shape == (P, 3, ROWS, COLS) and out.dtype == torch.float32
    bits = out.cpu().numpy().view(np.uint32).copy()
    logp = _tile_outputs(m, view, seg.tiles, False)
    ref, lim, lwr, lwc = _reference(seg, logp)
    _within(out, ref, lim, "blend=%s" % kind)
    # where a single tile has weight (every other covering tile is inside its margin or its ramp has not begun) that weight is
    # +0 and the tile's bits arrive
    weighted = np.zeros((P, ROWS, COLS), int)
    alone = np.zeros((P, 3, ROWS, COLS), np.uint32)
    for t, (p, r0, c0, *_) in enumerate(seg.tiles):
        w = np.isfinite(lwr[t])[:, None] & np.isfinite(lwc[t])[None, :]
        weighted[p, r0:r0 + TH, c0:c0 + TW] += w
        one = (lwr[t][:, None] == 0) & (lwc[t][None, :] == 0)
        alone[p, :, r0:r0 + TH, c0:c0 + TW][:, one] = logp[t].view(np.uint32)[:, one]
    single = np.broadcast_to(weighted[:, None] == 1, alone.shape)
    assert (weighted >= 1).all() and 0.2 < single.mean() < 0.9
    assert np.array_equal(bits[single], alone[single]), "a pixel that one tile weights does not hold that tile's bits"
    plain = _segmenter(m, margin=8)(view)
    assert not torch.equal(out, plain), "the blend changed nothing"
    assert torch.equal(seg(view), out), "replay is not repeatable"
    eager = _segmenter(m, margin=8, blend=kind, use_graph=False)(view)
    assert torch.equal(eager, out), "hipGraph replay differs from eager launches"


def test_blend_after_the_flip_merge():
    m, view = _uresnet(), _view()
    seg = _segmenter(m, margin=8, blend="linear", tta=("cols",))
    out = seg(view)
    merged = _tile_outputs(m, view, seg.tiles, False, tta=("cols",))
    ref, lim, _, _ = _reference(seg, merged)
    _within(out, ref, lim, "blend=linear, tta=cols")
    assert not torch.equal(out, _segmenter(m, margin=8, blend="linear")(view)), "the views changed nothing"


@pytest.mark.parametrize("kind", ["linear", "hann"])
def test_products_with_blend_are_post_ref_on_the_blended_scores(kind):
    m, view = _uresnet(), _view()
    scores = _segmenter(m, margin=8, blend=kind)(view)
    seg = _segmenter(m, margin=8, blend=kind, output="products")
    prod = seg(view)
    assert torch.equal(seg._blend_out, scores), "the dense buffer of the products path is not the scores path's result"
    whole = [(p, 0, 0, 0, ROWS, 0, COLS) for p in range(P)]
    ref = post_ref.reference(scores.cpu().numpy(), 3, ROWS, COLS, whole, view[:, 0].cpu().numpy(), 1, 10.0,
                             np.zeros((P, ROWS, COLS), np.uint8), np.zeros((P, ROWS, COLS), np.uint16), np.zeros((P, 3), np.int64), 255,
                             P, ROWS, COLS)
    assert int(ref["lit"].sum()) > 100
    post_ref.accept(prod.label.cpu().numpy(), prod.confidence.cpu().numpy().view(np.uint16), prod.counts.cpu().numpy(), ref,
                    what="products, blend=%s" % kind)
    again = seg(view)
    assert all(torch.equal(x, y) for x, y in zip(prod, again)), "the kept buffer shows in a second call"


def test_stacked_aspp_form():
    m, view = _aspp(), _view()
    seg = _segmenter(m, margin=8, blend="hann")
    assert seg.stacked and seg.tiles_per_event == 4
    out = seg(view)
    assert out.shape == (3, ROWS, COLS) and torch.isfinite(out).all()
    logp = _tile_outputs(m, view, seg.tiles, True)
    ref, lim, _, _ = _reference(seg, logp)
    _within(out, ref, lim, "stacked, blend=hann")
    prod = _segmenter(m, margin=8, blend="hann", output="products")(view)
    assert prod.label.shape == (ROWS, COLS) and prod.counts.shape == (3,) and int(prod.counts.sum()) > 100
    ref_p = post_ref.reference(out.cpu().numpy()[None], 3, ROWS, COLS, [(0, 0, 0, 0, ROWS, 0, COLS)], view[:, 0].cpu().numpy(), P, 10.0,
                               np.zeros((1, ROWS, COLS), np.uint8), np.zeros((1, ROWS, COLS), np.uint16), np.zeros((1, 3), np.int64), 255,
                               1, ROWS, COLS)
    post_ref.accept(prod.label.cpu().numpy()[None], prod.confidence.cpu().numpy().view(np.uint16)[None], prod.counts.cpu().numpy()[None], ref_p,
                    what="stacked products, blend=hann")
