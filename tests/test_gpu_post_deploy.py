"""Event products through the Python surface (GPU): WholeViewSegmenter(output="products") and segment_crops(output="products")
against the numpy reference of tests/post_ref.py applied on the host to the dense scores of the same call -- labels and counts
exactly, confidence by the rule of post_ref -- and output="scores" still bit-equal between hipGraph replay and eager launches."""
import os

import numpy as np
import pytest
import torch

import post_ref as R

pytestmark = pytest.mark.gpu

from oracle import uresnet_oracle as O
from ubresnet_amd import synthetic

if torch.cuda.is_available():
    from ubresnet_amd import deploy

THR = 10.0


def _uresnet(golden_dir):
    """seeded UResNet(num_classes=4, input_channels=1, inplanes=16) with the running statistics the reference calibrated"""
    g = np.load(os.path.join(golden_dir, "uresnet_ip16_nc4_norm_1x1x64x96.npz"))
    wseed = int(g["meta"][5])
    sd = O.state_dict_with_bn_stats(O.seeded_state_dict(O.uresnet_schema(4, 1, 16, 16), wseed), g["bn_keys"], g["bn_stats"])
    return deploy.load_model(None, "cuda:0", num_classes=4, state_dict=sd)


def _aspp(golden_dir):
    """seeded ASPP_ResNet(3, in_channels=3), calibrated likewise"""
    g = np.load(os.path.join(golden_dir, "aspp_ip16_norm_1x3x64x96.npz"))
    wseed = int(g["meta"][5])
    sd = O.state_dict_with_bn_stats(O.seeded_state_dict(O.aspp_resnet_schema(3, 3, 16), wseed), g["bn_keys"], g["bn_stats"])
    return deploy.load_model(None, "cuda:0", num_classes=3, input_channels=3, state_dict=sd, arch="aspp")


def _view(P, rows, cols, seed):
    v = np.zeros((P, 1, rows, cols), np.float32)
    for p in range(P):
        v[p, 0] = synthetic.make_crop(rows, cols, seed + p)[0]
    return v


def _host_products(scores, adc, vplanes, thr, fill=255):
    """the reference on dense scores [P,C,rows,cols]: every plane is one whole-view tile"""
    P, Cn, rows, cols = scores.shape
    desc = [(p, 0, 0, 0, rows, 0, cols) for p in range(P)]
    return R.reference(scores, Cn, rows, cols, desc, adc, vplanes, thr, np.zeros((P, rows, cols), np.uint8),
                       np.zeros((P, rows, cols), np.uint16), np.zeros((P, Cn), np.int64), fill, P, rows, cols)


def _bits(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def _check(prod, ref, what, lead=True):
    assert prod.label.dtype == torch.uint8 and prod.confidence.dtype == torch.float16 and prod.counts.dtype == torch.int64
    lab, cf, cnt = prod.label.cpu().numpy(), _bits(prod.confidence), prod.counts.cpu().numpy()
    if not lead:                                              # stacked: the plane axis is dropped
        lab, cf, cnt = lab[None], cf[None], cnt[None]
    share = R.accept(lab, cf, cnt, ref, what)
    print("%s: %d lit pixels of %d, near-tie share %.3f %%" % (what, int(ref["lit"].sum()), ref["lit"].size, 100 * share))


@pytest.fixture(scope="module")
def per_plane(golden_dir):
    """one model, one view, the dense scores once (graph replay), shared by the tests below"""
    m = _uresnet(golden_dir)
    P, rows, cols = 3, 96, 160
    view = torch.from_numpy(_view(P, rows, cols, 8100)).cuda()
    kw = dict(rows=rows, cols=cols, planes=P, tile=(64, 96), batch=4, dtype=torch.float32)
    scores = deploy.WholeViewSegmenter(m, output="scores", **kw)(view)
    return m, view, kw, scores


def test_per_plane_products_equal_the_reference_on_the_scores(per_plane):
    m, view, kw, scores = per_plane
    assert scores.shape == (3, 4, 96, 160) and torch.isfinite(scores).all()
    assert torch.equal(scores, deploy.WholeViewSegmenter(m, **kw)(view)), "output='scores' is the default"
    eager = deploy.WholeViewSegmenter(m, use_graph=False, **kw)
    assert torch.equal(scores, eager(view)), "hipGraph replay differs from eager launches"
    seg = deploy.WholeViewSegmenter(m, output="products", **kw)
    assert seg.tiles_per_event == 12
    prod = seg(view)
    assert isinstance(prod, deploy.Products)
    assert prod.label.shape == (3, 96, 160) and prod.confidence.shape == (3, 96, 160) and prod.counts.shape == (3, 4)
    ref = _host_products(scores.cpu().numpy(), view.cpu().numpy()[:, 0], 1, THR)
    assert 0 < ref["lit"].sum() < ref["lit"].size
    _check(prod, ref, "per-plane")
    again = seg(view)                                         # counts are zeroed per event, not accumulated across calls
    assert all(torch.equal(a, b) for a, b in zip(prod, again))
    eager_prod = deploy.WholeViewSegmenter(m, output="products", use_graph=False, **kw)(view)
    assert all(torch.equal(a, b) for a, b in zip(prod, eager_prod))


def test_threshold_off_lights_every_pixel(per_plane):
    m, view, kw, scores = per_plane
    prod = deploy.WholeViewSegmenter(m, output="products", adc_threshold=None, fill_label=7, **kw)(view)
    ref = _host_products(scores.cpu().numpy(), None, 1, THR)
    assert ref["lit"].all()
    _check(prod, ref, "threshold off")
    assert int(prod.counts.sum()) == 3 * 96 * 160 and int(prod.label.max()) <= 3


def test_fill_label_and_threshold_are_the_callers(per_plane):
    m, view, kw, scores = per_plane
    prod = deploy.WholeViewSegmenter(m, output="products", adc_threshold=40.0, fill_label=9, **kw)(view)
    ref = _host_products(scores.cpu().numpy(), view.cpu().numpy()[:, 0], 1, 40.0, fill=9)
    _check(prod, ref, "threshold 40, fill 9")
    assert bool((prod.label[view[:, 0] <= 40.0] == 9).all())


def test_stacked_products_equal_the_reference_on_the_scores(golden_dir):
    m = _aspp(golden_dir)
    P, rows, cols = 3, 64, 160
    view = torch.from_numpy(_view(P, rows, cols, 8200)).cuda()
    kw = dict(rows=rows, cols=cols, planes=P, tile=(64, 96), batch=4, dtype=torch.float16)
    scores = deploy.WholeViewSegmenter(m, output="scores", **kw)(view)
    assert scores.shape == (3, rows, cols) and torch.isfinite(scores).all()
    assert torch.equal(scores, deploy.WholeViewSegmenter(m, use_graph=False, **kw)(view)), "hipGraph replay differs from eager launches"
    seg = deploy.WholeViewSegmenter(m, output="products", **kw)
    assert seg.stacked and seg.tiles_per_event == 2
    prod = seg(view)
    assert prod.label.shape == (rows, cols) and prod.confidence.shape == (rows, cols) and prod.counts.shape == (3,)
    ref = _host_products(scores.cpu().numpy()[None], view.cpu().numpy()[:, 0], 3, THR)
    assert np.array_equal(ref["lit"][0], (view[:, 0] > THR).any(0).cpu().numpy())
    _check(prod, ref, "stacked", lead=False)


def test_precropped_products(per_plane):
    m = per_plane[0]
    x = torch.from_numpy(synthetic.make_batch(5, 64, 64, 8300)[0]).cuda()
    scores = deploy.segment_crops(m, x, batch=2)
    assert scores.shape == (5, 4, 64, 64)
    prod = deploy.segment_crops(m, x, batch=2, output="products")
    assert prod.label.shape == (5, 64, 64) and prod.counts.shape == (5, 4)
    ref = _host_products(scores.cpu().numpy(), x.cpu().numpy()[:, 0], 1, THR)
    _check(prod, ref, "pre-cropped")


def test_bad_arguments(per_plane):
    m, view, kw, _ = per_plane
    with pytest.raises(ValueError):
        deploy.WholeViewSegmenter(m, output="labels", **kw)
    with pytest.raises(ValueError):
        deploy.segment_crops(m, view, output="labels")
    with pytest.raises(RuntimeError, match="fill_label"):    # the library's own check surfaces with ubp_last_error
        deploy.WholeViewSegmenter(m, output="products", fill_label=256, **kw)(view)
