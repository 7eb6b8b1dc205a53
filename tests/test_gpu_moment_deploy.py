"""ClusterMoments behind whole-view inference (GPU): the seeded UResNet, the 3 x 1 x 96 x 160 cut of a synthetic labelled event and
the tiles of tests/test_gpu_cluster_deploy.py.  WholeViewSegmenter(output="products") -> EventClusterer -> ClusterMoments: the
table equals tests/moment_ref.py on the downloaded products, ids and view bit for bit, and the charge of a plane's clusters is the
scaled, rounded ADC sum of its lit pixels.  The same with output="pixels" feeding the clusterer and a SparseEvent feeding both the
segmenter and the moments."""
import numpy as np
import pytest
import torch

import moment_ref as R

pytestmark = pytest.mark.gpu

from oracle import uresnet_oracle as O

if torch.cuda.is_available():
    from ubresnet_amd import clusters, deploy, shapes, sparse, synthetic

P, ROWS, COLS, TH, TW, BATCH, C, SCALE = 3, 96, 160, 64, 96, 4, 3, 16
_CACHE = {}


def _model():
    if "model" not in _CACHE:
        sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
        _CACHE["model"] = deploy.load_model(None, "cuda:0", num_classes=C, state_dict=sd)
    return _CACHE["model"]


def _view():
    if "view" not in _CACHE:
        image, _ = synthetic.make_labelled_event(P, ROWS, COLS, 77)
        _CACHE["view"] = torch.from_numpy(image[:, None].copy()).cuda()
    return _CACHE["view"]


def _segmenter(output):
    return deploy.WholeViewSegmenter(_model(), ROWS, COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float32, output=output)


def _reference():
    """the table from the downloaded products, ids and view of the dense path, computed once"""
    if "ref" not in _CACHE:
        products = _segmenter("products")(_view())
        cl = clusters.EventClusterer(P, ROWS, COLS, C, 8, False, 255, 4096, "cuda:0")
        found = cl(products)
        torch.cuda.synchronize()
        ids, count = found.ids.cpu().numpy(), int(found.count.item())
        label, view = products.label.cpu().numpy(), _view()[:, 0].cpu().numpy()
        _CACHE["ref"] = (R.table(ids, label, view, C, SCALE, 4096, count), ids, label, view, count)
    return _CACHE["ref"]


def _plane_charge(ids, view):
    """the scaled, rounded ADC sum of every plane's lit pixels, without the table"""
    w, _, _ = R.weight(view, SCALE)
    return [int(w[p][ids[p] >= 0].sum()) for p in range(P)]


def test_products_feed_the_clusterer_and_the_moments():
    ref, ids, label, view, count = _reference()
    products = _segmenter("products")(_view())
    cl = clusters.EventClusterer(P, ROWS, COLS, C, 8, False, 255, 4096, "cuda:0")
    cm = shapes.ClusterMoments(cl, adc_scale=SCALE)
    mom = cm(cl(products), _view())
    torch.cuda.synchronize()
    assert count >= P and (mom.table[:count].cpu().numpy() == ref).all()
    tab = mom.read()
    assert len(tab) == len(tab.clusters) == count and tab.rows.numpy().tolist() == ref.tolist()
    per_plane = torch.zeros(P, dtype=torch.float64).index_add_(0, tab.clusters.plane, tab.charge())
    want = _plane_charge(ids, view)
    assert min(want) > 0 and per_plane.tolist() == [w / SCALE for w in want]
    assert (tab.weighted <= tab.clusters.pixels).all() and bool((tab.class_charge().sum(dim=1) == tab.charge()).all())
    box, cen = tab.clusters.bbox.double(), tab.centroid()
    has = tab.rows[:, 3] > 0
    assert bool(((cen[:, 0] >= box[:, 0]) & (cen[:, 0] <= box[:, 1]) & (cen[:, 1] >= box[:, 2]) & (cen[:, 1] <= box[:, 3]))[has].all())
    lin = tab.linearity()[has]
    assert bool(((lin >= 0) & (lin <= 1))[~torch.isnan(lin)].all())
    big = mom.read(min_pixels=4)
    assert (big.clusters.pixels >= 4).all() and big.rows.numpy().tolist() == ref[tab.clusters.pixels.numpy() >= 4].tolist()


def test_a_pixel_list_and_a_sparse_event_give_the_same_table():
    ref, ids, label, view, count = _reference()
    event = sparse.SparseEvent.from_dense(_view().cpu())
    pl = _segmenter("pixels")(event)
    cl = clusters.EventClusterer(P, ROWS, COLS, C, 8, False, 255, 4096, "cuda:0")
    cm = shapes.ClusterMoments(cl, adc_scale=SCALE)
    found = cl(pl)                                               # expanded on the device (PixelList.to_products)
    mom = cm(found, event)
    torch.cuda.synchronize()
    assert int(found.count.item()) == count and (found.ids.cpu().numpy() == ids).all()
    assert (mom.table[:count].cpu().numpy() == ref).all()
    tab = mom.read()
    per_plane = torch.zeros(P, dtype=torch.float64).index_add_(0, tab.clusters.plane, tab.charge())
    assert per_plane.tolist() == [w / SCALE for w in _plane_charge(ids, view)]
