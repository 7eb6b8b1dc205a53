"""ClusterOverlap behind whole-view inference (GPU): the seeded, untrained UResNet, the 3 x 1 x 96 x 160 cut of a synthetic labelled
event and the tiles of tests/test_gpu_moment_deploy.py.  WholeViewSegmenter(output="products") -> EventClusterer gives the
predicted clusters, overlap.truth_products -> EventClusterer the true ones, and ClusterOverlap matches the two with the view: the
table equals tests/overlap_ref.py on the downloaded maps bit for bit, its marginal over b is the `pixels` column of the predicted
ClusterTable, and its charge marginal is ShapeTable.charge() of ClusterMoments on the same clusters.  A SparseEvent view gives the
same bytes as the dense one."""
import numpy as np
import pytest
import torch

import overlap_ref as R

pytestmark = pytest.mark.gpu

from oracle import uresnet_oracle as O

if torch.cuda.is_available():
    from ubresnet_amd import clusters, deploy, overlap, shapes, sparse, synthetic

P, ROWS, COLS, TH, TW, BATCH, C, SCALE, CAPACITY = 3, 96, 160, 64, 96, 4, 3, 16, 4096
_CACHE = {}


def _event():
    if "event" not in _CACHE:
        image, truth = synthetic.make_labelled_event(P, ROWS, COLS, 77)
        _CACHE["event"] = (torch.from_numpy(image[:, None].copy()).cuda(), torch.from_numpy(truth).cuda())
    return _CACHE["event"]


def _clusterings():
    """(predicted Clusters, its clusterer, true Clusters, its clusterer), computed once and left unchanged"""
    if "found" not in _CACHE:
        view, truth = _event()
        sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
        model = deploy.load_model(None, "cuda:0", num_classes=C, state_dict=sd)
        seg = deploy.WholeViewSegmenter(model, ROWS, COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float32, output="products")
        cl_pred = clusters.EventClusterer(P, ROWS, COLS, C, 8, False, 255, CAPACITY, "cuda:0")
        cl_true = clusters.EventClusterer(P, ROWS, COLS, C, 8, True, 255, CAPACITY, "cuda:0")
        pred = cl_pred(seg(view))
        true = cl_true(*overlap.truth_products(truth, view))
        torch.cuda.synchronize()
        _CACHE["found"] = (pred, cl_pred, true, cl_true)
    return _CACHE["found"]


def test_truth_products_are_the_lit_truth():
    view, truth = _event()
    label, conf = overlap.truth_products(truth, view, adc_threshold=10.0)
    lit = (view[:, 0] > 10.0).cpu().numpy()
    want = np.where(lit, truth.cpu().numpy(), 255).astype(np.uint8)
    assert label.dtype == torch.uint8 and (label.cpu().numpy() == want).all() and 0 < lit.sum() < lit.size
    assert conf.dtype == torch.float16 and conf.shape == label.shape and bool((conf == 1).all())
    ignored = truth.long().clone()
    ignored[:, ::2] = -100
    label2, _ = overlap.truth_products(ignored, view[:, 0].contiguous(), fill_label=7)
    assert (label2[:, ::2] == 7).all() and (label2[:, 1::2].cpu().numpy() == np.where(lit, truth.cpu().numpy(), 7)[:, 1::2]).all()


def test_predicted_clusters_against_true_clusters_with_the_view():
    view, _ = _event()
    pred, cl_pred, true, _ = _clusterings()
    co = overlap.ClusterOverlap(P, ROWS, COLS, CAPACITY, None, SCALE, "cuda:0")
    ov = co(pred, true, view)
    mom = shapes.ClusterMoments(cl_pred, adc_scale=SCALE)(pred, view)
    torch.cuda.synchronize()
    ref = R.table(pred.ids.cpu().numpy(), true.ids.cpu().numpy(), view[:, 0].cpu().numpy(), SCALE)
    count = int(ov.count.item())
    assert count == len(ref) >= P and ov.status.tolist() == [0, 0] and (ov.table[:count].cpu().numpy() == ref).all()
    tab = ov.read()
    assert tab.rows.numpy().tolist() == ref.tolist() and tab.adc_scale == SCALE
    found, shape = pred.read(), mom.read()
    assert list(tab.sizes_a()) == list(range(len(found))) and list(tab.sizes_a().values()) == found.pixels.tolist()
    assert list(tab.sizes_b().values()) == true.read().pixels.tolist()
    assert [q / SCALE for q in tab.sizes_a(weighted=True).values()] == shape.charge().tolist()
    # the matching is usable: values in 0..1, best matches exist where both sides cover the pixel, ARI in -1..1
    for m in (tab.purity(), tab.efficiency(), tab.purity(weighted=True)):
        ok = ~torch.isnan(m.value)
        assert bool(((m.value[ok] >= 0) & (m.value[ok] <= 1)).all())
    assert -1.0 <= tab.ari() <= 1.0
    pairs = tab.matched(0.0, 0.0)
    assert len(pairs) + len(tab.unmatched_a()) == len(found) and len(pairs) + len(tab.unmatched_b()) == len(tab.sizes_b())


def test_a_sparse_event_view_gives_the_bytes_of_the_dense_one():
    view, _ = _event()
    pred, _, true, _ = _clusterings()
    co = overlap.ClusterOverlap(P, ROWS, COLS, CAPACITY, None, SCALE, "cuda:0")
    dense = co(pred, true, view)
    torch.cuda.synchronize()
    want, count = dense.table.cpu().numpy().tobytes(), int(dense.count.item())
    event = sparse.SparseEvent.from_dense(view.cpu())
    for _ in range(2):                                           # the scatter buffer is kept between the calls
        co.table.zero_()
        got = co(pred, true, event)
        torch.cuda.synchronize()
        assert int(got.count.item()) == count and got.table[:count].cpu().numpy().tobytes() == want[:count * 48]
    assert co._dense is not None and co._dense.shape == (P, 1, ROWS, COLS)
