"""EventClusters behind whole-view inference (GPU): a seeded UResNet, fp32 compute, a 3 x 1 x 96 x 160 cut of a synthetic labelled
event, tiles of 64 x 96 and batch 4.  WholeViewSegmenter(output="products") and output="pixels" feed an EventClusterer; the result
equals tests/cluster_ref.py on the downloaded products bit for bit, the `pixels` of the table sum to the products' lit counts per
plane, and of_pixels gives the cluster of every entry of the pixel list."""
import numpy as np
import pytest
import torch

import cluster_ref as R

pytestmark = pytest.mark.gpu

from oracle import uresnet_oracle as O

if torch.cuda.is_available():
    from ubresnet_amd import clusters, deploy, synthetic

P, ROWS, COLS, TH, TW, BATCH, C = 3, 96, 160, 64, 96, 4, 3
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


def _reference(label, conf, conn, by_class):
    return R.reference(label.cpu().numpy(), conf.cpu().numpy().view(np.uint16), C, 255, conn, by_class)


def _same(found, ref):
    torch.cuda.synchronize()
    assert (found.root.cpu().numpy() == ref["root"]).all() and (found.ids.cpu().numpy() == ref["ids"]).all()
    assert int(found.count.item()) == ref["count"] and int(found.status.item()) == ref["foreign"] == 0
    assert (found.table[:ref["count"]].cpu().numpy() == ref["table"]).all()


@pytest.mark.parametrize("conn,by_class", [(8, False), (4, True)])
def test_products_feed_the_clusterer(conn, by_class):
    products = _segmenter("products")(_view())
    cl = clusters.EventClusterer(P, ROWS, COLS, C, conn, by_class, 255, 4096, "cuda:0")
    found = cl(products)
    ref = _reference(products.label, products.confidence, conn, by_class)
    assert ref["count"] >= P, "the event has lit pixels in every plane"
    _same(found, ref)
    tab = found.read()
    assert len(tab) == tab.total == ref["count"]
    lit = products.counts.cpu().sum(dim=1)                       # lit pixels per plane
    per_plane = torch.zeros(P, dtype=torch.int64).index_add_(0, tab.plane, tab.pixels)
    assert per_plane.tolist() == lit.tolist()
    assert torch.zeros((P, C), dtype=torch.int64).index_add_(0, tab.plane, tab.class_counts).tolist() == products.counts.cpu().tolist()
    assert bool((tab.fractions().sum(dim=1) - 1).abs().max() < 1e-12) and bool((tab.mean_confidence() > 0).all())
    assert (tab.bbox[:, 0] <= tab.bbox[:, 1]).all() and (tab.bbox[:, 2] <= tab.bbox[:, 3]).all() and int(tab.bbox[:, 3].max()) < COLS


def test_a_pixel_list_feeds_the_clusterer_and_of_pixels():
    products = _segmenter("products")(_view())
    ref = _reference(products.label, products.confidence, 8, False)
    pl = _segmenter("pixels")(_view())
    cl = clusters.EventClusterer(P, ROWS, COLS, C, 8, False, 255, 4096, "cuda:0")
    found = cl(pl)                                               # expanded on the device (PixelList.to_products)
    _same(found, ref)
    k = clusters.of_pixels(found, pl)
    index, _, _ = pl.read()
    assert k.dtype == torch.int32 and k.shape == pl.index.shape
    got = k.cpu().numpy()
    assert (got[:len(index)] == ref["ids"].reshape(-1)[index.numpy()]).all() and (got[:len(index)] >= 0).all()
    assert (got[len(index):] == -1).all()
    assert (found.ids.reshape(-1)[pl.index[:len(index)].long()] == k[:len(index)]).all()
