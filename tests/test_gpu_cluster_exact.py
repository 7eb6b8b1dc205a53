"""libubresnet_cluster.so on the device against the numpy reference of tests/cluster_ref.py, bit for bit: root, ids, count, table
and status.  With T_H x T_W the tile of the local pass, the views are 1x1x1, 1x1x(T_W+1), 1x(T_H+1)x1, 2x(2T_H+3)x(2T_W+5) and
3x(T_H-1)x(T_W-1); the patterns are those of cluster_ref.PATTERNS (empty, all lit, checkerboard, a diagonal through every tile, a
serpentine, a "U", a diagonal touch across a four-tile corner, row wrap, plane wrap, striped classes, foreign labels, random fields
at 1 / 41 / 59 / 90 % lit), each at both connectivities with and without by_class, and one 3 x 200 x 700 cut of
synthetic.make_labelled_event.  Then: confidence edge values; capacity overflow; of_pixels; two calls and two streams; a captured
graph replayed over a changed input."""
import numpy as np
import pytest
import torch

import cluster_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import clusters, sparse, synthetic
    from ubresnet_amd import _cluster as I

_CACHE = {}


def _dev(label, conf):
    return torch.from_numpy(label).cuda(), torch.from_numpy(conf.view(np.float16)).cuda()


def _clusterer(shape, conn, by_class, capacity=None, C=R.C4):
    P, rows, cols = shape
    return clusters.EventClusterer(P, rows, cols, C, conn, by_class, R.FILL, capacity or P * rows * cols, "cuda:0")


def _host(found):
    torch.cuda.synchronize()
    return dict(root=found.root.cpu().numpy(), ids=found.ids.cpu().numpy(), table=found.table.cpu().numpy(),
                count=int(found.count.item()), status=int(found.status.item()))


def _same(got, ref, rows=None):
    """root, ids, count and status equal the reference; so do the first `rows` table rows (every row of the reference if None)"""
    assert got["root"].dtype == np.int32 and got["ids"].dtype == np.int32 and got["table"].dtype == np.int64
    assert (got["root"] == ref["root"]).all(), "root: first difference at %s" % (np.argwhere(got["root"] != ref["root"])[:1].tolist(),)
    assert (got["ids"] == ref["ids"]).all(), "ids: first difference at %s" % (np.argwhere(got["ids"] != ref["ids"])[:1].tolist(),)
    assert got["count"] == ref["count"] and got["status"] == ref["foreign"], (got["count"], ref["count"], got["status"], ref["foreign"])
    n = ref["count"] if rows is None else rows
    bad = np.argwhere(got["table"][:n] != ref["table"][:n])
    assert bad.size == 0, "table: first difference at row, column %s: %s against %s" % (
        bad[0].tolist(), got["table"][bad[0][0]].tolist(), ref["table"][bad[0][0]].tolist())


def test_geometry_is_the_reference_geometry():
    assert (I.TILE_H, I.TILE_W, I.PIXEL_BLOCK, I.TABLE_FIXED) == (R.T_H, R.T_W, R.PIXEL_BLOCK, R.TABLE_FIXED)
    assert R.VIEWS == {"1x1x1": (1, 1, 1), "row": (1, 1, R.T_W + 1), "col": (1, R.T_H + 1, 1),
                       "four-tiles": (2, 2 * R.T_H + 3, 2 * R.T_W + 5), "one-short": (3, R.T_H - 1, R.T_W - 1)}


@pytest.mark.parametrize("view", sorted(R.VIEWS))
@pytest.mark.parametrize("pattern", sorted(R.PATTERNS))
def test_patterns_on_every_view_bit_for_bit(view, pattern):
    shape = R.VIEWS[view]
    label, conf = R.PATTERNS[pattern](*shape), R.confidence_bits(shape)
    dl, dc = _dev(label, conf)
    for conn, by_class in R.MODES:
        ref = R.reference(label, conf, R.C4, R.FILL, conn, by_class)
        got = _host(_clusterer(shape, conn, by_class)(dl, dc))
        _same(got, ref)


def _event():
    """a 3 x 200 x 700 cut of a synthetic labelled event: the label where the image is above 10 ADC, the fill label elsewhere"""
    if "event" not in _CACHE:
        image, label = synthetic.make_labelled_event(3, 256, 768, 4242)
        image, label = image[:, 20:220, 30:730], label[:, 20:220, 30:730]
        lab = np.where(image > 10.0, label, R.FILL).astype(np.uint8)
        conf = R.confidence_bits(lab.shape, seed=11)
        _CACHE["event"] = (np.ascontiguousarray(lab), conf, {m: R.reference(lab, conf, 3, R.FILL, *m) for m in ((8, False), (4, True))})
    return _CACHE["event"]


@pytest.mark.parametrize("conn,by_class", [(8, False), (4, True)])
def test_a_cut_of_a_synthetic_labelled_event(conn, by_class):
    lab, conf, refs = _event()
    assert lab.shape == (3, 200, 700) and 0.002 < R.lit_mask(lab, 3, R.FILL).mean() < 0.5
    ref = refs[(conn, by_class)]
    assert ref["count"] > 3
    got = _host(_clusterer(lab.shape, conn, by_class, C=3)(*_dev(lab, conf)))
    _same(got, ref)


def test_stacked_products_count_as_one_plane():
    lab, conf, _ = _event()
    ref = R.reference(lab[:1], conf[:1], 3, R.FILL, 8, False)
    dl, dc = _dev(lab[0], conf[0])
    found = _clusterer((1, 200, 700), 8, False, C=3)(dl, dc)
    assert found.ids.shape == found.root.shape == (200, 700)
    got = _host(found)
    _same(dict(got, root=got["root"][None], ids=got["ids"][None]), ref)


def test_confidence_edge_values():
    """one cluster per edge value, and one cluster that holds them all: subnormals, 0x8000, negatives, inf and NaN"""
    edge = np.array([0x0000, 0x0001, 0x03FF, 0x0400, 0x3C00, 0x7BFF, 0x8000, 0x8001, 0xBC00, 0xFBFF, 0x7C00, 0xFC00, 0x7C01, 0x7E00, 0xFFFF],
                    np.uint16)
    n = len(edge)
    label = np.full((2, 3, 2 * n), R.FILL, np.uint8)
    conf = np.full(label.shape, 0x3800, np.uint16)
    label[0, 0, 0::2] = 1                                        # plane 0: separate pixels
    conf[0, 0, 0::2] = edge
    label[1, 1, :n] = 2                                          # plane 1: one run
    conf[1, 1, :n] = edge
    ref = R.reference(label, conf)
    assert ref["count"] == n + 1 and ref["table"][:n, 7].tolist() == [0] * 7 + [1] * 8 and ref["table"][n, 7] == 8
    assert ref["table"][:7, 6].tolist() == [0, 1, 1023, 1024, 1 << 24, 2047 << 29, 0] and ref["table"][n, 6] == sum(ref["table"][:n, 6])
    for conn, by_class in R.MODES:
        _same(_host(_clusterer(label.shape, conn, by_class)(*_dev(label, conf))), R.reference(label, conf, R.C4, R.FILL, conn, by_class))


def test_capacity_overflow_leaves_the_rows_past_capacity_alone():
    shape = R.VIEWS["four-tiles"]
    label, conf = R.PATTERNS["random-41"](*shape), R.confidence_bits(shape)
    ref = R.reference(label, conf)
    capacity = 5
    assert ref["count"] > 4 * capacity
    cl = _clusterer(shape, 8, False, capacity=capacity + 3)      # the last three rows are canaries the library is told nothing of
    cl.capacity = capacity
    cl.table.fill_(-77)
    found = cl(*_dev(label, conf))
    got = _host(found)
    _same(got, ref, rows=capacity)                               # the first rows are right, count is the total, ids is complete
    assert got["count"] == ref["count"] > capacity and (got["table"][capacity:] == -77).all()
    with pytest.raises(OverflowError, match="%d clusters, capacity %d" % (ref["count"], capacity)):
        found._replace(table=found.table[:capacity]).read()
    # capacity 1, and a capacity the count just fits
    for cap in (1, ref["count"] - 1, ref["count"]):
        found = _clusterer(shape, 8, False, capacity=cap)(*_dev(label, conf))
        _same(_host(found), ref, rows=cap)
        if cap < ref["count"]:
            with pytest.raises(OverflowError, match="%d clusters, capacity %d" % (ref["count"], cap)):
                found.read()
    exact = _clusterer(shape, 8, False, capacity=ref["count"])(*_dev(label, conf)).read(min_pixels=3)
    assert exact.total == ref["count"] and exact.rows.numpy().tolist() == ref["table"][ref["table"][:, 1] >= 3].tolist()


def test_of_pixels_is_ids_at_the_listed_pixels():
    lab, conf, refs = _event()
    ref = refs[(8, False)]
    found = _clusterer(lab.shape, 8, False, C=3)(*_dev(lab, conf))
    q = np.flatnonzero(R.lit_mask(lab, 3, R.FILL).reshape(-1)).astype(np.int32)
    stale = 9
    index = torch.from_numpy(np.concatenate([q, np.zeros(stale, np.int32)])).cuda()
    pl = sparse.PixelList(index, torch.zeros(len(index), dtype=torch.uint8).cuda(), torch.zeros(len(index), dtype=torch.float16).cuda(),
                          torch.tensor([len(q)]).cuda(), None, 3, 200, 700, R.FILL)
    out = torch.full((len(index),), -5, dtype=torch.int32, device="cuda")
    assert clusters.of_pixels(found, pl, out=out) is out
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:len(q)] == ref["ids"].reshape(-1)[q]).all() and (got[:len(q)] >= 0).all() and (got[len(q):] == -5).all()
    # a count above the capacity: the whole list, no further; an index outside the image: -1
    index[0], index[1] = -3, lab.size
    got = clusters.of_pixels(found, pl._replace(count=torch.tensor([1 << 40]).cuda())).cpu().numpy()
    assert got[:2].tolist() == [-1, -1] and (got[2:len(q)] == ref["ids"].reshape(-1)[q[2:]]).all() and (got[len(q):] == ref["ids"].reshape(-1)[0]).all()


def test_the_status_word_only_grows():
    shape = R.VIEWS["one-short"]
    label, conf = R.PATTERNS["foreign"](*shape), R.confidence_bits(shape)
    ref = R.reference(label, conf)
    cl = _clusterer(shape, 8, False)
    assert ref["foreign"] > 0 and _host(cl(*_dev(label, conf)))["status"] == ref["foreign"]
    assert _host(cl(*_dev(label, conf)))["status"] == 2 * ref["foreign"]
    assert _host(cl(*_dev(R.PATTERNS["all-lit"](*shape), conf)))["status"] == 2 * ref["foreign"]


def test_two_calls_and_two_streams_give_the_same_bytes():
    shape = R.VIEWS["four-tiles"]
    label, conf = R.PATTERNS["random-59"](*shape), R.confidence_bits(shape)
    ref = R.reference(label, conf, R.C4, R.FILL, 4, False)
    dl, dc = _dev(label, conf)
    a, b = _clusterer(shape, 4, False), _clusterer(shape, 4, False)
    first = _host(a(dl, dc))
    again = _host(a(dl, dc))                                     # the same buffers, overwritten
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        fa = a(dl, dc)
    with torch.cuda.stream(s2):
        fb = b(dl, dc)
    torch.cuda.synchronize()
    for got in (first, again, _host(fa), _host(fb)):
        _same(got, ref)
    assert all((first[k] == again[k]).all() for k in ("root", "ids", "table"))


def test_a_captured_graph_replays_label_and_tabulate_on_a_changed_input():
    shape = R.VIEWS["four-tiles"]
    conf = R.confidence_bits(shape)
    first, second = R.PATTERNS["serpentine"](*shape), R.PATTERNS["random-41"](*shape)
    dl, dc = _dev(first, conf)
    cl = _clusterer(shape, 8, False)
    cl(dl, dc)                                                   # warm-up outside the capture (module load)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        found = cl(dl, dc)
    torch.cuda.synchronize()
    dl.copy_(torch.from_numpy(second).cuda())
    graph.replay()
    replayed = _host(found)
    _same(replayed, R.reference(second, conf))
    eager = _host(_clusterer(shape, 8, False)(dl, dc))
    assert all((replayed[k] == eager[k]).all() for k in ("root", "ids", "table")) and replayed["count"] == eager["count"]
