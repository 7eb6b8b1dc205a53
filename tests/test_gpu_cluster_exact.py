"""libubresnet_cluster.so on the device against the numpy reference of tests/cluster_ref.py, bit for bit: root, ids, count, table
and status.  With T_H x T_W the tile of the local pass, the views are 1x1x1, 1x1x(T_W+1), 1x(T_H+1)x1, 2x(2T_H+3)x(2T_W+5) and
3x(T_H-1)x(T_W-1); the patterns are those of cluster_ref.PATTERNS (empty, all lit, checkerboard, a diagonal through every tile, a
serpentine, a "U", a diagonal touch across a four-tile corner, row wrap, plane wrap, striped classes, foreign labels, random fields
at 1 / 41 / 59 / 90 % lit), each at both connectivities with and without by_class, and one 3 x 200 x 700 cut of
synthetic.make_labelled_event.  Then: confidence edge values; capacity overflow; ubi_tabulate alone on hand-made root maps (S + 1
pixel blocks: the scan's second trip; one wave of two interleaved clusters and of 64 clusters); of_pixels; two calls and two
streams; a captured graph replayed over a changed input."""
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


def test_numbering_across_two_scan_trips():
    """ubi_tabulate alone on a hand-made root map of S + 1 pixel blocks, S the scan width: the second trip of the one-workgroup
    scan and its carry.  Every root is a cluster of one pixel, so the expected values are closed forms: ids is the exclusive
    cumulative sum of the root flags, count the number of roots, and table row k below the capacity is the k-th root's pixel."""
    from ubresnet_amd import _lib as L
    P, rows, cols, C = 1, I.SCAN_WIDTH + 1, I.PIXEL_BLOCK, R.C4
    n = P * rows * cols
    assert -(-n // I.PIXEL_BLOCK) == I.SCAN_WIDTH + 1
    flag = np.random.default_rng(1025).random(n) < 0.003
    flag[[5, n - 3]] = True                                      # a root in block 0 and one in block S
    q = np.flatnonzero(flag)
    capacity = 1000
    assert capacity < len(q) < 2 * 0.003 * n and q[0] < I.PIXEL_BLOCK and q[-1] >= I.SCAN_WIDTH * I.PIXEL_BLOCK
    root = np.where(flag, np.arange(n), -1).astype(np.int32)
    label = np.where(flag, np.arange(n) % C, R.FILL).astype(np.uint8)
    want_ids = np.where(flag, np.cumsum(flag) - flag, -1).astype(np.int32)
    want = np.zeros((capacity, R.TABLE_FIXED + C), np.int64)     # root, pixels, row_min, row_max, col_min, col_max, conf_sum, nonfinite
    k, qk = np.arange(capacity), q[:capacity]
    want[:, 0], want[:, 1], want[:, 6] = qk, 1, 1 << 24           # fix(1.0) = 2^24
    want[:, 2], want[:, 3], want[:, 4], want[:, 5] = qk // cols, qk // cols, qk % cols, qk % cols
    want[k, R.TABLE_FIXED + qk % C] = 1
    d_root, d_label = torch.from_numpy(root).cuda(), torch.from_numpy(label).cuda()
    d_conf = torch.full((n,), 1.0, dtype=torch.float16, device="cuda")
    ids = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    table = torch.full((len(q), R.TABLE_FIXED + C), -77, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(I.scratch_bytes(P, rows, cols) // 4, dtype=torch.int32, device="cuda")
    I.tabulate(d_label.data_ptr(), d_conf.data_ptr(), d_root.data_ptr(), C, R.FILL, ids.data_ptr(), table.data_ptr(), capacity,
               count.data_ptr(), scratch.data_ptr(), P, rows, cols, L.stream_ptr())
    torch.cuda.synchronize()
    got_ids, got = ids.cpu().numpy(), table.cpu().numpy()
    assert int(count.item()) == len(q)
    assert (got_ids == want_ids).all(), "ids: first difference at %s" % (np.flatnonzero(got_ids != want_ids)[:1].tolist(),)
    assert (got[:capacity] == want).all(), "table: first difference at row, column %s" % (np.argwhere(got[:capacity] != want)[:1].tolist(),)
    assert (got[capacity:] == -77).all(), "a row at or past the capacity was written"


@pytest.mark.parametrize("shape_of_keys", ["interleaved", "distinct"])
def test_the_tally_on_one_wave_of_hand_made_roots(shape_of_keys):
    """ubi_tabulate alone on one row of 64 pixels, all lit, the tally's whole wave: two clusters interleaved lane by lane (which
    no labelling of a single row can make), and 64 clusters of one pixel"""
    from ubresnet_amd import _lib as L
    n, C = 64, R.C4
    q = np.arange(n)
    root = (q % 2 if shape_of_keys == "interleaved" else q).astype(np.int32).reshape(1, 1, n)
    label, conf = (q // 3 % C).astype(np.uint8).reshape(1, 1, n), R.confidence_bits((1, 1, n))
    want_ids, want, want_count = R.tabulate(label, conf, root, C)
    assert want_count == (2 if shape_of_keys == "interleaved" else n) and want[:, 1].sum() == n
    ids = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    table = torch.full((want_count, R.TABLE_FIXED + C), -77, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(I.scratch_bytes(1, 1, n) // 4, dtype=torch.int32, device="cuda")
    (dl, dc), dr = _dev(label, conf), torch.from_numpy(root).cuda()
    I.tabulate(dl.data_ptr(), dc.data_ptr(), dr.data_ptr(), C, R.FILL, ids.data_ptr(), table.data_ptr(), want_count, count.data_ptr(),
               scratch.data_ptr(), 1, 1, n, L.stream_ptr())
    torch.cuda.synchronize()
    assert int(count.item()) == want_count and (ids.cpu().numpy() == want_ids.reshape(-1)).all()
    assert (table.cpu().numpy() == want).all(), (table.cpu().numpy().tolist(), want.tolist())


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
