"""libubresnet_moment.so on the device against the numpy reference of tests/moment_ref.py: the whole table buffer, bit for bit.
`ids` and `count` come from a real EventClusterer run on the same label.  The views and patterns are those of
tests/cluster_ref.py (connectivity 8), with `checker` and `random-41` also 4-connected, where nearly every lit pixel is a cluster
of its own, so that a workgroup meets far more clusters than its LDS table holds (the direct path and the flush of a full table).
Then: the contended case (all lit over many workgroups); a view of several trips per workgroup; dark and foreign pixels; capacity
below the count; stored, not added; the largest accepted plane in closed form; two calls and two streams; a captured graph;
sparse input; one hand-made case across every branch of the pixel walk shared with ClusterOverlap; views below four pixels."""
import numpy as np
import pytest
import torch

import cluster_ref as CR
import moment_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import clusters, shapes, sparse
    from ubresnet_amd import _moment as M

SENTINEL = -0x0123456789ABCDEF
SCALE = 16


def _clusterer(shape, conn=8, capacity=None, C=CR.C4):
    P, rows, cols = shape
    return clusters.EventClusterer(P, rows, cols, C, conn, False, CR.FILL, capacity or P * rows * cols, "cuda:0")


def _conf(shape):
    return torch.from_numpy(CR.confidence_bits(shape).view(np.float16)).cuda()


def _run(label, view, conn=8, capacity=None, C=CR.C4, scale=SCALE, cm=None, cl=None, prefill=SENTINEL):
    """-> (the whole table buffer, ids, count, cm, cl) after EventClusterer + ClusterMoments on the device"""
    cl = cl or _clusterer(label.shape, conn, capacity, C)
    cm = cm or shapes.ClusterMoments(cl, adc_scale=scale)
    if prefill is not None:
        cm.table.fill_(prefill)
    found = cl(torch.from_numpy(label).cuda(), _conf(label.shape))
    mom = cm(found, view if not isinstance(view, np.ndarray) else torch.from_numpy(view).cuda())
    torch.cuda.synchronize()
    return mom.table.cpu().numpy(), found.ids.cpu().numpy(), int(found.count.item()), cm, cl, mom


def _same(got, ids, count, label, view, capacity, C=CR.C4, scale=SCALE, prefill=SENTINEL):
    """the rows below min(count, capacity) equal the reference; the rows at or past it still hold the prefill"""
    ref = R.table(ids.reshape(label.shape), label, view, C, scale, capacity, count)
    n = min(count, capacity)
    assert got.dtype == np.int64 and got.shape == (capacity, R.TABLE_FIXED + C) and ref.shape[0] == n
    bad = np.argwhere(got[:n] != ref)
    assert bad.size == 0, "first difference at row, column %s: %s against %s" % (bad[0].tolist(), got[bad[0][0]].tolist(), ref[bad[0][0]].tolist())
    assert (got[n:] == prefill).all(), "a row at or past min(count, capacity) was touched"
    return ref


def test_geometry_is_the_reference_geometry():
    assert (M.TABLE_FIXED, M.TRIP_PIXELS, M.SLOTS, M.MAX_GRID, M.MAX_WEIGHT) == (R.TABLE_FIXED, R.TRIP_PIXELS, R.SLOTS, R.MAX_GRID, R.MAX_WEIGHT)


@pytest.mark.parametrize("view", sorted(CR.VIEWS))
@pytest.mark.parametrize("pattern", sorted(CR.PATTERNS))
def test_patterns_on_every_view_bit_for_bit(view, pattern):
    shape = CR.VIEWS[view]
    label = CR.PATTERNS[pattern](*shape)
    adc = R.adc(shape, lit=CR.lit_mask(label, CR.C4, CR.FILL))
    capacity = shape[0] * shape[1] * shape[2]
    got, ids, count, _, _, _ = _run(label, adc)
    _same(got, ids, count, label, adc, capacity)


@pytest.mark.parametrize("pattern", ["checker", "random-41"])
def test_far_more_clusters_than_slots_take_the_direct_path_and_the_full_table_flush(pattern):
    shape = CR.VIEWS["four-tiles"]
    label = CR.PATTERNS[pattern](*shape)
    adc = R.adc(shape, lit=CR.lit_mask(label, CR.C4, CR.FILL))
    capacity = shape[0] * shape[1] * shape[2]
    got, ids, count, _, _, _ = _run(label, adc, conn=4)
    per_trip = [len(np.unique(t[t >= 0])) for t in np.array_split(ids.reshape(-1), range(R.TRIP_PIXELS, ids.size, R.TRIP_PIXELS))]
    assert min(per_trip[:-1]) > 2 * R.SLOTS, "every full trip meets more than twice the clusters the LDS table holds"
    _same(got, ids, count, label, adc, capacity)


def test_all_lit_over_many_workgroups_is_the_contended_case():
    shape = (2, 200, 300)
    label = CR.PATTERNS["all-lit"](*shape)
    adc = R.adc(shape, seed=9)
    got, ids, count, _, _, _ = _run(label, adc, capacity=7)
    assert count == 2 and -(-label.size // R.TRIP_PIXELS) == 59, "one row per plane receives everything, from 59 workgroups"
    ref = _same(got, ids, count, label, adc, 7)
    assert (ref[:, 1] > 0).all() and (ref[:, 2] > 0).all(), "clipped and odd pixels in both planes"


def test_several_trips_per_workgroup_on_a_ragged_view():
    """1 x 1201 x 1801 pixels are 1057 trips, above the grid cap: workgroups take spans of two trips, the last trip is ragged and
    the pixel count is odd (the last lane group is loaded pixel by pixel)"""
    shape = (1, 1201, 1801)
    trips = -(-shape[1] * shape[2] // R.TRIP_PIXELS)
    assert trips > R.MAX_GRID and shape[1] * shape[2] % 4 == 1
    rng = np.random.default_rng(31)
    label = np.full(shape, CR.FILL, np.uint8)
    lit = rng.random(shape) < 0.03
    lit[0, 100:140, 200:900] = True                              # a slab that spans trips and workgroups
    lit[0, -1, -5:] = True                                       # the last pixels of the view
    label[lit] = rng.integers(0, CR.C4, int(lit.sum())).astype(np.uint8)
    adc = R.adc(shape, seed=13, lit=lit)
    capacity = 1 << 17
    got, ids, count, _, _, _ = _run(label, adc, capacity=capacity)
    assert 1000 < count < capacity
    _same(got, ids, count, label, adc, capacity)


def test_dark_and_foreign_pixels_change_nothing():
    shape = CR.VIEWS["four-tiles"]
    label = CR.PATTERNS["foreign"](*shape)
    lit = CR.lit_mask(label, CR.C4, CR.FILL)
    adc = R.adc(shape, lit=lit)
    wild = adc.copy()
    wild[~lit] = np.resize(np.array([1e30, np.nan, -5.0, np.inf, -np.inf, 4096.0], np.float32), int((~lit).sum()))
    zeroed = np.where(lit, adc, np.float32(0))
    capacity = label.size
    a, ids, count, _, _, _ = _run(label, wild)
    b, ids_b, count_b, _, _, _ = _run(label, zeroed)
    assert count == count_b and (ids == ids_b).all() and a.tobytes() == b.tobytes()
    _same(a, ids, count, label, zeroed, capacity)


def test_a_label_at_or_past_the_classes_is_odd_and_nothing_else():
    """ubi_label never gives such a pixel a cluster; the kernel guards it anyway: the label map changes after the clustering"""
    shape = CR.VIEWS["one-short"]
    label = CR.PATTERNS["stripes"](*shape)
    adc = R.adc(shape)
    cl = _clusterer(shape)
    cm = shapes.ClusterMoments(cl, adc_scale=SCALE)
    dl = torch.from_numpy(label).cuda()
    found = cl(dl, _conf(shape))
    changed = label.copy()
    changed[:, ::3, ::5] = 4
    changed[:, 1::3, 1::5] = 254
    dl.copy_(torch.from_numpy(changed).cuda())
    cm.table.fill_(SENTINEL)
    mom = cm(found, torch.from_numpy(adc).cuda())
    torch.cuda.synchronize()
    ref = _same(mom.table.cpu().numpy(), found.ids.cpu().numpy(), int(found.count.item()), changed, adc, label.size)
    assert ref[:, 2].sum() >= int((changed >= 4).sum())


def test_capacity_below_the_count_leaves_the_rows_past_it_alone():
    shape = CR.VIEWS["four-tiles"]
    label = CR.PATTERNS["random-41"](*shape)
    adc = R.adc(shape, lit=CR.lit_mask(label, CR.C4, CR.FILL))
    capacity = 5
    cl = _clusterer(shape, capacity=capacity + 3)                # the last three rows are canaries the library is told nothing of
    cm = shapes.ClusterMoments(cl, adc_scale=SCALE)
    cl.capacity = cm.capacity = capacity
    got, ids, count, _, _, mom = _run(label, adc, cm=cm, cl=cl)
    assert count > 4 * capacity and (got[capacity:] == SENTINEL).all()
    ref = R.table(ids, label, adc, CR.C4, SCALE, capacity, count)
    assert ref.shape[0] == capacity and (got[:capacity] == ref).all(), "the reference restricted to ids < capacity"
    with pytest.raises(OverflowError, match="%d clusters, capacity %d" % (count, capacity + 3)):
        mom.read()
    # a capacity the count just fits, and one it just does not
    for cap in (count, count - 1, 1):
        got, ids, n, _, _, mom = _run(label, adc, capacity=cap)
        _same(got, ids, n, label, adc, cap)
        if cap < n:
            with pytest.raises(OverflowError):
                mom.read()
        else:
            tab = mom.read(min_pixels=3)
            keep = tab.clusters.pixels.numpy() >= 3
            assert keep.all() and tab.rows.numpy().tolist() == got[:n][mom.clusters.table[:n, 1].cpu().numpy() >= 3].tolist()


def test_stored_not_added():
    shape = CR.VIEWS["four-tiles"]
    first, second = CR.PATTERNS["serpentine"](*shape), CR.PATTERNS["random-59"](*shape)
    adc1, adc2 = R.adc(shape, seed=1), R.adc(shape, seed=2)
    capacity = first.size
    _, _, _, cm, cl, _ = _run(first, adc1)
    got, ids, count, _, _, _ = _run(second, adc2, cm=cm, cl=cl, prefill=None)      # the same buffers, not cleared by the test
    ref = R.table(ids, second, adc2, CR.C4, SCALE, capacity, count)
    assert (got[:count] == ref).all(), "the second event's table, not the sum of the two"
    garbage, _, _, _, _, _ = _run(second, adc2, prefill=0x7EDCBA9876543210)
    assert (garbage[:count] == ref).all() and garbage[:count].tobytes() == got[:count].tobytes()


def test_the_largest_accepted_plane_in_closed_form():
    """P = 1, 1024 x 4096, all lit, one class, ADC 4095.9375 at scale 16: w = 65535 on every pixel, unclipped.  The expected row
    is a closed form; Qcc = 65535 * 1024 * (4095 * 4096 * 8191 / 6) is about 2^60.4"""
    rows, cols, w = 1024, 4096, 65535
    cl = clusters.EventClusterer(1, rows, cols, 1, 8, False, CR.FILL, 4, "cuda:0")
    cm = shapes.ClusterMoments(cl, adc_scale=16)
    cm.table.fill_(SENTINEL)
    label = torch.zeros((1, rows, cols), dtype=torch.uint8, device="cuda")
    found = cl(label, torch.ones((1, rows, cols), dtype=torch.float16, device="cuda"))
    mom = cm(found, torch.full((1, 1, rows, cols), 4095.9375, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert int(found.count.item()) == 1
    s1 = lambda n: n * (n - 1) // 2
    s2 = lambda n: (n - 1) * n * (2 * n - 1) // 6
    want = [rows * cols, 0, 0, w * rows * cols, w * cols * s1(rows), w * rows * s1(cols), w * cols * s2(rows), w * s1(rows) * s1(cols),
            w * rows * s2(cols), w * rows * cols]
    assert want[8] == 65535 * 1024 * (4095 * 4096 * 8191 // 6) and 2 ** 60 < want[8] < 2 ** 61
    got = mom.table.cpu().numpy()
    assert got[0].tolist() == want and (got[1:] == SENTINEL).all()
    tab = mom.read()
    assert tab.centroid()[0].tolist() == [(rows - 1) / 2, (cols - 1) / 2] and float(tab.charge()[0]) == 4095.9375 * rows * cols
    assert tab.covariance()[0].tolist() == [[(rows * rows - 1) / 12, 0.0], [0.0, (cols * cols - 1) / 12]] and tab.axis()[0].tolist() == [0.0, 1.0]


def test_two_calls_and_two_streams_give_the_same_bytes():
    shape = CR.VIEWS["four-tiles"]
    label = CR.PATTERNS["random-59"](*shape)
    adc = R.adc(shape, lit=CR.lit_mask(label, CR.C4, CR.FILL))
    first, ids, count, cm_a, cl_a, _ = _run(label, adc, conn=4)
    again, _, _, _, _, _ = _run(label, adc, cm=cm_a, cl=cl_a)
    cl_b = _clusterer(shape, 4)
    cm_b = shapes.ClusterMoments(cl_b, adc_scale=SCALE)
    cm_a.table.fill_(SENTINEL), cm_b.table.fill_(SENTINEL)
    dl, dc, dv = torch.from_numpy(label).cuda(), _conf(shape), torch.from_numpy(adc).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        ma = cm_a(cl_a(dl, dc), dv)
    with torch.cuda.stream(s2):
        mb = cm_b(cl_b(dl, dc), dv)
    torch.cuda.synchronize()
    _same(first, ids, count, label, adc, label.size)
    for got in (again, ma.table.cpu().numpy(), mb.table.cpu().numpy()):
        assert got.tobytes() == first.tobytes()


def test_a_captured_graph_replays_label_tabulate_and_moments_on_a_changed_input():
    shape = CR.VIEWS["four-tiles"]
    first, second = CR.PATTERNS["serpentine"](*shape), CR.PATTERNS["random-41"](*shape)
    adc1, adc2 = R.adc(shape, seed=3), R.adc(shape, seed=4)
    dl, dc, dv = torch.from_numpy(first).cuda(), _conf(shape), torch.from_numpy(adc1).cuda()
    cl = _clusterer(shape)
    cm = shapes.ClusterMoments(cl, adc_scale=SCALE)
    cm(cl(dl, dc), dv)                                           # warm-up outside the capture (module load)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mom = cm(cl(dl, dc), dv)
    torch.cuda.synchronize()
    dl.copy_(torch.from_numpy(second).cuda())
    dv.copy_(torch.from_numpy(adc2).cuda())
    cm.table.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    replayed = mom.table.cpu().numpy()
    _same(replayed, mom.clusters.ids.cpu().numpy(), int(mom.clusters.count.item()), second, adc2, second.size)
    eager, _, _, _, _, _ = _run(second, adc2)
    assert eager.tobytes() == replayed.tobytes()


def test_a_sparse_event_equals_the_dense_view():
    shape = CR.VIEWS["four-tiles"]
    label = CR.PATTERNS["random-41"](*shape)
    adc = R.adc(shape, lit=CR.lit_mask(label, CR.C4, CR.FILL))
    adc[np.isnan(adc)] = np.float32(-3.0)                        # (from_dense keeps every element whose bits are not +0.0's)
    event = sparse.SparseEvent.from_dense(torch.from_numpy(adc))
    dense, ids, count, cm, cl, _ = _run(label, adc)
    _same(dense, ids, count, label, adc, label.size)
    for _ in range(2):                                           # the scatter buffer is kept between the calls
        got, _, _, _, _, _ = _run(label, event, cm=cm, cl=cl)
        assert got.tobytes() == dense.tobytes()
    assert cm._dense is not None and cm._dense.shape == (shape[0], 1, shape[1], shape[2])


def _raw(ids, label, view, shape, capacity, count):
    """the whole table buffer after ubm_moments on maps no clusterer made, through the binding alone"""
    dev = [torch.from_numpy(np.ascontiguousarray(x).reshape(shape)).cuda() for x in (ids, label, view)]
    table = torch.full((capacity, R.TABLE_FIXED + CR.C4), SENTINEL, dtype=torch.int64, device="cuda")
    n = torch.tensor([count], dtype=torch.int64, device="cuda")
    M.moments(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), CR.C4, SCALE, table.data_ptr(), capacity, n.data_ptr(), *shape)
    torch.cuda.synchronize()
    return table.cpu().numpy()


def test_one_case_across_every_branch_of_the_shared_walk():
    """moment_ref.walk_case(): 2 * TRIP_PIXELS * 2 + 5 = 8197 pixels whose waves hold one id in all 64 lanes, 64 solo ids, two ids
    interleaved, a lane of two ids (the mixed round), lanes without a pixel, and a ragged last load, with the ADC edge values on
    them; tests/test_gpu_overlap_exact.py runs the same pixels through the other library.  ubm_moments takes at most 4096 columns,
    so the 8197 pixels are a 1 x 7 x 1171 view here: the walk is over the flat pixel index and is the 1 x 1 x 8197 view's"""
    ids, label, view, n_ids = R.walk_case()
    shape = (1, 7, 1171)
    assert ids.size == R.WALK_PIXELS == 7 * 1171 == 2 * R.TRIP_PIXELS * 2 + 5
    got = _raw(ids, label, view, shape, n_ids + 3, n_ids)
    ref = _same(got, ids, n_ids, label.reshape(shape), view.reshape(shape), n_ids + 3)
    assert (ref[:, :3].sum(0) > 0).all() and (got[n_ids:] == SENTINEL).all(), "weighted, clipped and odd pixels; the canary rows"


@pytest.mark.parametrize("n", [2, 3])
def test_a_view_below_four_pixels_takes_the_tail_of_the_id_load_alone(n):
    """n % 4 == 2 and 3 at n < 4 (n = 1 is the `1x1x1` view of test_patterns_on_every_view_bit_for_bit): no aligned 16-byte load"""
    ids, label = np.arange(n, dtype=np.int32) % 2, np.arange(n, dtype=np.uint8) % CR.C4
    view = np.array([4095.9375, 1e30, 2.5], np.float32)[:n]
    got = _raw(ids, label, view, (1, 1, n), 5, 2)
    ref = _same(got, ids, 2, label.reshape(1, 1, n), view.reshape(1, 1, n), 5)
    assert ref[:, 0].tolist() == [n - 1, 1] and ref[:, 1].tolist() == [0, 1]
