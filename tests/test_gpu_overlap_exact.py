"""libubresnet_overlap.so on the device against the numpy reference of tests/overlap_ref.py: the whole table buffer, bit for bit,
prefilled with a sentinel.  The id maps come from real EventClusterer runs on the labels of tests/overlap_ref.clustered_cases():
every pattern on every view of tests/cluster_ref.py with a 8-connected and b 4-connected by class, with and without a view; a map
against itself; `checker` and `random-41` 4-connected, where nearly every lit pixel is a pair of its own, so that a workgroup meets
far more pairs than its LDS table holds (the direct path and the flush of a full table); the contended case (all lit over many
workgroups); a ragged view of several trips per workgroup.  Then: one and both maps without a cluster; raw maps no clusterer made;
capacity below the count; a table of 64 slots against thousands of pairs (the bounded refusal); two calls and two streams; a
captured graph; one hand-made case across every branch of the pixel walk shared with ClusterMoments; views below four pixels.
tests/test_cpu_overlap.py shows that no insertion order can drop a pair in any case but the 64-slot one, so a
nonzero status[0] here is a bug."""
import numpy as np
import pytest
import torch

import cluster_ref as CR
import moment_ref as MR
import overlap_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import clusters, overlap
    from ubresnet_amd import _overlap as H

SENTINEL = -0x0123456789ABCDEF
SCALE = 16
CASES = R.clustered_cases()
_IDS = {}


def _ids(label, mode):
    """the ids map of a real EventClusterer run, on the device (a clone: the clusterer's buffer goes with the clusterer)"""
    P, rows, cols = label.shape
    cl = clusters.EventClusterer(P, rows, cols, CR.C4, mode[0], mode[1], CR.FILL, 16, "cuda:0")
    conf = torch.from_numpy(CR.confidence_bits(label.shape).view(np.float16)).cuda()
    return cl(torch.from_numpy(label).cuda(), conf).ids.clone()


def _case_ids(name):
    if name not in _IDS:
        label, mode_a, mode_b, _ = CASES[name]
        _IDS[name] = (_ids(label, mode_a), _ids(label, mode_b))
    return _IDS[name]


def _run(a, b, view=None, capacity=None, slots=None, co=None, prefill=SENTINEL):
    """-> (the whole table buffer, count, status [2], the Overlap, the ClusterOverlap) after one call on device maps a, b"""
    P, rows, cols = a.shape
    co = co or overlap.ClusterOverlap(P, rows, cols, capacity or a.numel(), slots, SCALE, "cuda:0")
    if prefill is not None:
        co.table.fill_(prefill)
    ov = co(a, b, view if not isinstance(view, np.ndarray) else torch.from_numpy(view).cuda())
    torch.cuda.synchronize()
    return ov.table.cpu().numpy(), int(ov.count.item()), ov.status.cpu().tolist(), ov, co


def _same(got, count, status, a, b, view, capacity):
    """the rows below min(count, capacity) equal the reference; the rows at or past it still hold the sentinel; nothing dropped"""
    ref = R.table(a.cpu().numpy(), b.cpu().numpy(), view, SCALE)
    n = min(len(ref), capacity)
    assert status == [0, 0], "pixels found no slot although no insertion order can drop a pair of this case"
    assert count == len(ref), "count %d, the reference has %d pairs" % (count, len(ref))
    assert got.dtype == np.int64 and got.shape == (capacity, R.COLUMNS)
    bad = np.argwhere(got[:n] != ref[:n])
    assert bad.size == 0, "first difference at row, column %s: %s against %s" % (bad[0].tolist(), got[bad[0][0]].tolist(), ref[bad[0][0]].tolist())
    assert (got[n:] == SENTINEL).all(), "a row at or past min(count, capacity) was touched"
    return ref


def _adc(shape, a, b):
    return MR.adc(shape, lit=((a >= 0) | (b >= 0)).cpu().numpy())


def test_geometry_is_the_reference_geometry():
    assert (H.COLUMNS, H.MAX_PROBES, H.MIN_SLOTS, H.TRIP_PIXELS, H.LDS_SLOTS, H.MAX_WEIGHT, H.COLUMN_NAMES) == \
        (R.COLUMNS, R.MAX_PROBES, R.MIN_SLOTS, R.TRIP_PIXELS, R.LDS_SLOTS, R.MAX_WEIGHT, R.COLUMN_NAMES)
    for capacity in (1, 511, 512, 513, 131072, 17822):
        assert H.default_slots(capacity) == R.default_slots(capacity)


@pytest.mark.parametrize("with_view", [False, True], ids=["no-view", "view"])
@pytest.mark.parametrize("view", sorted(CR.VIEWS))
@pytest.mark.parametrize("pattern", sorted(CR.PATTERNS))
def test_patterns_on_every_view_bit_for_bit(pattern, view, with_view):
    name = "%s/%s" % (pattern, view)
    label, _, _, capacity = CASES[name]
    a, b = _case_ids(name)
    adc = _adc(label.shape, a, b) if with_view else None
    got, count, status, _, _ = _run(a, b, adc, capacity)
    ref = _same(got, count, status, a, b, adc, capacity)
    if not with_view:
        assert (ref[:, 4:] == 0).all()
    # b refines a, and both cover the same lit pixels: no pair has a none side, and every b lies in one a
    assert (ref[:, :2] >= 0).all() and len(set(ref[:, 1].tolist())) == len(ref)


def test_a_map_against_itself():
    label, _, _, capacity = CASES["self"]
    a, _ = _case_ids("self")
    adc = _adc(label.shape, a, a)
    got, count, status, ov, _ = _run(a, a.clone(), adc, capacity)
    ref = _same(got, count, status, a, a, adc, capacity)
    assert count > 100 and (ref[:, 0] == ref[:, 1]).all() and ref[:, 0].tolist() == list(range(count)), "numbered by first pixel, as the clusters are"
    tab = ov.read()
    assert tab.purity().value.tolist() == [1.0] * count and tab.efficiency().best.tolist() == list(range(count)) and tab.ari() == 1.0
    assert len(tab.matched(1.0, 1.0)) == count and tab.unmatched_a() == [] and tab.unmatched_b() == []


def test_one_map_without_a_cluster_gives_only_none_pairs():
    label, _, _, capacity = CASES["self"]
    a, _ = _case_ids("self")
    none = torch.full_like(a, -1)
    adc = _adc(label.shape, a, none)
    got, count, status, ov, _ = _run(a, none, adc, capacity)
    ref = _same(got, count, status, a, none, adc, capacity)
    assert (ref[:, 1] == -1).all() and ref[:, 0].tolist() == list(range(count))
    got, count, status, _, _ = _run(torch.full_like(a, -5), a, adc, capacity)
    ref = _same(got, count, status, none, a, adc, capacity)
    assert (ref[:, 0] == -1).all()
    tab = ov.read()
    assert tab.purity().value.tolist() == [0.0] * len(tab) and tab.purity().best.tolist() == [-1] * len(tab) and tab.sizes_b() == {}


def test_both_maps_without_a_cluster_touch_no_row():
    none = torch.full(CR.VIEWS["four-tiles"], -1, dtype=torch.int32, device="cuda")
    got, count, status, ov, _ = _run(none, none - 3, MR.adc(tuple(none.shape)), 9)
    assert count == 0 and status == [0, 0] and (got == SENTINEL).all()
    assert len(ov.read()) == 0 and np.isnan(ov.read().ari())


@pytest.mark.parametrize("pattern", ["checker", "random-41"])
def test_far_more_pairs_than_lds_slots_take_the_direct_path_and_the_full_table_flush(pattern):
    name = "direct/" + pattern
    label, _, _, capacity = CASES[name]
    a, b = _case_ids(name)
    key = R.keys_of(a.cpu().numpy(), b.cpu().numpy())
    per_trip = [len(np.unique(t[t != 0])) for t in np.array_split(key, range(R.TRIP_PIXELS, key.size, R.TRIP_PIXELS))]
    assert min(per_trip[:-1]) > 2 * R.LDS_SLOTS, "every full trip meets more than twice the pairs the LDS table holds"
    adc = _adc(label.shape, a, b)
    got, count, status, _, _ = _run(a, b, adc, capacity)
    _same(got, count, status, a, b, adc, capacity)


def test_all_lit_over_many_workgroups_is_the_contended_case():
    label, _, _, capacity = CASES["all-lit-contended"]
    a, b = _case_ids("all-lit-contended")
    adc = MR.adc(label.shape, seed=9)
    got, count, status, _, _ = _run(a, b, adc, capacity)
    assert -(-label.size // R.TRIP_PIXELS) == 59, "one pair per plane receives everything, from 59 workgroups"
    ref = _same(got, count, status, a, b, adc, capacity)
    assert count == 2 and ref[:, 3].tolist() == [200 * 300] * 2 and ref[:, 2].tolist() == [0, 200 * 300]


def test_several_trips_per_workgroup_on_a_ragged_view():
    """1 x 1201 x 1801 pixels are 1057 trips, above the grid cap: workgroups take spans of two trips, the last trip is ragged and
    the pixel count is odd (the last lane group is loaded pixel by pixel)"""
    label, _, _, capacity = CASES["ragged"]
    assert -(-label.size // R.TRIP_PIXELS) > 1024 and label.size % 4 == 1
    a, b = _case_ids("ragged")
    adc = MR.adc(label.shape, seed=13, lit=(a >= 0).cpu().numpy())
    got, count, status, _, _ = _run(a, b, adc, capacity)
    assert 1000 < count < capacity
    ref = _same(got, count, status, a, b, adc, capacity)
    assert ref[-1, 2] >= label.size - 5, "the last pixels of the view are a pair"


def test_raw_maps_that_no_clusterer_made():
    na, nb = R.raw_maps()
    a, b = torch.from_numpy(na).cuda(), torch.from_numpy(nb).cuda()
    adc = MR.adc(na.shape, seed=21)
    got, count, status, ov, _ = _run(a, b, adc, na.size)
    ref = _same(got, count, status, a, b, adc, na.size)
    assert ref[:, :2].max() == 2 ** 31 - 1 and ref[:, :2].min() == -1 and count >= 60
    assert {(2 ** 31 - 1, -1), (-1, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1), (0, 0)} <= set(map(tuple, ref[:, :2].tolist()))
    tab = ov.read()
    assert sum(tab.sizes_a().values()) == int((na >= 0).sum()) and sum(tab.sizes_b().values()) == int((nb >= 0).sum())


def test_capacity_below_the_count_keeps_the_total_and_the_rows_below_it():
    label, _, _, _ = CASES["direct/random-41"]
    a, b = _case_ids("direct/random-41")
    adc = _adc(label.shape, a, b)
    ref = R.table(a.cpu().numpy(), b.cpu().numpy(), adc, SCALE)
    for capacity in (5, len(ref) - 1, len(ref)):
        co = overlap.ClusterOverlap(label.shape[0], label.shape[1], label.shape[2], capacity + 3, R.default_slots(label.size), SCALE, "cuda:0")
        co.capacity = capacity                                   # the last three rows are canaries the library is told nothing of
        got, count, status, ov, _ = _run(a, b, adc, co=co)
        assert count == len(ref) and status == [0, 0]
        assert (got[:capacity] == ref[:capacity]).all() and (got[capacity:] == SENTINEL).all()
    assert len(ov.read()) == len(ref)
    co = overlap.ClusterOverlap(label.shape[0], label.shape[1], label.shape[2], 5, R.default_slots(label.size), SCALE, "cuda:0")
    _, count, _, ov, _ = _run(a, b, adc, co=co)
    with pytest.raises(OverflowError, match=r"%d pairs, capacity 5 \(slots=%d\)" % (len(ref), co.slots)):
        ov.read()


def test_sixty_four_slots_against_thousands_of_pairs_is_a_bounded_refusal():
    label, _, _, _ = CASES["direct/checker"]                     # every lit pixel is a pair of its own
    a, b = _case_ids("direct/checker")
    adc = _adc(label.shape, a, b)
    ref = R.table(a.cpu().numpy(), b.cpu().numpy(), adc, SCALE)
    assert len(ref) > 8000
    co = overlap.ClusterOverlap(label.shape[0], label.shape[1], label.shape[2], 4096 + 3, 64, SCALE, "cuda:0")
    co.capacity = 4096
    got, count, status, ov, _ = _run(a, b, adc, co=co)
    assert status[0] > 0 and status[1] == 0 and 0 < count <= 64
    assert (got[count:] == SENTINEL).all(), "nothing past the rows of the pairs that found a slot"
    rows = got[:count]
    assert rows[:, 3].sum() + status[0] == int(ref[:, 3].sum()), "stored and dropped pixels are all the pixels that take part"
    want = {tuple(r[:2]): r.tolist() for r in ref}
    assert all(want[tuple(r[:2])] == r.tolist() for r in rows), "a pair that found a slot is wholly in the table"
    with pytest.raises(OverflowError, match="slots=64"):
        ov.read()


def test_stored_not_added_and_status_is_added_to():
    name = "random-59/four-tiles"
    a, b = _case_ids(name)
    first, count1, _, _, co = _run(a, b, None, CASES[name][3])
    again, count2, status, _, _ = _run(b, a, None, co=co, prefill=None)          # the same buffers, the sides swapped
    assert count1 == count2 > 0, "the swapped maps have as many pairs: the rows past them still hold the first call's sentinel"
    ref = _same(again, count2, status, b, a, None, CASES[name][3])
    assert first[:count1].tobytes() != again[:count1].tobytes() and (ref[:, 0] == R.table(a.cpu().numpy(), b.cpu().numpy())[:, 1]).all()
    co.status[0] = 41
    _, _, status, ov, _ = _run(a, b, None, co=co)
    assert status == [41, 0]
    with pytest.raises(OverflowError, match="41 pixels found no slot"):
        ov.read()


def test_two_calls_and_two_streams_give_the_same_bytes():
    name = "direct/random-41"
    label, _, _, capacity = CASES[name]
    a, b = _case_ids(name)
    adc = _adc(label.shape, a, b)
    dv = torch.from_numpy(adc).cuda()
    first, count, status, _, co_a = _run(a, b, dv, capacity)
    _same(first, count, status, a, b, adc, capacity)
    again, _, _, _, _ = _run(a, b, dv, co=co_a)
    co_b = overlap.ClusterOverlap(label.shape[0], label.shape[1], label.shape[2], capacity, None, SCALE, "cuda:0")
    co_a.table.fill_(SENTINEL), co_b.table.fill_(SENTINEL)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        oa = co_a(a, b, dv)
    with torch.cuda.stream(s2):
        ob = co_b(a, b, dv)
    torch.cuda.synchronize()
    for ov in (oa, ob):
        assert ov.table.cpu().numpy().tobytes() == first.tobytes() == again.tobytes()
        assert int(ov.count.item()) == count and ov.status.tolist() == [0, 0]


def test_a_captured_graph_replayed_twice_on_changed_inputs():
    n1, n2 = "serpentine/four-tiles", "random-41/four-tiles"
    label, _, _, capacity = CASES[n1]
    (a1, b1), (a2, b2) = _case_ids(n1), _case_ids(n2)
    adc1, adc2 = MR.adc(label.shape, seed=3), MR.adc(label.shape, seed=4)
    a, b, dv = a1.clone(), b1.clone(), torch.from_numpy(adc1).cuda()
    co = overlap.ClusterOverlap(label.shape[0], label.shape[1], label.shape[2], capacity, None, SCALE, "cuda:0")
    co(a, b, dv)                                                 # warm-up outside the capture (module load)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ov = co(a, b, dv)
    torch.cuda.synchronize()
    seen = []
    for ids_a, ids_b, adc in ((a2, b2, adc2), (a1, b1, adc1), (a2, b2, adc2)):
        a.copy_(ids_a), b.copy_(ids_b), dv.copy_(torch.from_numpy(adc).cuda())
        co.table.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        got = ov.table.cpu().numpy()
        _same(got, int(ov.count.item()), ov.status.tolist(), ids_a, ids_b, adc, capacity)
        seen.append(got.tobytes())
    assert seen[0] == seen[2] != seen[1]
    eager, _, _, _, _ = _run(a2, b2, adc2, capacity)
    assert eager.tobytes() == seen[2]


def _no_drop(a, b, slots):
    """the condition of tests/test_cpu_overlap.py for a case built here: no insertion order can drop a pair"""
    keys = np.unique(R.keys_of(a, b))
    held, dropped = R.occupied(keys[keys != 0].tolist(), slots)
    assert not dropped and R.longest_run(held, slots) < R.probes(slots)


def test_one_case_across_every_branch_of_the_shared_walk():
    """moment_ref.walk_case() as a 1 x 1 x 8197 view, the pixels tests/test_gpu_moment_exact.py runs through the other library: map
    a is its id map, map b halves the ids (so a pair of b holds two of a where the wave has both) and is none on every fourth lane
    of the interleaved waves; with and without the view"""
    ids, _, view, _ = MR.walk_case()
    n = ids.size
    shape = (1, 1, n)
    assert n == MR.WALK_PIXELS == 2 * R.TRIP_PIXELS * 2 + 5
    lane, wave = (np.arange(n) // 4) % 64, np.arange(n) // 256
    other = np.where(ids >= 0, ids // 2, -1).astype(np.int32)
    other[(wave % 4 == 2) & (lane % 4 == 3)] = -1
    _no_drop(ids, other, R.default_slots(n))
    a, b = torch.from_numpy(ids.reshape(shape)).cuda(), torch.from_numpy(other.reshape(shape)).cuda()
    for adc in (view.reshape(shape), None):
        got, count, status, _, _ = _run(a, b, adc, n)
        ref = _same(got, count, status, a, b, adc, n)
        assert (ref[:, 1] == -1).any() and ref[-1, 2:4].tolist() == [n - 5, 5], "pairs with a none side; the ragged tail is a pair"


@pytest.mark.parametrize("n", [2, 3])
def test_a_view_below_four_pixels_takes_the_tail_of_the_id_load_alone(n):
    """n % 4 == 2 and 3 at n < 4 (n = 1 is the `1x1x1` view of test_patterns_on_every_view_bit_for_bit): no aligned 16-byte load"""
    na, nb = np.array([[[7, 7, -1]]], np.int32)[:, :, :n], np.array([[[-1, 3, 3]]], np.int32)[:, :, :n]
    adc = np.array([[[4095.9375, 1e30, 2.5]]], np.float32)[:, :, :n]
    _no_drop(na, nb, 64)
    a, b = torch.from_numpy(np.ascontiguousarray(na)).cuda(), torch.from_numpy(np.ascontiguousarray(nb)).cuda()
    got, count, status, _, _ = _run(a, b, np.ascontiguousarray(adc), 4, slots=64)
    ref = _same(got, count, status, a, b, adc, 4)
    assert ref[:, :4].tolist() == [[7, -1, 0, 1], [7, 3, 1, 1], [-1, 3, 2, 1]][:n]
