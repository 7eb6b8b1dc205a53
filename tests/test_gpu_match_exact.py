"""libubresnet_match.so on the device against the numpy reference of tests/match_ref.py: profile, candidate table, pair table,
ncand and status, whole buffers bit for bit, the buffers prefilled so that a missing clear or a store outside the contract shows.
The id maps and cluster tables come from real EventClusterer runs on hand-made segment maps (tests/match_ref.segments), whose
number of clusters per plane and rows per plane are chosen: 0, 1, 64 and 65 candidates; a tile that mixes planes, a tile of one
plane and a tile whose time hulls do not meet; more candidates than slots; min_pixels at a boundary; time_bin 1 and 4; a row_shift
that pushes pixels out at both ends; clamped, NaN and negative ADC; a full-width lit bin at the largest weight; a captured graph
with ubi_label and ubi_tabulate; a SparseEvent; the refusals of the Python class.  Shapes: P 2, 3, 4; rows 5, 37, 130 (two whole
chunks of 64 bins and a ragged one); cols 12, 13 (a pixel count that is no multiple of four) and 260."""
import numpy as np
import pytest
import torch

import cluster_ref as CR
import match_ref as R
import moment_ref as MR

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import clusters, planes, sparse
    from ubresnet_amd import _match as U

SCALE = 16
GARBAGE = 0x5A5A5A5A


def _clusterer(label, capacity=4096):
    P, rows, cols = label.shape
    return clusters.EventClusterer(P, rows, cols, CR.C4, 8, False, CR.FILL, capacity, "cuda:0")


def _conf(shape):
    return torch.from_numpy(CR.confidence_bits(shape).view(np.float16)).cuda()


def _run(label, view, min_pixels=3, time_bin=1, row_shift=None, slots=64, capacity=4096):
    """one eager call on a fresh clusterer and matcher -> (dict of the whole buffers on the host, the reference, Matches, matcher)"""
    cl = _clusterer(label, capacity)
    found = cl(torch.from_numpy(label).cuda(), _conf(label.shape))
    pm = planes.PlaneMatcher(cl, slots, min_pixels, time_bin, row_shift, SCALE)
    pm.profile.fill_(GARBAGE), pm.candidates.fill_(GARBAGE), pm.pairs.fill_(R.SENTINEL), pm.ncand.fill_(GARBAGE), pm.scratch.fill_(-1)
    m = pm(found, torch.from_numpy(view).cuda())
    torch.cuda.synchronize()
    got = _buffers(m)
    ref = R.match(found.ids.cpu().numpy(), found.table.cpu().numpy(), int(found.count.item()), capacity, view, SCALE, min_pixels, time_bin,
                  row_shift or (0,) * label.shape[0], slots)
    return got, ref, m, pm


def _buffers(m):
    return dict(profile=m.profile.cpu().numpy().view(np.uint32), candidates=m.candidates.cpu().numpy(), pairs=m.pairs.cpu().numpy(),
                ncand=int(m.ncand.item()), status=m.status.cpu().tolist())


def _same(got, ref):
    assert got["ncand"] == ref["ncand"] and got["status"] == ref["status"], (got["ncand"], got["status"], ref["ncand"], ref["status"])
    for name in ("candidates", "profile", "pairs"):
        assert got[name].shape == ref[name].shape and got[name].dtype == ref[name].dtype
        bad = np.argwhere(got[name] != ref[name])
        assert bad.size == 0, "%s: first difference at %s: %s against %s" % (name, bad[0].tolist(), got[name][tuple(bad[0])], ref[name][tuple(bad[0])])


def _adc(label, seed=5):
    return MR.adc(label.shape, seed, lit=label != CR.FILL)


def test_geometry_is_the_reference_geometry():
    assert (U.TILE, U.CHUNK_BINS, U.CAND_COLUMNS, U.PAIR_COLUMNS, U.CLUSTER_FIXED, U.MIN_SLOTS, U.MAX_SLOTS, U.MAX_TIME_BIN, U.MAX_SHIFT, U.MAX_WEIGHT,
            U.CAND_NAMES, U.PAIR_NAMES) == (R.TILE, R.CHUNK_BINS, R.CAND_COLUMNS, R.PAIR_COLUMNS, R.CLUSTER_FIXED, R.MIN_SLOTS, R.MAX_SLOTS,
                                            R.MAX_TIME_BIN, R.MAX_SHIFT, R.MAX_WEIGHT, R.CAND_NAMES, R.PAIR_NAMES)


@pytest.mark.parametrize("time_bin", [1, 4])
@pytest.mark.parametrize("shape", [(2, 5, 12), (3, 37, 260), (4, 130, 12), (3, 5, 13), (2, 130, 260)], ids=lambda s: "x".join(map(str, s)))
def test_every_shape_bit_for_bit(shape, time_bin):
    P, rows, cols = shape
    per_plane = min(64 // P, (rows + 1) // 2 * (1 + (cols - 6) // R.SEGMENT_PITCH))
    label = R.segments(shape, [per_plane] * P, seed=sum(shape))
    got, ref, _, _ = _run(label, _adc(label), 3, time_bin, None, 64)
    _same(got, ref)
    assert 0 < ref["ncand"] <= 64 and (ref["pairs"][:ref["n"], :ref["n"], 0] > 0).any(), "the case has pairs that share bins"
    if shape == (3, 5, 13):
        assert label.size % 4 == 3
    if shape == (4, 130, 12) and time_bin == 1:
        assert ref["candidates"][:ref["n"], 5].max() >= 128, "a candidate in the ragged third chunk"


@pytest.mark.parametrize("count", [0, 1, 64, 65])
def test_zero_one_64_and_65_candidates(count):
    shape = (2, 37, 260)
    first = min(count, 40)
    label = R.segments(shape, [first, count - first], seed=count)
    got, ref, m, _ = _run(label, _adc(label), 3, 1, None, 128)
    _same(got, ref)
    assert ref["ncand"] == count
    if count == 65:
        planes_ = ref["candidates"][:65, 1]
        assert planes_[0] == 0 and planes_[63] == 1 and planes_[64] == 1, "tile (0, 0) mixes the planes; tile (0, 1) holds candidate 64 alone"
        assert (ref["pairs"][:40, 64, 0] > 0).any()
    tab = m.read()
    assert len(tab) == count and tab.cluster.tolist() == ref["candidates"][:count, 0].tolist()
    assert m.profiles().numpy().tolist() == ref["profile"][:count].astype(np.int64).tolist()


def test_tiles_skipped_by_plane_and_by_time_hull_hold_zeros():
    """64 candidates per plane: tiles (0, 0) and (1, 1) lie in one plane each; plane 0 keeps to rows 0..16 and plane 1 to rows
    20..36, so the hulls of tile (0, 1) do not meet.  Then the same with plane 1 in rows 10..30: tile (0, 1) has work."""
    shape = (2, 37, 260)
    for rows_1, meets in (((20, 37), False), ((10, 31), True)):
        label = R.segments(shape, [64, 64], seed=3, row_ranges=[(0, 17), rows_1])
        got, ref, _, _ = _run(label, _adc(label), 3, 1, None, 128)
        _same(got, ref)
        assert ref["ncand"] == 128 and (ref["candidates"][:64, 1] == 0).all() and (ref["candidates"][64:, 1] == 1).all()
        upper = np.triu(np.ones((64, 64), bool), 1)
        assert (got["pairs"][:64, :64][upper] == 0).all() and (got["pairs"][64:, 64:][upper] == 0).all(), "one plane: zeros"
        assert (got["pairs"][:64, :64][~upper] == R.SENTINEL).all(), "i >= j is not touched"
        assert (got["pairs"][:64, 64:] != 0).any() == meets


def test_more_candidates_than_slots():
    label = R.segments((3, 37, 260), [30, 30, 30], seed=8)
    got, ref, m, _ = _run(label, _adc(label), 3, 1, None, 64)
    _same(got, ref)
    assert ref["ncand"] == 90 and ref["status"][0] == 26 and ref["n"] == 64
    with pytest.raises(OverflowError, match=r"90 candidates, slots=64"):
        m.read()
    with pytest.raises(OverflowError, match="slots"):
        m.profiles()


def test_min_pixels_at_the_boundary():
    label = R.segments((2, 37, 260), [30, 30], seed=11)               # segments of 2..6 pixels
    sizes = None
    for min_pixels in (4, 5):
        got, ref, _, _ = _run(label, _adc(label), min_pixels, 1, None, 64)
        _same(got, ref)
        sizes = sizes or ref["ncand"]
    assert 0 < ref["ncand"] < sizes, "clusters of exactly four pixels are candidates at 4 and not at 5"


def test_a_row_shift_that_pushes_pixels_out_at_both_ends():
    label = R.segments((3, 37, 260), [20, 20, 20], seed=13)
    got, ref, m, _ = _run(label, _adc(label), 3, 4, (-9, 0, 11), 64)
    _same(got, ref)
    assert ref["status"][1] > 0 and (ref["candidates"][:ref["n"], 3] == 0).any(), "a candidate lost every pixel: its hull is empty"
    lost = ref["candidates"][:ref["n"], 3] == 0
    assert (ref["candidates"][:ref["n"]][lost][:, 4:6] == [-(-37 // 4), -1]).all()
    assert m.read().dropped == ref["status"][1]


def test_a_full_width_bin_at_the_largest_weight_fills_32_bits():
    """time_bin * cols = 65536 pixels of +inf ADC in one bin: 65536 * 65535 = 2^32 - 65536, the most the plan admits"""
    shape = (2, 16, 4096)
    label = np.full(shape, CR.FILL, np.uint8)
    label[0], label[1, 3:9] = 1, 2
    view = np.full(shape, np.inf, np.float32)
    got, ref, _, _ = _run(label, view, 1, 16, None, 64)
    _same(got, ref)
    assert ref["ncand"] == 2 and ref["profile"][0, 0] == 65536 * 65535 == 2 ** 32 - 65536
    assert ref["pairs"][0, 1].tolist() == [1, 6 * 4096 * 65535, 65536 * 65535, 6 * 4096 * 65535]


def test_a_captured_graph_with_label_and_tabulate_replays_the_same_bytes():
    shape = (3, 37, 260)
    l1, l2 = R.segments(shape, [25, 20, 15], seed=21), R.segments(shape, [10, 30, 20], seed=22)
    v1, v2 = _adc(l1, 3), _adc(l2, 4)
    eager = [_run(l, v, 3, 1, (0, 1, -1), 64)[0] for l, v in ((l1, v1), (l2, v2))]
    cl = _clusterer(l1)
    pm = planes.PlaneMatcher(cl, 64, 3, 1, (0, 1, -1), SCALE)
    label, conf, view = torch.from_numpy(l1).cuda(), _conf(shape), torch.from_numpy(v1).cuda()
    pm(cl(label, conf), view)                                        # warm-up outside the capture (module load)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m = pm(cl(label, conf), view)
    torch.cuda.synchronize()
    seen = []
    for l, v, want in ((l2, v2, eager[1]), (l1, v1, eager[0]), (l1, v1, eager[0])):
        label.copy_(torch.from_numpy(l)), view.copy_(torch.from_numpy(v))
        pm.pairs.fill_(R.SENTINEL), pm.status.zero_(), pm.profile.fill_(GARBAGE)
        graph.replay()
        torch.cuda.synchronize()
        got = _buffers(m)
        for name in ("profile", "candidates", "pairs"):
            assert got[name].tobytes() == want[name].tobytes(), name
        assert (got["ncand"], got["status"]) == (want["ncand"], want["status"])
        seen.append(b"".join(got[n].tobytes() for n in ("profile", "candidates", "pairs")))
    assert seen[1] == seen[2] != seen[0]


def test_a_sparse_event_gives_the_bytes_of_its_dense_view():
    label = R.segments((3, 37, 260), [20, 20, 20], seed=31)
    view = np.where(label != CR.FILL, _adc(label), np.float32(0)).astype(np.float32)
    view[np.isnan(view)] = 7.5
    dense, _, _, _ = _run(label, view, 3, 1, None, 64)
    cl = _clusterer(label)
    found = cl(torch.from_numpy(label).cuda(), _conf(label.shape))
    pm = planes.PlaneMatcher(cl, 64, 3, 1, None, SCALE)
    pm.pairs.fill_(R.SENTINEL)
    got = _buffers(pm(found, sparse.SparseEvent.from_dense(torch.from_numpy(view))))
    for name in ("profile", "candidates", "pairs"):
        assert got[name].tobytes() == dense[name].tobytes(), name


def test_the_refusals_of_the_python_class():
    label = R.segments((2, 5, 12), [2, 2], seed=1)
    cl = _clusterer(label)
    found = cl(torch.from_numpy(label).cuda(), _conf(label.shape))
    pm = planes.PlaneMatcher(cl, 64, 3)
    view = torch.zeros((2, 5, 12), device="cuda")
    other = _clusterer(label)
    with pytest.raises(ValueError, match="not the buffers of the clusterer"):
        pm(other(torch.from_numpy(label).cuda(), _conf(label.shape)), view)
    with pytest.raises(TypeError, match="must be the Clusters"):
        pm(found.ids, view)
    with pytest.raises(ValueError, match="expected a view of"):
        pm(found, view[:, :4])
    with pytest.raises(TypeError, match="float32"):
        pm(found, view.double())
    with pytest.raises(RuntimeError):
        pm(found, view.cpu())
    with pytest.raises(TypeError, match="torch tensor or a sparse.SparseEvent"):
        pm(found, None)
    one = clusters.EventClusterer(1, 5, 12, CR.C4, 8, False, CR.FILL, 16, "cuda:0")
    with pytest.raises(ValueError, match="needs 2..4 planes"):
        planes.PlaneMatcher(one)
    for kw in (dict(slots=96), dict(slots=32), dict(slots=8192), dict(min_pixels=0), dict(time_bin=3), dict(time_bin=128), dict(row_shift=(0,)),
               dict(row_shift=(0, 5000)), dict(adc_scale=3)):
        with pytest.raises(ValueError):
            planes.PlaneMatcher(cl, **kw)
    assert pm(found, view.reshape(2, 1, 5, 12)).read().dropped == 0
