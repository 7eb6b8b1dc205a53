"""libubresnet_crop.so on the device, exactly: ubn_occupancy, ubn_choose and ubn_gather on the cases of tests/crop_ref.py -- the
branch case of the selection (acceptance at try 0, with exactly min_lit, at a later try; fallbacks that keep the best and the
earliest try; every flip combination), a view that is one crop, cells of 4 and of 64 pixels, views one element past 16-byte
alignment, stacked planes with one label image, the three label types with their edge values and an offset, class masks, the
lit rule on threshold ties, NaN and the infinities, one crop and 257 of them, one try and 64, the enable switches, an eligible
plane list, and a caller's own table with a row out of range in every field.  Every buffer -- table of sums, crop table, image,
label, weight, status -- is compared WHOLE, between guard margins and with a pattern in the bytes that must stay untouched; every
comparison is np.array_equal on bits; every case runs twice.  Then the three calls replayed from a captured graph on new
contents.  tests/test_cpu_crops.py holds the case ids against the compiled kernels."""
import numpy as np
import pytest
import torch

import crop_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _crop as N
    from ubresnet_amd import _lib as L

CASES = R.KERNEL_CASES
DEV = "cuda"
MARGIN = 256                                                    # bytes: the payload keeps the allocation's alignment
PATTERN = 0xA5
u8, u32, i32, i64 = np.uint8, np.uint32, np.int32, np.int64


class Buf:
    """`nbytes` bytes on the device, `offset` bytes past a 256-byte boundary, between two margins, all of it the pattern (or the
    bytes of `init`); host() is the whole allocation on the host, expect(payload) what it must be if only the payload changed"""

    def __init__(self, nbytes, offset=0, init=None):
        self.nbytes, self.lo = int(nbytes), MARGIN + offset
        self.full = torch.full((self.lo + self.nbytes + MARGIN,), PATTERN, dtype=torch.uint8, device=DEV)
        assert self.full.data_ptr() % 256 == 0
        self.ptr = self.full.data_ptr() + self.lo
        if init is not None:
            self.set(init)

    def set(self, arr):
        raw = np.ascontiguousarray(arr).view(u8).reshape(-1)
        assert raw.size == self.nbytes
        self.full[self.lo:self.lo + self.nbytes].copy_(torch.from_numpy(raw.copy()))
        return self

    def host(self):
        return self.full.cpu().numpy()

    def expect(self, payload):
        e = np.full(self.lo + self.nbytes + MARGIN, PATTERN, u8)
        e[self.lo:self.lo + self.nbytes] = np.ascontiguousarray(payload).view(u8).reshape(-1)
        return e

    def payload(self, dtype):
        return self.host()[self.lo:self.lo + self.nbytes].view(dtype)


class Case:
    """the operands of a case on the device, the calls, and the whole-buffer comparison with the reference"""

    def __init__(self, name):
        a = self.a = R.inputs(name)
        self.name, s = name, a["shift"]
        self.K, self.C = a["K"], (a["P"] if a["stacked"] else 1)
        hw = a["H"] * a["W"]
        self.image = Buf(a["image"].nbytes, 4 * s, init=a["image"])
        self.label = Buf(a["label"].nbytes, a["label"].itemsize * s, init=a["label"])
        self.weight = None if a["weight"] is None else Buf(a["weight"].nbytes, 4 * s, init=a["weight"])
        self.sat_shape = N.sat_shape(a["Q"], a["rows"], a["cols"], a["g"])
        self.sat = Buf(4 * int(np.prod(self.sat_shape)), 4 * s)
        self.table = Buf(4 * R.TABLE_FIELDS * self.K, 4 * s, init=a["table"])
        self.oi, self.ol, self.ow = Buf(4 * self.K * self.C * hw, 4 * s), Buf(8 * self.K * hw, 8 * s), Buf(4 * self.K * hw, 4 * s)
        self.status = Buf(8, init=np.array([a["status0"]], np.uint64))

    def call(self):
        a, st = self.a, L.stream_ptr()
        if not a["own"]:
            masked = a["mask"] is not None
            N.occupancy(self.image.ptr, self.label.ptr if masked else None, a["kind"] if masked else N.LABEL_NONE, a["offset"], a["mask"] or 0,
                        a["stacked"], a["thr"], a["P"], a["rows"], a["cols"], a["g"], self.sat.ptr, st)
            N.choose(self.sat.ptr, a["Q"], a["rows"], a["cols"], a["H"], a["W"], a["g"], a["planes"], self.K, a["T"], a["min_lit"], a["seed"],
                     a["number"], a["flip_rows"], a["flip_cols"], self.table.ptr, st)
        N.gather(self.image.ptr, self.label.ptr, a["kind"], a["offset"], None if self.weight is None else self.weight.ptr, a["stacked"],
                 a["P"], a["rows"], a["cols"], a["H"], a["W"], self.table.ptr, self.K, self.oi.ptr, self.ol.ptr, self.ow.ptr, self.status.ptr, st)

    def outputs(self):
        return [b.host() for b in (self.sat, self.table, self.oi, self.ol, self.ow, self.status)]

    def check(self, what, runs=1):
        a = self.a
        ref = self.ref = R.reference(a)
        got = self.outputs()
        want = [self.sat.expect(ref["sat"]) if not a["own"] else self.sat.expect(np.full(self.sat.nbytes, PATTERN, u8)),
                self.table.expect(ref["table"]), self.oi.expect(ref["image"]), self.ol.expect(ref["label"]), self.ow.expect(ref["weight"]),
                self.status.expect(np.array([a["status0"] + runs * ref["bad"]], np.uint64))]       # added to, once per run
        for g, e, field in zip(got, want, ("sat", "table", "out_image", "out_label", "out_weight", "status")):
            if not np.array_equal(g, e):
                where = np.flatnonzero(g != e)
                raise AssertionError("%s %s: %s, or the bytes around it: %d bytes differ, first at byte %d of the allocation (payload from %d)"
                                     % (self.name, what, field, where.size, where[0], MARGIN))
        # the inputs are as they were
        assert np.array_equal(self.image.host(), self.image.expect(a["image"])) and np.array_equal(self.label.host(), self.label.expect(a["label"]))
        if self.weight is not None:
            assert np.array_equal(self.weight.host(), self.weight.expect(a["weight"]))
        return got


def _run(name):
    """the case once, checked whole against the reference; then once more into the same buffers: identical bytes"""
    case = Case(name)
    case.call()
    torch.cuda.synchronize()
    first = case.check("first run")
    case.call()
    torch.cuda.synchronize()
    second = case.check("second run", runs=2)
    for x, y in zip(first[:-1], second[:-1]):
        assert np.array_equal(x, y), "%s: two runs differ" % name
    return case


def test_the_branch_case_takes_every_branch_of_the_selection():
    case = _run("branch")
    table = case.table.payload(i32).reshape(-1, 8)
    assert table[0].tolist() == [0, 0, 0, 512, 0, 1, 1, 0] and table[5].tolist() == [1, 32, 48, 1, 2, 0, 0, 0]
    other = _run("other-number")                                # the same view and seed, the next event: the reference's other table
    assert not np.array_equal(table, other.table.payload(i32).reshape(-1, 8))


@pytest.mark.parametrize("name", ["one-position", "g4-tails", "g64", "wide-scan", "unaligned", "unaligned-i64", "stacked", "stacked-f32", "no-mask-no-weight",
                                  "k1-t1", "k257", "t64", "planes-list", "seed-hi"])
def test_geometry_and_batch_sizes(name):
    case = _run(name)
    a, table = case.a, case.table.payload(i32).reshape(-1, 8)
    if name == "one-position":
        assert (table[:, 1:3] == 0).all() and a["geo"]["NR"] == a["geo"]["NC"] == 1
    if name == "g4-tails":
        assert a["g"] == 4 and (table[:, 1:3] % 4 == 0).all() and (table[:, 1:3] % 8 != 0).any()
    if name == "wide-scan":
        assert a["geo"]["CC"] == 260 > N.LANES and a["geo"]["CR"] == 2, "every wave of the row scan holds counts, and it takes a second trip"
        assert (case.sat.payload(i32).reshape(case.sat_shape)[:, 1, 1:] > 0).all()
    if name == "g64":
        assert a["g"] == 64
    if name == "k257":
        assert len(table) == 257 and table[256].any()
    if name == "planes-list":
        assert set(table[:, 0].tolist()) == {0, 2}
    if name == "t64":
        assert (table[:, 5] == 0).all() and table[:, 4].max() > 3, "a fallback found deep in the tries"
    if name.startswith("unaligned"):
        assert case.image.ptr % 16 != 0 and case.oi.ptr % 16 != 0 and case.ol.ptr % 16 == 8


@pytest.mark.parametrize("name", ["label-u8", "label-i64", "label-f32-edges", "class-mask", "lit-rule", "all-lit", "all-dark"])
def test_the_predicate(name):
    case = _run(name)
    a, ref = case.a, case.ref
    sat = case.sat.payload(i32).reshape(case.sat_shape)
    if name == "all-lit":
        assert (sat[:, -1, -1] == a["rows"] * a["cols"]).all()
    if name == "all-dark":
        assert not sat.any() and (case.table.payload(i32).reshape(-1, 8)[:, 3:6] == 0).all(), "ADC at the threshold is not lit"
    if name == "class-mask":
        L_ = R.convert_labels(a["label"], 0)
        assert {32, 255, -1, 31, 2} <= set(L_.reshape(-1).tolist())
        assert not ref["count"][np.isin(L_, [32, 255, -1, 0, 1, 3])].any() and ref["count"][(L_ == 31) & (a["image"] > 10)].all()
    if name == "label-f32-edges":
        assert R.convert_labels(R.EDGE_LABELS, -1).tolist() == R.EDGE_LABELS_MINUS_1
        assert (case.ol.payload(i64) == R.NO_LABEL).any() and (case.ol.payload(i64) == 2147483519).any()
    if name == "lit-rule":
        flat = a["image"].reshape(-1)
        assert np.isnan(flat).any() and (flat == R.THR).any() and np.isposinf(flat).any()
        assert int(sat[0, -1, -1]) == int(np.isin(flat.view(u32), np.array([np.nextafter(R.THR, np.float32(np.inf)), np.inf, 11.0, 3.0e38],
                                                                          np.float32).view(u32)).sum())


def test_the_enable_switches():
    off, on, rows_only = _run("switches-off"), _run("switches-on"), _run("rows-only")
    t_off, t_on, t_rows = (c.table.payload(i32).reshape(-1, 8) for c in (off, on, rows_only))
    assert not t_off[:, 6:].any() and t_on[:, 6].any() and t_on[:, 7].any() and len({tuple(r) for r in t_on[:, 6:].tolist()}) == 4
    assert np.array_equal(t_off[:, 0:3], t_on[:, 0:3]) and np.array_equal(t_rows[:, 6], t_on[:, 6]) and not t_rows[:, 7].any()


@pytest.mark.parametrize("name", ["own-table", "own-table-stacked"])
def test_a_callers_table_with_rows_out_of_range_in_every_field(name):
    case = _run(name)
    a, ref = case.a, case.ref
    assert ref["bad"] == 9 and int(case.status.payload(np.uint64)[0]) == a["status0"] + 2 * 9
    bad = [k for k in range(case.K) if not R.row_is_valid(a["table"][k], a["stacked"], a["P"], a["rows"], a["cols"], a["H"], a["W"])]
    assert bad == list(range(2, 11))
    oi = case.oi.payload(u32).reshape(case.K, -1)
    assert not oi[bad].any() and not case.ol.payload(i64).reshape(case.K, -1)[bad].any() and not case.ow.payload(u32).reshape(case.K, -1)[bad].any()
    assert oi[0].any() and (a["table"][:2, 1:3] % 4).any(), "in-range rows at offsets no cell divides are gathered"
    assert (case.sat.host() == PATTERN).all(), "the gather alone ran"


def test_a_captured_graph_replays_the_three_calls_on_new_contents():
    """captured on one view's contents, replayed on another's in the same buffers: the launches read everything from the device"""
    case = Case("unaligned")
    case.call()                                                 # warm-up outside the capture (module load)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        case.call()
    torch.cuda.synchronize()
    b = dict(case.a)
    rs = R.rng("replay")
    shape = b["image"].shape
    b["image"] = np.where(rs.uniform(size=shape) < 0.3, np.float32(12.0), np.float32(-1.0)).astype(np.float32)
    b["label"] = rs.randint(0, 4, b["label"].shape).astype(b["label"].dtype)
    b["weight"] = rs.uniform(0.0, 3.0, b["weight"].shape).astype(np.float32)
    case.a = b
    case.image.set(b["image"]), case.label.set(b["label"]), case.weight.set(b["weight"])
    for buf in (case.sat, case.table, case.oi, case.ol, case.ow):
        buf.full.fill_(PATTERN)
    graph.replay()
    torch.cuda.synchronize()
    replayed = case.check("replay")
    case.call()                                                 # and eagerly once more: the same bytes
    torch.cuda.synchronize()
    for x, y in zip(replayed[:-1], case.outputs()[:-1]):
        assert np.array_equal(x, y)
