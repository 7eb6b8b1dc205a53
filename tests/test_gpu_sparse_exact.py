"""libubresnet_sparse.so on the device, exactly: ubz_scatter_view, ubz_compact and ubz_expand on the cases of tests/sparse_ref.py --
images of 1, B - 1, B and B + 1 pixels, of exactly S and S + 1 pixel blocks, rows of 1, 3, 61 and 67 pixels, one and three planes
and three stacked ADC planes; every occupancy and capacity of the table, the lit rule on threshold ties, NaN and the infinities,
adc == NULL; entry lists that are empty, hit the first and the last pixel, carry -0.0, subnormals, NaN payloads and infinities,
take their length from the device, and break the validity rule in every way.  Every buffer is compared WHOLE, between guard
margins and with a pattern in the bytes that must stay untouched; every comparison is np.array_equal on bits; every call runs
twice.  Round trips, and each call replayed from a captured graph with new contents in the same buffers.
tests/test_cpu_sparse.py holds the case ids against the compiled kernels."""
import numpy as np
import pytest
import torch

import sparse_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _sparse as Z

CASES = R.KERNEL_CASES
DEV = "cuda"
MARGIN = 256                                                    # bytes: the payload keeps the allocation's alignment
PATTERN = 0xA5
u8, u16, u32, i32 = np.uint8, np.uint16, np.uint32, np.int32


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
        if raw.size:
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


def _word(v):
    return Buf(8, init=np.array([v], np.uint64))


class Compact:
    """the operands of a compact case on the device, the call, and the whole-buffer comparison with the reference"""

    def __init__(self, name):
        a = self.a = R.compact_inputs(name)
        self.name = name
        P, rows, cols = a["image"]
        self.n, self.cap = P * rows * cols, a["capacity"]
        self.label, self.conf = Buf(self.n, init=a["label"]), Buf(2 * self.n, init=a["conf"])
        self.adc = None if a["adc"] is None else Buf(a["adc"].nbytes, 4 * a["offset"], init=a["adc"])
        self.sbytes = Z.compact_scratch_bytes(P, rows, cols)
        self.oi, self.ol, self.oc = Buf(4 * self.cap), Buf(self.cap), Buf(2 * self.cap)
        self.count, self.scratch = _word(0xA5A5A5A5A5A5A5A5), Buf(self.sbytes)

    def call(self):
        a = self.a
        P, rows, cols = a["image"]
        Z.compact(self.label.ptr, self.conf.ptr, None if self.adc is None else self.adc.ptr, a["vplanes"], a["thr"], P, rows, cols, self.cap,
                  self.oi.ptr, self.ol.ptr, self.oc.ptr, self.count.ptr, self.scratch.ptr, self.sbytes, L.stream_ptr())

    def outputs(self):
        return [b.host() for b in (self.oi, self.ol, self.oc, self.count)]

    def check(self, what):
        a = self.a
        P, rows, cols = a["image"]
        oi, ol, oc = np.full(self.cap, 0xA5A5A5A5, u32).view(i32), np.full(self.cap, PATTERN, u8), np.full(self.cap, 0xA5A5, u16)
        total = R.compact(a["label"], a["conf"], a["adc"], a["vplanes"], a["thr"], P, rows, cols, oi, ol, oc)
        assert total == a["total"]
        got = self.outputs()
        assert np.array_equal(got[3], self.count.expect(np.array([total], np.uint64))), "%s %s: count" % (self.name, what)
        for g, b, e, field in zip(got, (self.oi, self.ol, self.oc), (oi, ol, oc), ("out_index", "out_label", "out_confidence")):
            assert np.array_equal(g, b.expect(e)), "%s %s: %s, or the bytes around it" % (self.name, what, field)
        # the inputs are as they were, and nothing beyond the scratch was touched
        assert np.array_equal(self.label.host(), self.label.expect(a["label"])) and np.array_equal(self.conf.host(), self.conf.expect(a["conf"]))
        if self.adc is not None:
            assert np.array_equal(self.adc.host(), self.adc.expect(a["adc"]))
        s = self.scratch.host()
        assert (s[:MARGIN] == PATTERN).all() and (s[MARGIN + self.sbytes:] == PATTERN).all(), "%s %s: beyond the scratch" % (self.name, what)
        return got


class Listed:
    """the operands of a scatter or expand case on the device, the call, and the whole-buffer comparison with the reference"""

    def __init__(self, name):
        a = self.a = R.list_inputs(name)
        self.name, self.is_expand = name, R.CASES[name]["call"] == "expand"
        self.pixels = R.pixels_of(a["image"])
        self.m = len(a["index"])
        self.index = Buf(4 * self.m, init=a["index"])
        self.value, self.lab, self.conf = Buf(4 * self.m, init=a["value"]), Buf(self.m, init=a["label"]), Buf(2 * self.m, init=a["conf"])
        self.count = None if a["count"] is None else _word(a["count"])
        self.status = _word(a["status0"])
        off = a["offset"]
        self.view = Buf(4 * self.pixels, 4 * off)
        self.ol, self.oc = Buf(self.pixels, off), Buf(2 * self.pixels, 2 * off)

    def call(self):
        a = self.a
        P, rows, cols = a["image"]
        cnt = None if self.count is None else self.count.ptr
        if self.is_expand:
            Z.expand(self.index.ptr, self.lab.ptr, self.conf.ptr, self.m, cnt, a["fill_label"], self.ol.ptr, self.oc.ptr, P, rows, cols,
                     self.status.ptr, L.stream_ptr())
        else:
            Z.scatter_view(self.index.ptr, self.value.ptr, self.m, cnt, self.view.ptr, P, rows, cols, self.status.ptr, L.stream_ptr())

    def outputs(self):
        return [b.host() for b in ((self.ol, self.oc) if self.is_expand else (self.view,))] + [self.status.host()]

    def check(self, what, runs=1):
        a = self.a
        if self.is_expand:
            l, c, status, named = R.expand(a["index"], a["label"], a["conf"], a["count"], a["fill_label"], self.pixels, a["status0"])
            pairs = [(self.ol, l, named), (self.oc, c, named)]
        else:
            v, status, named = R.scatter_view(a["index"], a["value"], a["count"], self.pixels, a["status0"])
            pairs = [(self.view, v, named)]
        bad = status - a["status0"]
        got = self.outputs()
        want_status = a["status0"] + runs * bad                # added to, once per run
        assert np.array_equal(got[-1], self.status.expect(np.array([want_status], np.uint64))), "%s %s: status" % (self.name, what)
        for g, (b, e, nm) in zip(got, pairs):
            e = b.expect(e)
            if bad:                                             # the elements that entries name are unspecified, nothing else is
                free = np.zeros(e.size, bool)
                free[b.lo:b.lo + b.nbytes] = np.repeat(nm, b.nbytes // self.pixels)
                assert free.sum() < 40 * (b.nbytes // self.pixels)
                g, e = g[~free], e[~free]
            assert np.array_equal(g, e), "%s %s: an output, or the bytes around it" % (self.name, what)
        for b, src in ((self.index, a["index"]), (self.value, a["value"]), (self.lab, a["label"]), (self.conf, a["conf"])):
            assert np.array_equal(b.host(), b.expect(src)), "%s %s: an input changed" % (self.name, what)
        if self.count is not None:
            assert np.array_equal(self.count.host(), self.count.expect(np.array([a["count"]], np.uint64)))
        return got


def _run(name):
    """the case once, checked whole against the reference; then once more into the same buffers: identical bytes"""
    case = Compact(name) if R.CASES[name]["call"] == "compact" else Listed(name)
    case.call()
    torch.cuda.synchronize()
    first = case.check("first run")
    case.call()
    torch.cuda.synchronize()
    second = case.check("second run") if isinstance(case, Compact) else case.check("second run", runs=2)
    for a, b in zip(first[:-1], second[:-1]):
        assert np.array_equal(a, b), "%s: two runs differ" % name
    return case


@pytest.mark.parametrize("name", ["c-1px-lit", "c-1px-dark", "c-Bm1-checker", "c-B-random", "c-Bp1-last", "c-first", "c-all-lit", "c-all-dark",
                                  "c-null-adc", "c-per-wave", "c-stacked", "c-lit-rule", "c-unaligned", "c-S-blocks", "c-Sp1-random",
                                  "c-cap-short", "c-cap-1"])
def test_compact(name):
    case = _run(name)
    total = int(case.count.payload(np.uint64)[0])
    if name == "c-cap-short":
        assert total == case.cap + 1, "the count is the total, the list holds one entry less"
    if name in ("c-1px-dark", "c-all-dark"):
        assert total == 0 and (case.oi.host() == PATTERN).all(), "nothing is lit and nothing was written"
    if name == "c-cap-1":
        assert total > 1 and case.cap == 1


@pytest.mark.parametrize("name", ["s-empty", "s-ends", "s-random", "s-count-small", "s-count-large", "s-invalid", "s-stride", "s-fill-stride"])
def test_scatter_view(name):
    case = _run(name)
    if name == "s-empty":
        assert not case.view.payload(u32).any()
    if name == "s-invalid":
        assert int(case.status.payload(np.uint64)[0]) == (1 << 40) + 3 + 2 * 9


@pytest.mark.parametrize("name", ["e-empty", "e-ends", "e-random", "e-count-large", "e-invalid", "e-stride"])
def test_expand(name):
    case = _run(name)
    if name == "e-empty":
        assert (case.ol.payload(u8) == 255).all() and not case.oc.payload(u16).any()


# ------------------------------------------------------------------------------------------------------------------------
# round trips
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c-Sp1-random", "c-stacked", "c-lit-rule", "c-all-lit", "c-all-dark"])
def test_expand_of_compact_is_the_products_and_compact_of_that_is_the_list(name):
    """products whose unlit pixels hold fill_label / +0, as ubp_stitch_products leaves them: expand(compact(p)) == p on every
    byte, with the list's length taken from the device count; and compact(expand(list)) == list"""
    a = R.compact_inputs(name)
    P, rows, cols = a["image"]
    n, fill = P * rows * cols, 255
    label, conf = np.where(a["lit"], a["label"], fill).astype(u8), np.where(a["lit"], a["conf"], 0).astype(u16)
    dl, dc = Buf(n, init=label), Buf(2 * n, init=conf)
    adc = None if a["adc"] is None else Buf(a["adc"].nbytes, init=a["adc"])
    adc_ptr = None if adc is None else adc.ptr
    sbytes = Z.compact_scratch_bytes(P, rows, cols)
    oi, ol, oc, count, scratch = Buf(4 * n), Buf(n), Buf(2 * n), _word(0), Buf(sbytes)
    Z.compact(dl.ptr, dc.ptr, adc_ptr, a["vplanes"], a["thr"], P, rows, cols, n, oi.ptr, ol.ptr, oc.ptr, count.ptr, scratch.ptr, sbytes, L.stream_ptr())
    el, ec, status = Buf(n), Buf(2 * n), _word(0)
    Z.expand(oi.ptr, ol.ptr, oc.ptr, n, count.ptr, fill, el.ptr, ec.ptr, P, rows, cols, status.ptr, L.stream_ptr())
    torch.cuda.synchronize()
    assert int(count.payload(np.uint64)[0]) == a["total"] and int(status.payload(np.uint64)[0]) == 0
    assert np.array_equal(el.host(), el.expect(label)) and np.array_equal(ec.host(), ec.expect(conf))
    oi2, ol2, oc2, count2 = Buf(4 * n), Buf(n), Buf(2 * n), _word(0)
    Z.compact(el.ptr, ec.ptr, adc_ptr, a["vplanes"], a["thr"], P, rows, cols, n, oi2.ptr, ol2.ptr, oc2.ptr, count2.ptr, scratch.ptr, sbytes, L.stream_ptr())
    torch.cuda.synchronize()
    for x, y in ((oi, oi2), (ol, ol2), (oc, oc2), (count, count2)):
        assert np.array_equal(x.host(), y.host())


# ------------------------------------------------------------------------------------------------------------------------
# graph capture
# ------------------------------------------------------------------------------------------------------------------------
def _captured(case):
    """capture the case's call; the capture itself runs nothing"""
    case.call()                                                 # warm-up outside the capture (module load)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        case.call()
    torch.cuda.synchronize()
    return graph


def test_a_captured_graph_replays_compact_on_new_contents():
    """captured on one case's contents, replayed on another's in the same buffers: the three launches read everything, the count
    included, from the device"""
    case = Compact("c-Bm1-checker")
    graph = _captured(case)
    b = R.compact_inputs("c-Bm1-checker")
    rs = R.rng("replay")
    lit = rs.uniform(size=case.n) < 0.4
    b["adc"] = np.where(lit, np.float32(12.0), np.float32(-1.0)).astype(np.float32).reshape(b["adc"].shape)
    b["label"], b["conf"] = rs.randint(0, 256, case.n).astype(u8), rs.randint(0, 1 << 16, case.n).astype(u16)
    b["lit"], b["total"] = lit, int(lit.sum())
    assert 1 < b["total"] < case.cap, "the new list is shorter: the tail keeps the pattern"
    case.a = b
    case.label.set(b["label"]), case.conf.set(b["conf"]), case.adc.set(b["adc"])
    for buf in (case.oi, case.ol, case.oc):
        buf.full.fill_(PATTERN)
    graph.replay()
    torch.cuda.synchronize()
    case.check("replay")


@pytest.mark.parametrize("name", ["s-random", "e-random"])
def test_a_captured_graph_replays_scatter_and_expand_on_new_contents(name):
    case = Listed(name)
    graph = _captured(case)
    a = dict(case.a)
    rs = R.rng("replay-" + name)
    keep = np.sort(rs.choice(case.pixels, case.m, replace=False)).astype(i32)      # as many entries, at other pixels
    a["index"], a["value"] = keep, rs.randint(0, 1 << 32, case.m, dtype=np.uint64).astype(u32)
    a["label"], a["conf"] = rs.randint(0, 256, case.m).astype(u8), rs.randint(0, 1 << 16, case.m).astype(u16)
    if a["count"] is not None:
        a["count"] = case.m // 3                                # the device count changes between the capture and the replay
        case.count.set(np.array([a["count"]], np.uint64))
    a["status0"] = 11
    case.status.set(np.array([11], np.uint64))
    case.a = a
    case.index.set(a["index"]), case.value.set(a["value"]), case.lab.set(a["label"]), case.conf.set(a["conf"])
    for buf in (case.view, case.ol, case.oc):
        buf.full.fill_(PATTERN)
    graph.replay()
    torch.cuda.synchronize()
    case.check("replay")
