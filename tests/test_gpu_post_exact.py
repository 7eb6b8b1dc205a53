"""ubp_stitch_products (libubresnet_post.so) on synthetic buffers, bit for bit against the numpy reference of tests/post_ref.py.
No network runs here.  CASES is the module's table -- post_ref.KERNEL_CASES, one entry per compiled kernel --
and tests/test_cpu_post.py holds it against the library's symbol table and against the case ids below."""
import ctypes as C

import numpy as np
import pytest
import torch

import post_ref as R

pytestmark = pytest.mark.gpu

CASES = R.KERNEL_CASES
THR = 10.0

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _post as PL
    from ubresnet_amd import deploy


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(logp, Cn, th, tw, desc, adc, vplanes, thr, label, conf, counts, fill, P, rows, cols):
    """one ubp_stitch_products call on device tensors; -> return code"""
    flat = [v for t in desc for v in t]
    d = (C.c_int32 * max(len(flat), 1))(*flat)
    return PL.lib().ubp_stitch_products(L.ptr(logp), Cn, th, tw, d, len(desc), L.ptr(adc), vplanes, thr, L.ptr(label), L.ptr(conf),
                                        L.ptr(counts), fill, P, rows, cols, L.stream_ptr())


def _run(what, logp, desc, adc, vplanes, P, rows, cols, counts0, fill=255, launches=1, label0=0xA5, conf0=0x7B7B, thr=THR,
         exception=True):
    """run the descriptors in `launches` calls of equal size, compare every byte of the outputs with the reference; `what` is
    the case's id in CASES"""
    assert any(what in ids for ids in CASES.values()), "case %r is not in the table" % what
    nt, Cn, th, tw = logp.shape
    lab0 = np.full((P, rows, cols), label0, np.uint8)
    cf0 = np.full((P, rows, cols), conf0, np.uint16)
    ref = R.reference(logp, Cn, th, tw, desc, adc, vplanes, thr, lab0, cf0, counts0, fill, P, rows, cols)
    dl, da = _dev(logp), _dev(adc)
    lab, cf = _dev(lab0), _dev(cf0.view(np.int16))
    cnt = _dev(counts0)
    per = nt // launches
    assert per * launches == nt
    for i in range(0, nt, per):
        rc = _call(dl[i:i + per], Cn, th, tw, desc[i:i + per], da, vplanes, thr, lab, cf, cnt, fill, P, rows, cols)
        assert rc == 0, PL.lib().ubp_last_error().decode()
    torch.cuda.synchronize()
    share = R.accept(lab.cpu().numpy(), cf.cpu().numpy().view(np.uint16), None if cnt is None else cnt.cpu().numpy(), ref, what,
                     exception=exception)
    print("%s: %d lit pixels of %d written, near-tie share %.3f %%" % (what, int(ref["lit"].sum()),
                                                                        int((ref["label"] != label0).sum()), 100 * share))
    return ref


@pytest.mark.parametrize(("case", "Cn"), [("ragged-C3", 3), ("ragged-C4", 4)], ids=["ragged-C3", "ragged-C4"])
def test_ragged_regular_tiling(case, Cn):
    P, rows, cols, th, tw = 2, 45, 83, 32, 64
    desc = R.regular_desc(P, [0, 13], [0, 19], th, tw, rows, cols, deploy._keep_windows)
    assert len(desc) == 8
    rs = np.random.RandomState(100 + Cn)
    logp = R.logsoftmax_scores(rs, len(desc), Cn, th, tw)
    adc = R.adc_view(rs, P, rows, cols, THR)
    counts0 = rs.randint(1, 1000, (P, Cn)).astype(np.int64)
    ref = _run(case, logp, desc, adc, 1, P, rows, cols, counts0, launches=2)
    assert (ref["label"] != 0xA5).all(), "the tiling covers the view"
    assert 0.4 < ref["lit"].mean() < 0.6


def test_hand_built_descriptors_leave_every_other_byte_alone():
    """one keep window runs past the right and bottom edges of the view, the strip of columns 20..23 is kept by no tile, plane 1
    of 3 is touched by no tile: bytes outside the kept, in-view pixels and the counts of plane 1 keep their prefill"""
    P, rows, cols, th, tw, Cn = 3, 40, 50, 32, 32, 4
    desc = [(0, 0, 0, 0, 32, 0, 20),        # rows 0..31, cols 0..19
            (0, 16, 24, 2, 32, 0, 32),      # rows 18..47 -> 18..39, cols 24..55 -> 24..49: past both edges
            (2, 8, 18, 1, 9, 6, 30)]        # plane 2: rows 9..16, cols 24..47
    rs = np.random.RandomState(7)
    logp = R.logsoftmax_scores(rs, len(desc), Cn, th, tw)
    adc = R.adc_view(rs, P, rows, cols, THR)
    counts0 = rs.randint(1, 1000, (P, Cn)).astype(np.int64)
    ref = _run("hand-built", logp, desc, adc, 1, P, rows, cols, counts0, fill=200)
    untouched = np.ones((P, rows, cols), bool)
    untouched[0, 0:32, 0:20] = False
    untouched[0, 18:40, 24:50] = False
    untouched[2, 9:17, 24:48] = False
    assert (ref["label"][untouched] == 0xA5).all() and (ref["conf"][untouched] == 0x7B7B).all()
    assert not (ref["label"][~untouched] == 0xA5).any()
    assert np.array_equal(ref["counts"][1], counts0[1]) and not np.array_equal(ref["counts"][0], counts0[0])


def test_stacked_planes_lit_by_any():
    """P = 1, vplanes = 3: every lit pixel is lit by exactly one of the three planes"""
    rows, cols, th, tw, Cn = 30, 70, 32, 64, 4
    desc = R.regular_desc(1, [0], [0, 6], th, tw, rows, cols, deploy._keep_windows)
    rs = np.random.RandomState(11)
    logp = R.logsoftmax_scores(rs, len(desc), Cn, th, tw)
    which = rs.randint(0, 6, (rows, cols))                   # 0..2: that plane is above threshold; 3..5: none
    adc = rs.uniform(0.0, THR, (3, rows, cols)).astype(np.float32)
    for v in range(3):
        adc[v][which == v] = np.float32(THR + 1.0 + v)
    adc[0][which == 5] = np.float32(np.nan)
    ref = _run("stacked", logp, desc, adc, 3, 1, rows, cols, np.zeros((1, Cn), np.int64))
    assert np.array_equal(ref["lit"][0], which < 3)


def test_adc_null_lights_everything():
    P, rows, cols, th, tw, Cn = 2, 45, 83, 32, 64, 3
    desc = R.regular_desc(P, [0, 13], [0, 19], th, tw, rows, cols, deploy._keep_windows)
    logp = R.logsoftmax_scores(np.random.RandomState(21), len(desc), Cn, th, tw)
    ref = _run("adc-null", logp, desc, None, 1, P, rows, cols, np.zeros((P, Cn), np.int64))
    assert ref["lit"].all() and int(ref["counts"].sum()) == P * rows * cols


def test_counts_null():
    P, rows, cols, th, tw, Cn = 1, 33, 64, 32, 64, 4
    desc = R.regular_desc(P, [0, 1], [0], th, tw, rows, cols, deploy._keep_windows)
    rs = np.random.RandomState(22)
    logp = R.logsoftmax_scores(rs, len(desc), Cn, th, tw)
    _run("counts-null", logp, desc, R.adc_view(rs, P, rows, cols, THR), 1, P, rows, cols, None)


def test_view_shorter_than_the_tile():
    P, rows, cols, th, tw, Cn = 2, 20, 100, 32, 64, 4
    desc = R.regular_desc(P, [0], [0, 36], th, tw, rows, cols, deploy._keep_windows)
    assert all(d[4] == 20 for d in desc)
    desc = [d[:4] + (th,) + d[5:] for d in desc]             # the keep window as a caller that does not clip would pass it
    rs = np.random.RandomState(23)
    logp = R.logsoftmax_scores(rs, len(desc), Cn, th, tw)
    ref = _run("short-view", logp, desc, R.adc_view(rs, P, rows, cols, THR), 1, P, rows, cols, rs.randint(1, 9, (P, Cn)).astype(np.int64))
    assert (ref["label"] != 0xA5).all()


def test_edge_values_bit_for_bit():
    rows, cols, Cn = 8, 16, 4
    logp = np.empty((1, Cn, rows, cols), np.float32)
    logp[0] = np.array(R.EDGE_FILLER, np.float32)[:, None, None]
    where = {}
    for i, (name, s, lab, bits) in enumerate(R.EDGE_ROWS):
        y, x = (3 * i) // cols + 1, (3 * i) % cols
        logp[0, :, y, x] = np.array(s, np.float32)
        where[name] = (y, x, lab, bits)
    ref = _run("edge-values", logp, [(0, 0, 0, 0, rows, 0, cols)], None, 1, 1, rows, cols, np.zeros((1, Cn), np.int64), exception=False)
    for name, (y, x, lab, bits) in where.items():           # the reference itself against the hand-computed bits
        assert ref["label"][0, y, x] == lab, name
        if bits is None:
            assert R._is_nan16(ref["conf"][0, y, x]), name
        else:
            assert ref["conf"][0, y, x] == bits, name


_GOOD = dict(Cn=4, ntiles=2, desc=[(0, 0, 0, 0, 32, 0, 64), (1, 4, 8, 0, 32, 0, 64)], fill=255, alloc=2)
_BAD = {
    "ntiles 0": dict(ntiles=0, desc=[]),
    "ntiles 65": dict(ntiles=65, desc=[(0, 0, 0, 0, 32, 0, 64)] * 65, alloc=65),
    "origin outside the view": dict(desc=[(0, 0, 0, 0, 32, 0, 64), (1, 40, 8, 0, 32, 0, 64)]),
    "plane outside the view": dict(desc=[(0, 0, 0, 0, 32, 0, 64), (2, 4, 8, 0, 32, 0, 64)]),
    "keep window outside the tile": dict(desc=[(0, 0, 0, 0, 33, 0, 64), (1, 4, 8, 0, 32, 0, 64)]),
    "C 17": dict(Cn=17),
    "fill_label 256": dict(fill=256),
    "vplanes 0": dict(vplanes=0),
}


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_errors_launch_nothing(name):
    a = dict(_GOOD, vplanes=1)
    a.update(_BAD[name])
    P, rows, cols, th, tw = 2, 40, 80, 32, 64
    logp = torch.zeros((a["alloc"], 17, th, tw), device="cuda")
    adc = torch.full((P, rows, cols), 50.0, device="cuda")
    lab = torch.full((P, rows, cols), 0xA5, dtype=torch.uint8, device="cuda")
    cf = torch.full((P, rows, cols), 0x7B7B, dtype=torch.int16, device="cuda")
    cnt = torch.full((P, 17), 5, dtype=torch.int64, device="cuda")
    rc = _call(logp, a["Cn"], th, tw, a["desc"], adc, a["vplanes"], THR, lab, cf, cnt, a["fill"], P, rows, cols)
    msg = PL.lib().ubp_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and msg.startswith("ubp_stitch_products"), (rc, msg)
    assert bool((lab == 0xA5).all()) and bool((cf == 0x7B7B).all()) and bool((cnt == 5).all())
    with pytest.raises(RuntimeError, match="ubp_stitch_products"):
        PL.check(rc, name)
