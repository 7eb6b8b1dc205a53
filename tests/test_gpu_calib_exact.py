"""libubresnet_calib.so on the GPU against tests/calib_ref.py: every accumulate case of the table within the derived bound of its
sums, the counters exactly; two adds; the same call twice, bit for bit; every apply case within its bound, in place against out of
place, the probabilities' sum, the arg-max above the derived margin, and the -inf / NaN rules by bit pattern.  Between them the
cases launch every compiled kernel of the library once (tests/test_cpu_calib.py holds the table against the symbol table)."""
import numpy as np
import pytest
import torch

import calib_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _calib as F
    from ubresnet_amd import calibration as CB

CASES = R.KERNEL_CASES
_CACHE = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _accumulate(a, table=None, counters=None):
    """one ubf_accumulate call on the inputs `a` of a case -> (table, counters) device tensors, added to when given"""
    N, C, H, W = a["scores"].shape
    K = len(a["betas"])
    table = torch.zeros((a["G"], K, 3), dtype=torch.float64, device="cuda") if table is None else table
    counters = torch.zeros((a["G"], 3), dtype=torch.int64, device="cuda") if counters is None else counters
    nbytes = F.scratch_bytes(N, H, W, K)
    scratch = torch.full((nbytes // 8,), 0x7FF8DEAD, dtype=torch.int64, device="cuda")           # never cleared: the pass writes it all
    s, t, l, g, b = _dev(a["scores"]), _dev(a["truth"]), _dev(a["lit"]), _dev(a["groups"]), _dev(a["betas"])
    F.accumulate(s.data_ptr(), t.data_ptr(), F.TRUTH_I64 if a["truth"].dtype == np.int64 else F.TRUTH_U8,
                 None if l is None else l.data_ptr(), a["thr"], g.data_ptr(), b.data_ptr(), K, N, C, H, W, a["G"], table.data_ptr(),
                 counters.data_ptr(), scratch.data_ptr(), nbytes, _stream())
    torch.cuda.synchronize()
    return table, counters


def _reference(name):
    if name not in _CACHE:
        a = R.acc_inputs(name)
        _CACHE[name] = (a, R.accumulate(a["scores"], a["truth"], a["lit"], a["thr"], a["groups"], a["betas"], a["G"]))
    return _CACHE[name]


def _within(got, ref, bound, what):
    err = np.abs(got - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    print("%s: worst error / bound %.3f" % (what, float(ratio.max()) if ratio.size else 0.0))
    assert np.isfinite(got).all(), what
    if ratio.size:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        assert float(ratio.max()) <= 1.0, "%s: at %s got %r, fp64 %r, bound %.3e" % (what, i, got[i], ref[i], bound[i])


def _run(name):
    if name in R.ACC_CASES:
        a, (ref, cref, bound) = _reference(name)
        table, counters = _accumulate(a)
        assert np.array_equal(counters.cpu().numpy().view(np.uint64), cref), (name, counters.cpu().numpy(), cref)
        _within(table.cpu().numpy(), ref, bound, name)
        return a, ref, cref
    c = R.APPLY_CASES[name]
    n, C, H, W = c["shape"]
    x = _apply_input(c["shape"], sum(ord(ch) for ch in name))
    betas = np.array([0.25, 1.0, 4.0, 0.6, 1.7][:n], dtype=np.float32)
    ref, bound = R.apply(x, betas)
    flat = torch.empty(x.size + 4, dtype=torch.float32, device="cuda")
    buf = flat[c["offset"]:c["offset"] + x.size].view(n, C, H, W)
    buf.copy_(torch.from_numpy(x))
    out = torch.empty(x.size + 4, dtype=torch.float32, device="cuda")[c["offset"]:c["offset"] + x.size].view(n, C, H, W)
    b = _dev(betas)
    F.apply(buf.data_ptr(), out.data_ptr(), b.data_ptr(), n, C, H, W, _stream())
    F.apply(buf.data_ptr(), buf.data_ptr(), b.data_ptr(), n, C, H, W, _stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), buf.cpu().numpy().view(np.uint32)), "%s: in place differs from out of place" % name
    _within(got.astype(np.float64), ref, bound, name)
    # every pixel's probabilities sum to one: each exp(out_c) is off by at most its bound, relatively
    p = np.exp(ref)
    psum = np.exp(got.astype(np.float64)).sum(1)
    assert (np.abs(psum - 1.0) <= R.C_ACC * (p * bound).sum(1) + 2.0 ** -50).all(), name
    # the arg-max stays where the top-2 margin of the input is above the derived one
    if C > 1:
        top = np.sort(x.astype(np.float64), axis=1)
        gap = top[:, -1] - top[:, -2]
        need = np.array([R.margin(v) for v in betas]).reshape(n, 1, 1)
        assert (gap > need).all(), "the case was built so that no pixel falls under the margin"
        assert np.array_equal(got.argmax(1), x.argmax(1)), name
    return got


def _apply_input(shape, seed):
    """log-probabilities whose top-2 margin is at least 1e-3 (above MARGIN(0.25) = 2^-20), a fifth of the pixels 60 nat apart"""
    n, C, H, W = shape
    rs = np.random.RandomState(seed)
    z = rs.standard_normal(shape) * 2.5
    z = np.where(rs.rand(n, 1, H, W) < 0.2, z * 24.0, z)
    z = z - z.max(1, keepdims=True)
    x = (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)
    if C > 1:                                                       # push a runner-up that is too close down by 1e-2
        order = np.argsort(x, axis=1)
        second = np.take_along_axis(x, order[:, -2:-1], 1)
        close = (np.take_along_axis(x, order[:, -1:], 1) - second) < 1e-3
        np.put_along_axis(x, order[:, -2:-1], np.where(close, second - np.float32(1e-2), second), 1)
    return x


@pytest.mark.parametrize("name", ["one-pixel", "nothing-counts", "odd-width", "partial-trip", "two-workgroups", "all-lit-c1", "c1-i64",
                                  "c2-i64", "c2-u8", "c3-u8", "c4-u8", "c4-i64", "c5-u8", "c16-i64", "strided-trips"])
def test_accumulate(name):
    a, ref, cref = _run(name)
    c = R.ACC_CASES[name]
    if name == "nothing-counts":
        assert not ref.any() and not cref.any()
    elif name == "one-pixel":
        assert cref.sum() == 1
    else:
        assert cref[:, 0].sum() > 0
        if c["shape"][0] * c["shape"][2] * c["shape"][3] >= 8:
            assert cref[:, 1].sum() > 0 and cref[:, 2].sum() == 2, "ignored truths and the two non-finite scores"
    if c["lit"] == "cut":
        assert cref.sum() < a["truth"].size, "the threshold cut nothing"
    if name == "two-workgroups":
        assert not ref[1].any() and ref[0].any() and ref[2].any(), "groups (2, 0): group 1 stays empty"


def test_two_adds_and_the_python_surface():
    a, (ref1, cref1, bound1) = _reference("c4-u8")
    b = R.acc_inputs("c4-i64")                                    # another shape, int64 truth, no lit: added to the same table
    K = len(a["betas"])
    assert K == 33
    fit = CB.TemperatureFit(4, groups=1, adc_threshold=a["thr"])
    fit.add(_dev(a["scores"]), _dev(a["truth"]), _dev(a["lit"]))
    fit.add(_dev(b["scores"]), _dev(b["truth"]))
    assert fit.calls == 2
    ref, cref, bound = R.accumulate(b["scores"], b["truth"], None, 0.0, b["groups"], a["betas"], 1, ref1.copy(), cref1.copy(), bound1.copy())
    cal = fit.read()
    assert np.array_equal(cal.counters, cref)
    _within(cal.table, ref, bound, "two adds")
    beta, edge, empty, _ = R.solve(cal.betas, cal.table[0, :, 1], cal.table[0, :, 2], cal.counters[0, 0])
    assert (cal.at_edge[0], cal.empty[0]) == (edge, empty) and abs(cal.inverse_temperatures[0] - beta) <= 1e-12 * beta
    fit.reset()
    assert not fit.read().table.any() and fit.read().empty == [True]


def test_the_same_call_twice_gives_the_same_bits():
    for name in ("two-workgroups", "odd-width", "c16-i64"):
        a, _ = _reference(name)
        t1, c1 = _accumulate(a)
        t2, c2 = _accumulate(a)
        assert torch.equal(t1.view(torch.int64), t2.view(torch.int64)) and torch.equal(c1, c2), name


@pytest.mark.parametrize("name", ["apply-c1-vec", "apply-c1-scalar", "apply-c2-vec", "apply-c2-scalar", "apply-c3-vec", "apply-c3-scalar",
                                  "apply-c4-vec", "apply-c4-scalar", "apply-c5-vec", "apply-c5-scalar", "apply-c16-vec", "apply-c16-scalar",
                                  "apply-misaligned", "apply-two-trips"])
def test_apply(name):
    got = _run(name)
    assert np.isfinite(got).all(), name


def test_apply_edge_values_bit_for_bit():
    """-inf stays -inf beside a finite maximum; all -inf stays; a NaN or +inf makes the pixel the quiet NaN -- on both paths"""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    pixels = np.array([[-1.0, -inf, -2.0], [-inf, -inf, -inf], [nan, -1.0, -2.0], [-1.0, inf, -2.0], [-inf, -0.5, -inf],
                       [np.float32(-3e38), 0.0, np.float32(3e38)], [-inf, nan, inf], [0.0, 0.0, 0.0]], dtype=np.float32)
    for (H, W) in ((2, 4), (1, 7)):                               # vector path, scalar path
        x = np.zeros((2, 3, H, W), np.float32)
        x += np.array([-0.2, -2.0, -3.0], np.float32).reshape(1, 3, 1, 1)
        flat = x.transpose(0, 2, 3, 1).reshape(-1, 3)
        flat[:len(pixels)] = pixels
        x = np.ascontiguousarray(flat.reshape(2, H, W, 3).transpose(0, 3, 1, 2))
        betas = np.array([4.0, 0.25], np.float32)
        buf, b = _dev(x), _dev(betas)
        F.apply(buf.data_ptr(), buf.data_ptr(), b.data_ptr(), 2, 3, H, W, _stream())
        torch.cuda.synchronize()
        got = buf.cpu().numpy().transpose(0, 2, 3, 1).reshape(-1, 3)
        bits = got.view(np.uint32)
        ninf = np.float32(-inf).view(np.uint32)
        assert bits[0, 1] == ninf and np.isfinite(got[0, [0, 2]]).all() and abs(np.exp(got[0, [0, 2]].astype(np.float64)).sum() - 1) < 1e-6
        assert (bits[1] == ninf).all()
        for i in (2, 3, 6):
            assert (bits[i] == R.QNAN_BITS).all(), (i, [hex(v) for v in bits[i]])
        assert bits[4, 0] == ninf and bits[4, 2] == ninf and bits[4, 1] == 0, "a lone finite class has probability one: +0"
        assert bits[5, 2] == 0 and bits[5, 0] == ninf and bits[5, 1] == ninf, "finite inputs 6e38 apart: -inf, never NaN"
        assert np.allclose(got[7], -np.log(3.0), atol=1e-6)
        ref, bound = R.apply(x, betas)
        g64 = buf.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(g64), np.isnan(ref)) and np.array_equal(np.isneginf(g64), np.isneginf(ref))
        fin = np.isfinite(ref)
        assert (np.abs(g64[fin] - ref[fin]) <= bound[fin]).all()


def test_scale_apply_is_the_library_call():
    x = _apply_input((3, 4, 8, 12), 77)
    scale = CB.TemperatureScale([2.0, 1.0, 0.5])
    t = _dev(x)
    assert scale.apply_(t) is t
    ref, bound = R.apply(x, scale.betas_for([0, 1, 2]))
    _within(t.cpu().numpy().astype(np.float64), ref, bound, "TemperatureScale.apply_")
    one = _dev(x)
    scale.apply_(one, groups=[1, 1, 1])
    _within(one.cpu().numpy().astype(np.float64), x.astype(np.float64), R.apply(x, np.ones(3, np.float32))[1], "T = 1")
