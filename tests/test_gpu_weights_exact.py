"""ubw_pixel_weights (libubresnet_weight.so) on synthetic label images, bit for bit against the numpy reference of
tests/weights_ref.py.  No network runs here.  CASES is the module's table -- weights_ref.KERNEL_CASES, one entry per compiled
kernel -- and tests/test_cpu_weights.py holds it against the library's symbol table and against the case ids below.

Every region (labels, weights, counts) sits in a buffer of its own between GUARD guard words; the whole buffers are compared,
as bit patterns, so a store before or behind a region, or into the labels, fails the case.  The counts are pre-filled with
garbage.  `mis` = 1 moves the labels by 8 bytes and the weights by 4: no region is 16-byte aligned then and the kernels take
their element accesses."""
import numpy as np
import pytest
import torch

import weights_ref as R

pytestmark = pytest.mark.gpu

CASES = R.KERNEL_CASES
GUARD = 8                      # words in front of and behind every region: 32 bytes of float, 64 of int64
F_GUARD, L_GUARD = 0x7B7B7B7B, -0x5A5A5A5A5A5A5A5B
INF = float("inf")

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _weight as WL


class _Buf(object):
    """[GUARD + mis guard words | data | GUARD guard words] on the device"""

    def __init__(self, data, mis):
        data = data.reshape(-1)
        self.lo = GUARD + mis
        self.int64 = data.dtype == np.int64
        bits = data if self.int64 else data.view(np.int32)
        self.guard = L_GUARD if self.int64 else F_GUARD
        self.host = np.full(self.lo + bits.size + GUARD, self.guard, bits.dtype)
        self.host[self.lo:self.lo + bits.size] = bits
        self.dev = torch.from_numpy(self.host).cuda()
        self.ptr = self.dev.data_ptr() + self.lo * self.host.itemsize
        assert self.dev.data_ptr() % 64 == 0

    def check(self, want, what):
        """the whole buffer, guards included, against the guards around `want`"""
        want = want.reshape(-1)
        bits = want if self.int64 else want.view(np.int32)
        full = np.full_like(self.host, self.guard)
        full[self.lo:self.lo + bits.size] = bits
        got = self.dev.cpu().numpy()
        bad = np.flatnonzero(got != full)
        assert bad.size == 0, "%s: %d words differ, first at %d of [%d, %d): got %#x, reference %#x" % (
            what, bad.size, int(bad[0]) - self.lo, 0, bits.size, int(got[bad[0]]), int(full[bad[0]]))


def _buffers(label, mis):
    rs = np.random.RandomState(label.size % 9973)
    wgt0 = rs.rand(label.size).astype(np.float32) + np.float32(100.0)
    cnt0 = rs.randint(-2 ** 40, 2 ** 40, label.shape[0] * R.MAX_CLASSES).astype(np.int64)     # garbage the call must zero
    return _Buf(label, mis), _Buf(wgt0, mis), _Buf(cnt0, 0), wgt0, cnt0


def _call(bl, bw, bc, shape, C, max_weight, r, gain, lo):
    return WL.lib().ubw_pixel_weights(bl.ptr, bw.ptr, bc.ptr, shape[0], shape[1], shape[2], C, max_weight, r, gain, lo, L.stream_ptr())


def _run(what, label, C, r, max_weight=INF, gain=2.5, lo=1, mis=0, calls=1):
    """`calls` ubw_pixel_weights calls on the same buffers; compares every buffer with the reference after each; `what` is the
    case's id in CASES"""
    for kernel in ("count_kernel", "apply_kernel<%d>" % r):
        assert what in CASES[kernel], "case %r is not in the table of %s" % (what, kernel)
    label = np.ascontiguousarray(label, np.int64)
    ref_w, ref_c = R.reference(label, C, max_weight, r, gain, lo)
    bl, bw, bc, _, _ = _buffers(label, mis)
    tag = "%s shape=%s C=%d r=%d max=%s gain=%s lo=%d mis=%d" % (what, label.shape, C, r, max_weight, gain, lo, mis)
    for i in range(calls):
        rc = _call(bl, bw, bc, label.shape, C, max_weight, r, gain, lo)
        assert rc == 0, WL.lib().ubw_last_error().decode()
        torch.cuda.synchronize()
        bl.check(label, tag + " [labels, call %d]" % i)
        bw.check(ref_w, tag + " [weights, call %d]" % i)
        bc.check(ref_c, tag + " [counts, call %d]" % i)
    return ref_w, ref_c


def _unmarked(label, C, max_weight=INF, lo=1):
    """the weights with the gain off: what every pixel that is no interface pixel gets"""
    return R.reference(label, C, max_weight, 0, 1.0, lo)[0]


@pytest.mark.parametrize(("case", "r"), [("geometry-r0", 0), ("geometry-r1", 1), ("geometry-r2", 2), ("geometry-r3", 3), ("geometry-r4", 4)],
                         ids=["r0", "r1", "r2", "r3", "r4"])
def test_geometry_at_every_radius(case, r):
    rs = np.random.RandomState(50 + r)
    marked = 0
    for shape in R.GEOMETRY:
        for mis in (0, 1):
            label = R.sprinkle_invalid(rs, R.blobs(rs, *shape, 3), 3) if shape[1] * shape[2] > 8 else R.noise(rs, *shape, 3)
            w, _ = _run(case, label, 3, r, mis=mis)
            marked += int((w.view(np.int32) != _unmarked(label, 3).view(np.int32)).sum())
    assert (marked > 0) == (r > 0)


def test_an_odd_image_size_starts_the_second_image_unaligned():
    rs = np.random.RandomState(60)
    for shape in ((2, 5, 13), (3, 3, 6), (2, 1, 1027)):        # H*W odd; H*W even and no multiple of 4; odd and several waves
        label = R.sprinkle_invalid(rs, R.noise(rs, *shape, 3), 3)
        _run("odd-image", label, 3, 1)


@pytest.mark.parametrize("r", [0, 1])
def test_one_three_and_sixteen_classes(r):
    rs = np.random.RandomState(61 + r)
    for C in (1, 3, 16):
        label = R.noise(rs, 3, 9, 20, C)
        if C > 1:
            label[1][label[1] == C - 1] = 0                    # classes absent from an image
            label[2][label[2] == 1] = C - 1
        _, counts = _run("classes", label, C, r, lo=0 if C == 1 else 1)
        assert (counts[:, C:] == 0).all() and counts[:, :C].sum() == label.size
        if C > 1:
            assert counts[1, C - 1] == 0 and counts[2, 1] == 0 and len(set(map(tuple, counts))) == 3


def test_invalid_values_weigh_nothing_and_are_not_counted():
    rs = np.random.RandomState(63)
    for C in (1, 3, 16):
        bad = R.invalid_values(C)
        label = R.noise(rs, 2, 6, 11, C)
        flat = label.reshape(-1)
        at = rs.choice(flat.size, 2 * len(bad), replace=False)
        flat[at] = np.resize(np.array(bad, np.int64), at.size)
        for mis in (0, 1):
            w, counts = _run("invalid-values", label, C, 1, mis=mis, lo=0)
            assert not w.reshape(-1).view(np.int32)[at].any()          # +0.0f, bit for bit
            assert counts.sum() == flat.size - at.size


def test_an_invalid_pixel_in_a_window_neither_marks_nor_is_marked():
    X, T = -100, 2 ** 32 + 2                                           # T: the low word is class 2
    rows = [[1, X, 2, 0, 0, 1, T, 0, 0, 2, X, X, 1],                   # 1 and 2 two apart with r = 1; T beside 1 is no class 2
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [1, 1, T, 2, 2, 0, 0, 0, X, 1, 0, 0, 0],
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 0, X]]                   # one true contact, so that the gain is seen to work
    label = np.array([rows], np.int64)
    w, _ = _run("invalid-in-window", label, 3, 1, gain=2.5)
    plain = _unmarked(label, 3)
    marked = w != plain
    assert marked[0, 6, 4] and marked[0, 6, 5] and marked.sum() == 2
    assert not w[0][label[0] < 0].view(np.int32).any() and not w[0][label[0] == T].view(np.int32).any()


@pytest.mark.parametrize("r", [3, 4])
def test_a_window_never_reaches_into_the_next_image(r):
    B, H, W = 3, 14, 9
    label = np.zeros((B, H, W), np.int64)
    for b in range(B):
        label[b, :b + 1] = 2                                           # every image begins on class 2 ...
        label[b, H - 2:] = 1                                           # ... and ends on class 1, farther than r from it
        label[b, 6, :b] = 0
        label[b, 6, b:2 * b + 1] = -1                                  # different counts per image
    for mis in (0, 1):
        w, counts = _run("image-isolation", label, 3, r, mis=mis)
        assert np.array_equal(w.view(np.int32), _unmarked(label, 3).view(np.int32)), "the reference itself marks something"
        assert len(set(map(tuple, counts))) == B


@pytest.mark.parametrize("r", [2, 4])
def test_a_window_never_wraps_from_one_row_into_the_next(r):
    for W in (7, 8):
        label = np.zeros((2, 6, W), np.int64)
        label[:, 2, W - 1] = 1                                         # neighbours in memory, W - 1 > r columns apart
        label[:, 3, 0] = 2
        w, _ = _run("row-isolation", label, 3, r)
        assert np.array_equal(w.view(np.int32), _unmarked(label, 3).view(np.int32)), "the reference itself marks something"


def test_cap_gain_and_the_lower_class_bound():
    rs = np.random.RandomState(64)
    label = R.sprinkle_invalid(rs, R.blobs(rs, 3, 21, 70, 3), 3)
    label[:, 10, 10] = 2
    label[0][label[0] == 2] = 0
    label[0, 10, 10:12] = 2                                            # image 0: class 2 is rare
    _, counts = R.reference(label, 3)
    cap = 8.0
    full = counts[0].sum() / (3.0 * counts[0, :3])
    assert full[2] > cap and (full[:2] < cap).all(), "the cap must bind the rare class of image 0 alone"
    gain_inexact = 1.1                                                  # fl32(1.1) * fl32(w) needs rounding
    for lo in (0, 1, 3):
        for max_weight, gain in ((cap, 2.5), (INF, 0.0), (INF, 2.5), (INF, gain_inexact), (cap, gain_inexact)):
            w, _ = _run("parameters", label, 3, 2, max_weight=max_weight, gain=gain, lo=lo)
            plain = _unmarked(label, 3, max_weight)
            changed = w.view(np.int32) != plain.view(np.int32)
            assert changed.any() == (lo < 3), "lo = C marks nothing, anything below marks something"
            if max_weight == cap:
                assert plain[0][label[0] == 2].max() == np.float32(cap)
            if gain == 0.0 and lo < 3:
                assert not w.view(np.int32)[changed].any()
    marked = R.reference(label, 3, INF, 2, 2.0, 1)[0] != _unmarked(label, 3)
    exact = _unmarked(label, 3).astype(np.float64) * float(np.float32(gain_inexact))
    assert (exact[marked].astype(np.float32).astype(np.float64) != exact[marked]).any(), "no product was inexact"


def test_counts_come_back_exact_out_of_garbage():
    rs = np.random.RandomState(65)
    label = np.stack([rs.choice(3, size=(7, 33), p=[0.7 - 0.1 * b, 0.2 + 0.05 * b, 0.1 + 0.05 * b]) for b in range(4)]).astype(np.int64)
    label = R.sprinkle_invalid(rs, label, 3)
    bl, bw, bc, _, cnt0 = _buffers(label, 0)
    assert (cnt0.reshape(4, 16)[:, 3:] != 0).all()
    _, counts = _run("counts-garbage", label, 3, 0)
    assert (counts[:, 3:] == 0).all() and (counts[:, :3] > 0).all() and len(set(map(tuple, counts))) == 4
    assert [int(c) for c in counts[1, :3]] == [int(((label[1] == c)).sum()) for c in range(3)]


def test_two_calls_in_a_row_give_the_same_bits():
    rs = np.random.RandomState(66)
    label = R.sprinkle_invalid(rs, R.blobs(rs, 2, 33, 130, 3), 3)
    _run("twice", label, 3, 1, max_weight=50.0, gain=1.1, calls=2)


def test_several_workgroups_per_image_and_a_strided_count():
    rs = np.random.RandomState(67)
    span = R.BLOCK * R.LANE_PIXELS
    # eight count workgroups per image; then more images than UBW_MAX_GRID: one workgroup per image strides over three trips
    for shape in ((3, 40, 200), (R.MAX_GRID // 2 + 1, 4, 587), (R.MAX_GRID // 2 + 1, 4, 588)):
        B, H, W = shape
        per, cap = -(-H * W // span), max(1, R.MAX_GRID // B)
        assert (per > 1 and cap >= per) if B == 3 else (cap == 1 and H * W > 2 * span)
        label = rs.choice(4, size=shape, p=[0.9, 0.05, 0.04, 0.01]).astype(np.int64)       # 3 is invalid at C = 3
        label[1::2][label[1::2] == 2] = 0
        _run("many-chunks", label, 3, 2)


_BAD = {
    "B 0": dict(B=0),
    "H 0": dict(H=0),
    "W negative": dict(W=-3),
    "B*H*W 2^31": dict(B=2 ** 15, H=2 ** 8, W=2 ** 8),
    "H*W overflows int32": dict(H=2 ** 16, W=2 ** 16),
    "C 0": dict(C=0),
    "C 17": dict(C=17),
    "radius -1": dict(r=-1),
    "radius 5": dict(r=5),
    "lo -1": dict(lo=-1),
    "lo above C": dict(lo=4),
    "max_weight nan": dict(max_weight=float("nan")),
    "max_weight 0": dict(max_weight=0.0),
    "max_weight negative": dict(max_weight=-1.0),
    "gain nan": dict(gain=float("nan")),
    "gain negative": dict(gain=-0.5),
    "gain inf": dict(gain=INF),
    "null label": dict(label=None),
    "null weight": dict(weight=None),
    "null counts": dict(counts=None),
}


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_errors_launch_nothing(name):
    rs = np.random.RandomState(70)
    label = R.noise(rs, 2, 8, 16, 3)
    bl, bw, bc, wgt0, cnt0 = _buffers(label, 0)
    a = dict(label=bl.ptr, weight=bw.ptr, counts=bc.ptr, B=2, H=8, W=16, C=3, max_weight=INF, r=1, gain=2.0, lo=1)
    a.update(_BAD[name])
    rc = WL.lib().ubw_pixel_weights(a["label"], a["weight"], a["counts"], a["B"], a["H"], a["W"], a["C"], a["max_weight"], a["r"],
                                    a["gain"], a["lo"], L.stream_ptr())
    msg = WL.lib().ubw_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -1 and msg.startswith("ubw_pixel_weights"), (rc, msg)
    for b, want in ((bl, label), (bw, wgt0), (bc, cnt0)):
        b.check(want, name)
    with pytest.raises(RuntimeError, match="ubw_pixel_weights"):
        WL.check(rc, name)

