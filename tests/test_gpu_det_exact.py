"""ubx_apply (libubresnet_det.so) on synthetic buffers against the reference of tests/det_ref.py: dead wires and gain bit for bit,
noisy elements within the derived bound of the float64 result.  No network runs here.  CASES is the module's table --
det_ref.KERNEL_CASES, one entry per compiled kernel -- and tests/test_cpu_det.py holds it against the library's symbol table and
against the case ids below.

Every region (image, labels, weights, table) sits in a buffer of its own between GUARD guard words; the whole buffers are compared,
so a store before or behind a region, into the table, or into a label or weight that the rule leaves alone fails the case.
`mis` = 1 moves every 4-byte region by 4 bytes and the labels by 8: the image is not 16-byte aligned then and the kernel works by
elements.  The tables carry set bits at and beyond W, which the kernel must ignore."""
import numpy as np
import pytest
import torch

import det_ref as R
import kref

pytestmark = pytest.mark.gpu

CASES = R.KERNEL_CASES
GUARD = 8                      # words in front of and behind every region: 32 bytes of 4-byte words, 64 of int64
F_GUARD, L_GUARD = 0x7B7B7B7B, -0x5A5A5A5A5A5A5A5B
SHAPES = R.SHAPES
f32 = np.float32

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _det as XL


class _Buf(object):
    """[GUARD + mis guard words | data | GUARD guard words] on the device; 4-byte data is held as int32 bit patterns"""

    def __init__(self, data, mis):
        data = np.ascontiguousarray(data).reshape(-1)
        self.lo = GUARD + mis
        self.int64 = data.dtype == np.int64
        bits = data if self.int64 else data.view(np.int32)
        self.guard = L_GUARD if self.int64 else F_GUARD
        self.host = np.full(self.lo + bits.size + GUARD, self.guard, bits.dtype)
        self.host[self.lo:self.lo + bits.size] = bits
        self.dev = torch.from_numpy(self.host).cuda()
        self.ptr = self.dev.data_ptr() + self.lo * self.host.itemsize
        self.size = bits.size
        assert self.dev.data_ptr() % 64 == 0

    def check(self, want, what, skip=None):
        """the whole buffer, guards included, against the guards around `want` (words where `skip` is True are not compared);
        -> the region as it is on the device"""
        want = np.ascontiguousarray(want).reshape(-1)
        bits = want if self.int64 else want.view(np.int32)
        full = np.full_like(self.host, self.guard)
        full[self.lo:self.lo + bits.size] = bits
        got = self.dev.cpu().numpy()
        differ = got != full
        if skip is not None:
            differ[self.lo:self.lo + bits.size] &= ~np.ascontiguousarray(skip).reshape(-1)
        bad = np.flatnonzero(differ)
        assert bad.size == 0, "%s: %d words differ, first at %d of [%d, %d): got %#x, reference %#x" % (
            what, bad.size, int(bad[0]) - self.lo, 0, bits.size, int(got[bad[0]]), int(full[bad[0]]))
        return got[self.lo:self.lo + self.size]


def _run(what, image, label, weight, table, sigma=0.0, noise_all=False, seed=0, seq=0, dead_label=None, dead_weight=None, mis=0,
         null_label=False, null_weight=False):
    """one ubx_apply call; compares every buffer with the reference; `what` is the case's id in CASES;
    -> (image, label, weight as they are on the device, worst ratio of an error to its bound)"""
    kernel = "detector_kernel<%s>" % ("true" if sigma > 0 else "false")
    assert what in CASES[kernel], "case %r is not in the table of %s" % (what, kernel)
    b, p, h, w = image.shape
    assert table.shape == (b, p, R.row_words(w)) and table.dtype == np.uint32
    ref = R.reference(image, label, weight, table, sigma, noise_all, seed, seq, dead_label, dead_weight)
    bi, bl, bg, bt = _Buf(image, mis), _Buf(label, mis), _Buf(weight, mis), _Buf(table, mis)
    assert (bi.ptr % 16 == 0) == (mis == 0)
    rc = XL.lib().ubx_apply(bi.ptr, None if null_label else bl.ptr, None if null_weight else bg.ptr, b, p, h, w, bt.ptr, sigma,
                            1 if noise_all else 0, seed, seq, 0 if dead_label is None else 1, 0 if dead_label is None else dead_label,
                            0 if dead_weight is None else 1, 0.0 if dead_weight is None else dead_weight, L.stream_ptr())
    assert rc == 0, XL.lib().ubx_last_error().decode()
    torch.cuda.synchronize()
    tag = "%s %dx%dx%dx%d sigma=%s all=%s key=(%d, %d) dead=(%s, %s) mis=%d" % (what, b, p, h, w, sigma, noise_all, seed, seq, dead_label,
                                                                                  dead_weight, mis)
    bt.check(table, tag + " [table, read only]")
    got_l = bl.check(ref["label"], tag + " [label]").reshape(b, h, w)
    got_g = bg.check(ref["weight"], tag + " [weight]").view(f32).reshape(b, h, w)
    got_i = bi.check(ref["exact"], tag + " [image]", skip=ref["noisy"]).view(f32).reshape(b, p, h, w)
    worst = R.compare(got_i, ref)
    return got_i, got_l, got_g, worst


def _labels(rs, b, h, w):
    return rs.randint(0, 3, (b, h, w)).astype(np.int64), (rs.rand(b, h, w) * 10.0 + 0.5).astype(f32)


def _dead_mask(rs, b, p, w):
    """column 0, column W - 1 and a run across a word boundary where there is one, in turn over the planes; a few random ones"""
    dead = rs.rand(b, p, w) < 0.15
    for i in range(b):
        for j in range(p):
            k = (i * p + j) % 3
            if k == 0:
                dead[i, j, 0] = True
            elif k == 1:
                dead[i, j, w - 1] = True
            if w > 32:
                dead[i, j, 30:35] = True
    dead[0, :, w // 2] = True                              # dead in every plane of image 0
    return dead


def _gains(rs, b, p):
    g = rs.uniform(0.8, 1.25, (b, p)).astype(f32)
    g[0, 0] = 1.0                                          # one plane with the unit gain
    return g


# ------------------------------------------------------------------------------------------------------------------------
# dead wires and gain only: bit for bit
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mis", [0, 1])
def test_dead_wires_and_gain_at_the_smallest_shapes(mis):
    rs = np.random.RandomState(20 + mis)
    for b, p, h, w in SHAPES:
        image = R.crop(rs, b, p, h, w, lit=0.5)
        label, weight = _labels(rs, b, h, w)
        dead = _dead_mask(rs, b, p, w)
        table = R.make_table(_gains(rs, b, p), dead, junk=True)
        img, lab, wgt, _ = _run("dead-gain", image, label, weight, table, dead_label=-100, dead_weight=0.0, mis=mis)
        assert not img[0, :, :, w // 2].view(np.int32).any() and (lab[0, :, w // 2] == -100).all() and (wgt[0, :, w // 2] == 0.0).all()
        assert not img[:, :, :, 0][dead[:, :, 0]].view(np.int32).any()
        live = ~dead.all(axis=1)
        assert np.array_equal(lab[np.broadcast_to(live[:, None, :], lab.shape)], label[np.broadcast_to(live[:, None, :], lab.shape)])
        if w % 32:                                          # the set bits at and beyond W sit next to a last column that is live somewhere
            assert (~dead[:, :, w - 1]).any()
        # an all-zero table with unit gains leaves every byte alone
        none = R.make_table(np.ones((b, p), f32), np.zeros((b, p, w), bool), junk=True)
        _run("dead-gain", image, label, weight, none, dead_label=-100, dead_weight=0.0, mis=mis)


@pytest.mark.parametrize("mis", [0, 1])
def test_a_column_dead_in_some_planes_and_in_all(mis):
    rs = np.random.RandomState(30)
    for b, p, h, w in [(2, 3, 5, 12), (2, 3, 2, 37)]:
        image = R.crop(rs, b, p, h, w, lit=1.0)
        label, weight = _labels(rs, b, h, w)
        dead = np.zeros((b, p, w), bool)
        dead[0, 1, 3] = True                               # one plane of three
        dead[0, (0, 2), 5] = True                          # two of three
        dead[1, :, 6] = True                               # all three
        dead[1, :, w - 1] = True
        dead[0, :, 0] = True
        table = R.make_table(np.ones((b, p), f32), dead, junk=True)
        img, lab, wgt, _ = _run("dead-some-planes", image, label, weight, table, dead_label=7, dead_weight=-2.5, mis=mis)
        assert np.array_equal(lab[0, :, 3], label[0, :, 3]) and np.array_equal(wgt[0, :, 5], weight[0, :, 5])
        assert not img[0, 1, :, 3].any() and img[0, 0, :, 3].all() and img[0, 2, :, 3].all() and img[0, 1, :, 5].all()
        for i, c in ((1, 6), (1, w - 1), (0, 0)):
            assert (lab[i, :, c] == 7).all() and (wgt[i, :, c] == -2.5).all() and not img[i, :, :, c].any()
        assert (lab == 7).sum() == 3 * h


@pytest.mark.parametrize(("set_label", "set_weight"), [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_label_and_weight_switches_with_null_pointers_where_allowed(set_label, set_weight):
    rs = np.random.RandomState(40)
    b, p, h, w = 2, 3, 5, 12
    image = R.crop(rs, b, p, h, w, lit=0.5)
    label, weight = _labels(rs, b, h, w)
    dead = np.zeros((b, p, w), bool)
    dead[:, :, 4:7] = True
    table = R.make_table(_gains(rs, b, p), dead, junk=True)
    kw = dict(dead_label=-100 if set_label else None, dead_weight=0.25 if set_weight else None)
    for null_label in ([False, True] if not set_label else [False]):
        for null_weight in ([False, True] if not set_weight else [False]):
            for mis in (0, 1):
                _, lab, wgt, _ = _run("switches", image, label, weight, table, mis=mis, null_label=null_label, null_weight=null_weight, **kw)
                assert (lab[:, :, 4:7] == -100).all() == bool(set_label) and (wgt[:, :, 4:7] == 0.25).all() == bool(set_weight)


@pytest.mark.parametrize("mis", [0, 1])
def test_unit_gain_keeps_every_bit_and_a_dead_wire_zeroes_anything(mis):
    b, p, h, w = 2, 1, 3, 8
    specials = np.array([0x7FC01234, 0xFFC00001, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7F7FFFFF,
                         0x00000000, 0x3F800000, 0xC2C80000], np.uint32)
    image = np.resize(specials, b * p * h * w).view(f32).reshape(b, p, h, w)
    label, weight = _labels(np.random.RandomState(41), b, h, w)
    dead = np.zeros((b, p, w), bool)
    dead[0, 0, 1] = True                                   # a lane that stores: its other three columns keep their bits
    table = R.make_table(np.ones((b, p), f32), dead, junk=True)
    img, _, _, _ = _run("unit-gain-specials", image, label, weight, table, dead_label=0, dead_weight=0.0, mis=mis)
    keep = np.ones(image.shape, bool)
    keep[0, 0, :, 1] = False
    assert np.array_equal(img.view(np.uint32)[keep], image.view(np.uint32)[keep])
    # every column dead: NaN, infinities and the rest all read +0.0f
    table = R.make_table(np.full((b, p), 3.0, f32), np.ones((b, p, w), bool), junk=True)
    img, lab, _, _ = _run("dead-over-specials", image, label, weight, table, dead_label=-1, dead_weight=0.0, mis=mis)
    assert not img.view(np.uint32).any() and (lab == -1).all()
    assert np.isnan(image).sum() >= 6 and np.isinf(image).sum() >= 4


@pytest.mark.parametrize("mis", [0, 1])
def test_a_gain_over_the_edge_values_is_the_fp32_product(mis):
    rows = kref.edge_table(torch.float32)
    bits = np.array([v for _, v in rows], np.uint32)
    assert len(rows) == 14
    b, p, h, w = 1, 2, 3, 260
    image = np.resize(bits, b * p * h * w).view(f32).reshape(b, p, h, w)
    label, weight = _labels(np.random.RandomState(42), b, h, w)
    for gains in ([[1.1, 0.9]], [[-0.5, 3.0]], [[1e-30, 1e30]]):
        g = np.array(gains, f32)
        table = R.make_table(g, np.zeros((b, p, w), bool), junk=True)
        img, _, _, _ = _run("gain-edge-values", image, label, weight, table, mis=mis)
        with np.errstate(all="ignore"):
            want = (image * g[:, :, None, None]).astype(f32)                            # numpy's own fp32 multiply
        assert np.array_equal(img.view(np.uint32), want.view(np.uint32))


def test_the_grid_strides():
    b, p, h, w = R.STRIDE_SHAPE
    assert R.groups(b, h, w) > R.MAX_GRID * R.BLOCK
    rs = np.random.RandomState(50)
    image = R.crop(rs, b, p, h, w, lit=0.05)
    label, weight = _labels(rs, b, h, w)
    dead = rs.rand(b, p, w) < 0.1
    dead[:, :, [0, 31, 32, w - 1]] = True
    table = R.make_table(_gains(rs, b, p) * f32(1.5), dead)
    _, lab, _, _ = _run("grid-stride", image, label, weight, table, dead_label=-100, dead_weight=0.0)
    assert (lab[:, h - 1, w - 1] == -100).all() and (lab[:, 0, 0] == -100).all()
    _, _, _, worst = _run("noise-grid-stride", image, label, weight, table, sigma=2.0, seed=3, seq=9, dead_label=-100, dead_weight=0.0)
    print("noise-grid-stride: worst error / bound %.3f" % worst)


# ------------------------------------------------------------------------------------------------------------------------
# noise: within the bound of the float64 reference
# ------------------------------------------------------------------------------------------------------------------------
SPECIALS = [((0, 0, 0, 1), 0x80000000), ((0, 0, 0, 2), 0x7FC01234), ((0, 0, 0, 5), 0x00000000), ((0, 0, 1, 5), 0x80000000)]


def _noise_inputs(rs, b, p, h, w):
    """a half-lit crop, labels, weights and a table with dead wires and gains.  SPECIALS -- a -0.0, a NaN with a payload, a +0.0
    and a second -0.0 -- sit in plane (0, 0), whose gain is the unit gain, on columns that are made live: 1 and 2 share their lane
    with column 0, which _dead_mask kills there, so that lane stores; 5 is in the next lane"""
    image = R.crop(rs, b, p, h, w, lit=0.5)
    dead = _dead_mask(rs, b, p, w)
    for (i, j, r, c), bits in SPECIALS:
        image.view(np.uint32)[i, j, r, c] = bits
        dead[i, j, c] = False
    label, weight = _labels(rs, b, h, w)
    table = R.make_table(_gains(rs, b, p), dead, junk=True)
    gbits, back = R.unpack_table(table, w)
    assert gbits[0, 0] == R.ONE_BITS and back[0, 0, 0] and not any(back[i, j, c] for (i, j, r, c), _ in SPECIALS)
    assert min(s[3] for s in SHAPES) > 5 and min(s[2] for s in SHAPES) > 1
    return image, label, weight, table


def _specials(img):
    return [int(img.view(np.uint32)[at]) for at, _ in SPECIALS]


@pytest.mark.parametrize("mis", [0, 1])
def test_noise_on_lit_pixels(mis):
    rs = np.random.RandomState(60)
    worst = 0.0
    for b, p, h, w in SHAPES:
        image, label, weight, table = _noise_inputs(rs, b, p, h, w)
        for sigma in (1.5, 1e-3):
            img, _, _, r = _run("noise-lit", image, label, weight, table, sigma=sigma, seed=11, seq=4, dead_label=-100, dead_weight=0.0, mis=mis)
            worst = max(worst, r)
            _, dead = R.unpack_table(table, w)
            dead4 = np.broadcast_to(dead[:, :, None, :], image.shape)
            zero = (image == 0) & ~dead4
            gain1 = np.broadcast_to((table[..., 0] == R.ONE_BITS)[:, :, None, None], image.shape)
            # a zero of either sign stays its own bits (under the unit gain; a gain keeps it a zero), a NaN stays a NaN
            assert np.array_equal(img.view(np.uint32)[zero & gain1], image.view(np.uint32)[zero & gain1]) and not img[zero].any()
            assert np.isnan(img[np.isnan(image) & ~dead4]).all()
            # the live specials under the unit gain: both -0.0 and the +0.0 keep their bits, the NaN is still a NaN
            assert not any(dead4[at] for at, _ in SPECIALS) and all(gain1[at] for at, _ in SPECIALS)
            got = _specials(img)
            assert [got[0], got[2], got[3]] == [0x80000000, 0x00000000, 0x80000000] and np.isnan(img[SPECIALS[1][0]])
            assert not img.view(np.uint32)[dead4].any()                                  # noise on a dead column is still +0.0f
            lit = (image != 0) & ~dead4 & np.isfinite(image)
            assert (img[lit] != (image * table[..., 0].view(f32)[:, :, None, None])[lit]).mean() > 0.9
    print("noise-lit mis=%d: worst error / bound %.3f" % (mis, worst))


@pytest.mark.parametrize("mis", [0, 1])
def test_noise_on_every_live_pixel(mis):
    rs = np.random.RandomState(61)
    worst = 0.0
    for b, p, h, w in SHAPES:
        image, label, weight, table = _noise_inputs(rs, b, p, h, w)
        img, _, _, r = _run("noise-all", image, label, weight, table, sigma=1.5, noise_all=True, seed=12, seq=5, dead_label=-100, dead_weight=0.0,
                            mis=mis)
        worst = max(worst, r)
        _, dead = R.unpack_table(table, w)
        dead4 = np.broadcast_to(dead[:, :, None, :], image.shape)
        assert not img.view(np.uint32)[dead4].any()
        zero = (image == 0) & ~dead4
        assert zero.sum() < 4 or (img[zero] != 0).mean() > 0.9                          # the zeros took noise too
        assert not any(dead4[at] for at, _ in SPECIALS) and np.isnan(img[SPECIALS[1][0]])
        assert all(img[SPECIALS[k][0]] != 0 for k in (0, 2, 3))                         # zeros of either sign among them
    print("noise-all mis=%d: worst error / bound %.3f" % (mis, worst))


def test_noise_is_a_function_of_the_key_and_the_place_alone():
    rs = np.random.RandomState(62)
    for b, p, h, w in [(2, 3, 5, 12), (1, 2, 3, 260)]:
        image, label, weight, table = _noise_inputs(rs, b, p, h, w)
        kw = dict(sigma=1.5, noise_all=True, dead_label=-100, dead_weight=0.0)
        first = _run("noise-repeat", image, label, weight, table, seed=7, seq=3, **kw)[0]
        again = _run("noise-repeat", image, label, weight, table, seed=7, seq=3, **kw)[0]
        shifted = _run("noise-repeat", image, label, weight, table, seed=7, seq=3, mis=1, **kw)[0]
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32)), "two calls with one key differ"
        assert np.array_equal(first.view(np.uint32), shifted.view(np.uint32)), "the vector and the element path differ"
        seq2 = _run("noise-other-key", image, label, weight, table, seed=7, seq=4, **kw)[0]
        seed2 = _run("noise-other-key", image, label, weight, table, seed=8, seq=3, **kw)[0]
        _, dead = R.unpack_table(table, w)
        live = ~np.broadcast_to(dead[:, :, None, :], image.shape) & np.isfinite(image)
        for other in (seq2, seed2):
            assert (other[live] != first[live]).mean() > 0.95
        assert (seq2[live] != seed2[live]).mean() > 0.95


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_code_and_writes_nothing():
    rs = np.random.RandomState(90)
    b, p, h, w = 2, 1, 8, 8
    image = R.crop(rs, b, p, h, w, lit=0.5)
    label, weight = _labels(rs, b, h, w)
    table = R.make_table(np.full((b, p), 2.0, f32), np.ones((b, p, w), bool))           # a call that got through would change every byte
    bi, bl, bg, bt = _Buf(image, 0), _Buf(label, 0), _Buf(weight, 0), _Buf(table, 0)
    good = dict(image=bi.ptr, label=bl.ptr, weight=bg.ptr, B=b, P=p, H=h, W=w, table=bt.ptr, sigma=1.0, all=1, seed=1, seq=2, set_label=1,
                dead_label=-100, set_weight=1, dead_weight=0.0)
    bad = [(dict(image=None), "null pointer"), (dict(table=None), "null pointer"), (dict(label=None), "null label"),
           (dict(weight=None), "null weight"), (dict(B=0), ">= 1"), (dict(P=-1), ">= 1"), (dict(H=0), ">= 1"), (dict(W=0), ">= 1"),
           (dict(H=32768, W=32768), "below 2^31"), (dict(sigma=-1.0), "finite and >= 0"), (dict(sigma=float("nan")), "finite and >= 0"),
           (dict(sigma=float("inf")), "finite and >= 0"), (dict(dead_weight=float("inf")), "dead_weight"),
           (dict(dead_weight=float("nan")), "dead_weight"), (dict(image=bi.ptr + 2), "natural alignment"),
           (dict(label=bl.ptr + 4), "natural alignment"), (dict(weight=bg.ptr + 1), "natural alignment"),
           (dict(table=bt.ptr + 2), "natural alignment"), (dict(label=bi.ptr), "image overlaps label"),
           (dict(weight=bi.ptr + 4), "image overlaps weight"), (dict(table=bi.ptr + 8), "image overlaps table"),
           (dict(weight=bl.ptr + 8), "label overlaps weight"), (dict(table=bl.ptr + 1016), "label overlaps table"),
           (dict(table=bg.ptr + 508), "weight overlaps table")]
    for change, message in bad:
        a = dict(good)
        a.update(change)
        rc = XL.lib().ubx_apply(a["image"], a["label"], a["weight"], a["B"], a["P"], a["H"], a["W"], a["table"], a["sigma"], a["all"], a["seed"],
                                a["seq"], a["set_label"], a["dead_label"], a["set_weight"], a["dead_weight"], L.stream_ptr())
        msg = XL.lib().ubx_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -1 and msg.startswith("ubx_apply") and message in msg, (change, rc, msg)
        for buf, want in ((bi, image), (bl, label), (bg, weight), (bt, table)):
            buf.check(want, msg)
