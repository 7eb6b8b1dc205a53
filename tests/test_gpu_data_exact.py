"""ubd_prep_batch (libubresnet_data.so) on synthetic buffers, bit for bit against the numpy reference of tests/data_ref.py.
No network runs here.  CASES is the module's table -- data_ref.KERNEL_CASES, one entry per compiled kernel -- and
tests/test_cpu_data.py holds it against the library's symbol table and against the case ids below.

Every region (wire labels, labels, image, weights) sits in a buffer of its own between GUARD guard words; the whole buffers
are compared, as bit patterns, so a store before or behind a region, into an image that must not be touched or into a weight
region that is not filled fails the case.  `mis` = 1 moves the wire labels, the image and the weights by 4 bytes and the labels
by 8: no region is 16-byte aligned then and the kernel takes its element accesses."""
import numpy as np
import pytest
import torch

import data_ref as R

pytestmark = pytest.mark.gpu

CASES = R.KERNEL_CASES
GUARD = 8                      # words in front of and behind every region: 32 bytes of float, 64 of int64
F_GUARD, L_GUARD = 0x7B7B7B7B, -0x5A5A5A5A5A5A5A5B

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _data as DL


class _Buf(object):
    """[GUARD + mis guard words | data | GUARD guard words] on the device"""

    def __init__(self, data, mis):
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
        bits = want if self.int64 else want.view(np.int32)
        full = np.full_like(self.host, self.guard)
        full[self.lo:self.lo + bits.size] = bits
        got = self.dev.cpu().numpy()
        bad = np.flatnonzero(got != full)
        assert bad.size == 0, "%s: %d words differ, first at %d of [%d, %d): got %#x, reference %#x" % (
            what, bad.size, int(bad[0]) - self.lo, 0, bits.size, int(got[bad[0]]), int(full[bad[0]]))


def _run(what, wire, off, image=None, planes=1, hw=1, thr=None, fill=True, mis=0, pass_image=True):
    """one ubd_prep_batch call; compares every buffer with the reference; `what` is the case's id in CASES"""
    kernel = "prep_batch_kernel<%s>" % ("false" if thr is None else "true")
    assert what in CASES[kernel], "case %r is not in the table of %s" % (what, kernel)
    n = wire.size
    rs = np.random.RandomState(n % 9973)
    wgt0 = rs.rand(n).astype(np.float32)
    lab0 = np.full(n, 0x0123456789ABCDEF, np.int64)
    ref_lab, ref_img, ref_wgt = R.reference(wire, off, image, planes, hw, thr, wgt0, fill)
    bw, bl, bg = _Buf(wire, mis), _Buf(lab0, mis), _Buf(wgt0, mis)
    bi = None if image is None else _Buf(image, mis)
    rc = DL.lib().ubd_prep_batch(bw.ptr, bl.ptr, n, off, bi.ptr if (bi is not None and pass_image) else None, planes, hw,
                                 0 if thr is None else 1, 0.0 if thr is None else thr, bg.ptr if fill else None, L.stream_ptr())
    assert rc == 0, DL.lib().ubd_last_error().decode()
    torch.cuda.synchronize()
    tag = "%s n=%d off=%d planes=%d hw=%d thr=%s fill=%s mis=%d" % (what, n, off, planes, hw, thr, fill, mis)
    bw.check(wire, tag + " [wire labels]")
    bl.check(ref_lab, tag + " [labels]")
    bg.check(ref_wgt, tag + " [weights]")
    if bi is not None:
        bi.check(ref_img, tag + " [image]")
    return ref_lab, ref_img, ref_wgt


@pytest.mark.parametrize(("case", "mis"), [("counts-aligned", 0), ("counts-offset", 1)], ids=["counts-aligned", "counts-offset"])
def test_counts_with_the_threshold_off(case, mis):
    rs = np.random.RandomState(10 + mis)
    for n in R.COUNTS:
        wire = R.wire_labels(rs, n)
        for off in (0, -1):
            for fill in (True, False):
                _run(case, wire, off, fill=fill, mis=mis)


@pytest.mark.parametrize("mis", [0, 1])
def test_two_trips_of_the_grid(mis):
    n = R.STRIDE_COUNT
    assert n > 2 * R.MAX_GRID * R.BLOCK_SPAN
    lab, _, wgt = _run("grid-stride", R.wire_labels(np.random.RandomState(12), n), -1, fill=True, mis=mis)
    assert (wgt == 1.0).all() and (lab == R.INT64_MIN).sum() >= 7


@pytest.mark.parametrize("mis", [0, 1])
def test_edge_labels_bit_for_bit(mis):
    wire = np.array([e for e, _ in R.EDGE_LABELS] * 3, np.float32)[:-1]            # 44 values: full vectors and a tail of 0
    wire = np.concatenate([wire, wire[:3]])                                         # 47: and a tail of 3
    for off in (0, -1):
        lab, _, _ = _run("edge-labels", wire, off, fill=False, mis=mis)
        for i, (v, want) in enumerate(R.EDGE_LABELS):                               # the reference itself against the hand-written values
            assert lab[i] == (R.INT64_MIN if want is None else want + off), v


@pytest.mark.parametrize("pass_image", [True, False])
def test_threshold_off_touches_neither_image_nor_weights(pass_image):
    rs = np.random.RandomState(13)
    nb, planes, hw = 2, 3, 516
    img = R.adc_image(rs, nb, planes, hw, 10.0)
    _, out, wgt = _run("untouched", R.wire_labels(rs, nb * hw), 0, image=img, planes=planes, hw=hw, fill=False, pass_image=pass_image)
    assert np.array_equal(out.view(np.int32), img.view(np.int32)) and not (wgt == 1.0).all()


def _images_of(n):
    """(images, pixels per image) to run a pixel count at: one image always (hw % 4 == 0 and the aligned image take vector
    accesses), three images where n allows (a lane's four pixels then cross from one image into the next)"""
    return [(1, n)] + ([(3, n // 3)] if n % 3 == 0 and n > 3 else [])


@pytest.mark.parametrize(("case", "planes", "thr", "mis"),
                         [("thr10-p1", 1, 10.0, 0), ("thr10-p3", 3, 10.0, 0), ("thr0-p3", 3, 0.0, 0), ("thr10-p3-offset", 3, 10.0, 1)],
                         ids=["thr10-p1", "thr10-p3", "thr0-p3", "thr10-p3-offset"])
def test_counts_with_the_threshold_on(case, planes, thr, mis):
    rs = np.random.RandomState(20 + planes + mis)
    shapes = [s for n in R.COUNTS for s in _images_of(n)] + [(2, 516), (4, 256), (5, 7 * 5)]
    dark = total = 0
    for nb, hw in shapes:
        wire = R.wire_labels(rs, nb * hw)
        img = R.adc_image(rs, nb, planes, hw, thr)
        for off, fill in ((0, True), (-1, False)):
            lab, out, _ = _run(case, wire, off, image=img, planes=planes, hw=hw, thr=thr, fill=fill, mis=mis)
        dark += int(np.all(img.reshape(nb, planes, hw) < np.float32(thr), axis=1).sum())
        total += nb * hw
    assert 0.05 < dark / total < 0.9, "the images must leave both dark and lit pixels"


@pytest.mark.parametrize(("nb", "rest"), [(1, 3), (4, 0)])
def test_two_trips_of_the_grid_with_the_threshold_on(nb, rest):
    n = R.STRIDE_COUNT - 3 + rest
    assert n % nb == 0 and n > 2 * R.MAX_GRID * R.BLOCK_SPAN and ((n // nb) % 4 == 0) == (rest == 0)
    rs = np.random.RandomState(30 + nb)
    _run("thr-grid-stride", R.wire_labels(rs, n), 0, image=R.adc_image(rs, nb, 3, n // nb, 10.0), planes=3, hw=n // nb, thr=10.0, fill=True)


@pytest.mark.parametrize("mis", [0, 1])
def test_a_pixel_lit_in_one_of_three_planes_keeps_its_label(mis):
    t = np.float32(10.0)
    below, above = np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))
    hw = 8
    img = np.full((1, 3, hw), 2.0, np.float32)
    img[0, :, 1] = [below, above, -0.0]            # lit by plane 1 alone
    img[0, :, 2] = [1.0, 2.0, t]                   # at the threshold is not below
    img[0, :, 3] = [np.nan, 1.0, 2.0]              # a NaN is not below
    img[0, :, 4] = [below, below, -0.0]            # dark
    img[0, :, 5] = [50.0, 60.0, 70.0]
    wire = np.full(hw, 2.0, np.float32)
    lab, out, _ = _run("one-of-three", wire, -1, image=img.reshape(-1), planes=3, hw=hw, thr=10.0, fill=True, mis=mis)
    assert lab.tolist() == [0, 1, 1, 1, 0, 1, 0, 0]
    out = out.reshape(3, hw)
    assert out[:, 1].view(np.int32).tolist() == [0, int(above.view(np.int32)), 0]
    assert out[2, 2] == t and np.isnan(out[0, 3]) and out[:, 5].tolist() == [50.0, 60.0, 70.0] and not out[:, 4].view(np.int32).any()


_BAD = {
    "n 0": dict(n=0),
    "n 2^31": dict(n=2 ** 31),
    "planes 0": dict(planes=0),
    "null wire label": dict(wire=None),
    "threshold on, null image": dict(use=1, image=None),
}


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_errors_launch_nothing(name):
    n = 1024
    rs = np.random.RandomState(40)
    wire, img, wgt = R.wire_labels(rs, n), R.adc_image(rs, 1, 1, n, 10.0), rs.rand(n).astype(np.float32)
    lab = np.full(n, 77, np.int64)
    bw, bl, bi, bg = _Buf(wire, 0), _Buf(lab, 0), _Buf(img, 0), _Buf(wgt, 0)
    a = dict(wire=bw.ptr, out=bl.ptr, n=n, image=bi.ptr, planes=1, use=0)
    a.update(_BAD[name])
    rc = DL.lib().ubd_prep_batch(a["wire"], a["out"], a["n"], 0, a["image"], a["planes"], n, a["use"], 10.0, bg.ptr, L.stream_ptr())
    msg = DL.lib().ubd_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and msg.startswith("ubd_prep_batch"), (rc, msg)
    for b, want in ((bw, wire), (bl, lab), (bi, img), (bg, wgt)):
        b.check(want, name)
    with pytest.raises(RuntimeError, match="ubd_prep_batch"):
        DL.check(rc, name)
