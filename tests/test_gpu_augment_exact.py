"""uba_augment_batch (libubresnet_aug.so) on synthetic buffers, bit for bit against the numpy reference of tests/augment_ref.py.
No network runs here.  CASES is the module's table -- augment_ref.KERNEL_CASES, one entry per compiled kernel -- and
tests/test_cpu_augment.py holds it against the library's symbol table and against the case ids below.

Every region (image, wire labels, weights and the three outputs) sits in a buffer of its own between GUARD guard words; the
whole buffers are compared, as bit patterns, so a store before or behind an output or into a source fails the case.  `mis` = 1
moves every float region by 4 bytes and the labels by 8: no region is 16-byte aligned then and the kernel stores by elements."""
import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

CASES = R.KERNEL_CASES
GUARD = 8                      # words in front of and behind every region: 32 bytes of float, 64 of int64
F_GUARD, L_GUARD = 0x7B7B7B7B, -0x5A5A5A5A5A5A5A5B
FLIPS = [(0, 0), (1, 0), (0, 1), (1, 1)]
# (H, W, pad): an offset of 8 shifts whole rows and columns of the 8 x 8 image out; W % 4 == 0 but W % 8 != 0; the element path; a row longer than
# a wave's span of 256 columns; flips only
SHAPES = [(8, 8, 4), (5, 12, 4), (5, 7, 4), (3, 260, 4), (6, 12, 0)]
PADS = [(0, 0.0), (-100, 1.0), (0, 1.0), (-100, 0.0)]

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _aug as AL
    from ubresnet_amd import _data as DL


class _Buf(object):
    """[GUARD + mis guard words | data | GUARD guard words] on the device"""

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

    def check(self, want, what):
        """the whole buffer, guards included, against the guards around `want`; -> the region as it is on the device"""
        want = np.ascontiguousarray(want).reshape(-1)
        bits = want if self.int64 else want.view(np.int32)
        full = np.full_like(self.host, self.guard)
        full[self.lo:self.lo + bits.size] = bits
        got = self.dev.cpu().numpy()
        bad = np.flatnonzero(got != full)
        assert bad.size == 0, "%s: %d words differ, first at %d of [%d, %d): got %#x, reference %#x" % (
            what, bad.size, int(bad[0]) - self.lo, 0, bits.size, int(got[bad[0]]), int(full[bad[0]]))
        return got[self.lo:self.lo + self.size]


def _run(what, image, wire, weight, params, pad, off=0, thr=None, pad_label=0, pad_weight=0.0, mis=0):
    """one uba_augment_batch call; compares every buffer with the reference; `what` is the case's id in CASES;
    -> the three outputs as they are on the device"""
    kernel = "augment_batch_kernel<%s>" % ("false" if thr is None else "true")
    assert what in CASES[kernel], "case %r is not in the table of %s" % (what, kernel)
    b, p, h, w = image.shape
    n = b * h * w
    params = np.ascontiguousarray(params, np.int32).reshape(b, 4)
    ref = R.reference(image, wire, weight, params, pad, off, thr, pad_label, pad_weight)
    bi, bw = _Buf(image, mis), _Buf(wire, mis)
    bg = None if weight is None else _Buf(weight, mis)
    oi = _Buf(np.full(p * n, 123.25, np.float32), mis)
    ol = _Buf(np.full(n, 0x0123456789ABCDEF, np.int64), mis)
    og = _Buf(np.full(n, -77.5, np.float32), mis)
    rc = AL.lib().uba_augment_batch(bi.ptr, bw.ptr, None if bg is None else bg.ptr, oi.ptr, ol.ptr, og.ptr, b, p, h, w, pad,
                                    params.ctypes.data, off, 0 if thr is None else 1, 0.0 if thr is None else thr,
                                    pad_label, pad_weight, L.stream_ptr())
    assert rc == 0, AL.lib().uba_last_error().decode()
    torch.cuda.synchronize()
    tag = "%s %dx%dx%dx%d pad=%d params=%s off=%d thr=%s weight=%s pads=(%d, %s) mis=%d" % (
        what, b, p, h, w, pad, params.tolist() if b <= 5 else "...", off, thr, weight is not None, pad_label, pad_weight, mis)
    bi.check(image, tag + " [image, a source]")
    bw.check(wire, tag + " [wire labels, a source]")
    if bg is not None:
        bg.check(weight, tag + " [weights, a source]")
    got_i = oi.check(ref[0], tag + " [image_out]").view(np.float32).reshape(b, p, h, w)
    got_l = ol.check(ref[1], tag + " [label_out]").reshape(b, h, w)
    got_g = og.check(ref[2], tag + " [weight_out]").view(np.float32).reshape(b, h, w)
    return got_i, got_l, got_g


def _inputs(rs, b, p, h, w, thr):
    n = b * h * w
    image = R.adc_image(rs, b, p, h * w, 10.0 if thr is None else thr).reshape(b, p, h, w)
    wire = R.wire_labels(rs, n).reshape(b, h, w)
    weight = (rs.rand(b, h, w) * 10.0).astype(np.float32)
    return image, wire, weight


@pytest.mark.parametrize(("case", "thr"), [("sweep", None), ("sweep-thr10", 10.0), ("sweep-thr0", 0.0)],
                         ids=["sweep", "sweep-thr10", "sweep-thr0"])
def test_every_flip_and_offset_at_the_smallest_shapes(case, thr):
    """per shape, flip combination, P and alignment: five images per call whose column offsets are the five offsets, one call
    per row offset -- all 25 pairs; the other switches (weight source, label offset, the two pad values) take their 16
    combinations in turn, per P and alignment, and their coverage is asserted at the end"""
    rs = np.random.RandomState(50 + int(thr or 0))
    switches = [(has_w, off, pads) for has_w in (1, 0) for off in (0, -1) for pads in PADS]
    turn = {}
    seen = set()
    padded = total = 0
    for h, w, pad in SHAPES:
        offsets = sorted(set([0, min(1, 2 * pad), min(3, 2 * pad), pad, 2 * pad]))
        b = len(offsets)
        for p in (1, 3):
            image, wire, weight = _inputs(rs, b, p, h, w, thr)
            for fr, fc in FLIPS:
                for orow in offsets:
                    for mis in (0, 1):
                        params = [(fr, fc, orow, ocol) for ocol in offsets]
                        turn[mis, p] = turn.get((mis, p), -1) + 1
                        has_w, off, pads = switches[turn[mis, p] % len(switches)]
                        seen.add((has_w, off, pads, mis, p))
                        _, lab, _ = _run(case, image, wire, weight if has_w else None, params, pad, off, thr, pads[0], pads[1], mis)
                        inside = R.source_index(np.array(params), b, h, w, pad)[2]
                        padded += int((~inside).sum())
                        total += inside.size
                        if (h, w, pad) == (8, 8, 4) and orow == 8:
                            gone = ~inside.any(axis=2)                                    # half of the rows went out whole
                            assert gone.sum() == b * 4 and (lab[gone] == pads[0]).all()
    assert len(seen) == 2 * 2 * 4 * 2 * 2, "a combination of the switches was never drawn: %d of 64" % len(seen)
    assert 0.1 < padded / total < 0.9


@pytest.mark.parametrize(("case", "thr"), [("three-images", None), ("three-images-thr", 10.0)], ids=["off", "thr10"])
@pytest.mark.parametrize("mis", [0, 1])
def test_three_images_with_three_parameter_sets(case, thr, mis):
    rs = np.random.RandomState(60 + mis)
    for h, w, pad in SHAPES:
        for p in (1, 3):
            image, wire, weight = _inputs(rs, 3, p, h, w, thr)
            params = [(0, 1, min(1, 2 * pad), 2 * pad), (1, 0, 2 * pad, min(3, 2 * pad)), (1, 1, pad, 0)]
            out = _run(case, image, wire, weight, params, pad, -1, thr, -100, 1.0, mis)
            for i in range(3):                     # each image alone gives the same: the parameter word of image b reaches image b
                one = R.reference(image[i:i + 1], wire[i:i + 1], weight[i:i + 1], [params[i]], pad, -1, thr, -100, 1.0)
                for name, a, c in zip(("image", "label", "weight"), out, one):
                    assert np.array_equal(np.ascontiguousarray(a[i]).view(np.int32), np.ascontiguousarray(c[0]).view(np.int32)), (name, i)


@pytest.mark.parametrize(("case", "thr"), [("edge-values", None), ("edge-values-thr", 10.0)], ids=["off", "thr10"])
@pytest.mark.parametrize("mis", [0, 1])
def test_edge_labels_and_image_specials_bit_for_bit(case, thr, mis):
    h, w, pad = 5, 12, 4
    t = np.float32(10.0)
    below, above = np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))
    edges = np.array([e for e, _ in R.EDGE_LABELS], np.float32)
    wire = np.resize(edges, h * w).reshape(1, h, w)
    special = np.array([below, t, above, -0.0, 0.0, np.nan, 50.0, -3.0], np.float32)
    image = np.stack([np.resize(np.roll(special, s), h * w).reshape(h, w) for s in (0, 3, 5)])[None]
    weight = np.resize(np.array([0.0, -0.0, np.nan, np.inf, 1e-40, 3.5], np.float32), h * w).reshape(1, h, w)
    for fr, fc in FLIPS:
        for off in (0, -1):
            params = [(fr, fc, 3, 1)]
            img, lab, wgt = _run(case, image, wire, weight, params, pad, off, thr, -100, 1.0, mis)
            sr, sc, inside = R.source_index(np.array(params), 1, h, w, pad)
            checked = 0
            for r in range(h):
                for c in range(w):
                    if not inside[0, r, c]:
                        assert lab[0, r, c] == -100 and wgt[0, r, c] == 1.0 and not img[0, :, r, c].view(np.int32).any()
                        continue
                    y, x = int(sr[0, r]), int(sc[0, c])
                    src = image[0, :, y, x]
                    with np.errstate(invalid="ignore"):
                        dark = thr is not None and bool(np.all(src < t))
                    want = R.EDGE_LABELS[(y * w + x) % len(edges)][1]       # the hand-written value, not the reference's
                    assert lab[0, r, c] == (0 if dark else R.INT64_MIN if want is None else want + off), (r, c)
                    for pl in range(3):
                        v = src[pl]
                        keep = thr is None or not v < t                      # a NaN is not below
                        assert img[0, pl, r, c].view(np.int32) == (v.view(np.int32) if keep else 0), (pl, r, c)
                    assert wgt[0, r, c].view(np.int32) == weight[0, y, x].view(np.int32)
                    checked += 1
            assert checked >= 12


def test_two_trips_of_the_grid_and_a_part_of_a_third():
    b, h, w = R.stride_shape()
    assert R.groups(b, h, w) > 2 * R.MAX_GRID * R.BLOCK and w % 4 == 0
    rs = np.random.RandomState(70)
    image = rs.uniform(-50.0, 50.0, (b, 1, h, w)).astype(np.float32)
    wire = rs.randint(0, 3, (b, h, w)).astype(np.float32)
    weight = rs.rand(b, h, w).astype(np.float32)
    params = [(0, 1, 8, 3), (1, 0, 0, 8), (1, 1, 5, 5), (0, 0, 1, 0)]
    _, lab, _ = _run("grid-stride", image, wire, weight, params, 4, 0, None, -100, 0.0, 0)
    assert (lab[:, -1] == -100).sum() >= w and (lab[:, h // 2] >= 0).any()


@pytest.mark.parametrize("mis", [0, 1])
def test_labels_and_weights_move_with_the_image(mis):
    """image, wire labels and weights hold the pixel's own index + 1: everywhere the three outputs name the same source pixel"""
    b, h, w, pad = 3, 37, 52, 4
    idx = (np.arange(b * h * w, dtype=np.float32) + 1.0).reshape(b, h, w)
    for params in ([(0, 0, 0, 0), (1, 0, 8, 3), (0, 1, 2, 7)], [(1, 1, 1, 1), (1, 1, 8, 8), (0, 0, 4, 4)]):
        img, lab, wgt = _run("same-pixel", idx[:, None], idx, idx, params, pad, 0, None, 0, 0.0, mis)
        assert np.array_equal(img[:, 0].view(np.int32), wgt.view(np.int32)) and np.array_equal(lab, wgt.astype(np.int64))
        assert (lab == 0).any() and len(np.unique(lab)) > b * (h - 8) * (w - 8)
    img, lab, wgt = _run("same-pixel", idx[:, None], idx, idx, [(0, 0, 4, 4)] * 3, pad, 0, None, 0, 0.0, mis)
    assert np.array_equal(wgt, idx)                                  # the centre cut without a flip is the batch itself


@pytest.mark.parametrize(("case", "thr"), [("identity", None), ("identity-thr", 10.0)], ids=["off", "thr10"])
@pytest.mark.parametrize("has_weight", [True, False])
def test_identity_parameters_give_what_prep_batch_gives(case, thr, has_weight):
    rs = np.random.RandomState(80)
    for b, p, h, w in ((2, 1, 16, 20), (3, 3, 5, 7), (2, 3, 8, 260)):
        image, wire, weight = _inputs(rs, b, p, h, w, thr)
        n = b * h * w
        img, lab, wgt = _run(case, image, wire, weight if has_weight else None, np.zeros((b, 4), np.int32), 0, -1, thr, -100, 5.0, 0)
        d_img, d_wire, d_wgt = (torch.from_numpy(a.copy()).cuda() for a in (image, wire, weight))
        d_lab = torch.empty(n, dtype=torch.int64, device="cuda")
        DL.prep_batch(d_wire.data_ptr(), d_lab.data_ptr(), n, -1, image=d_img.data_ptr(), planes=p, hw=h * w, threshold=thr,
                      weight_fill=None if has_weight else d_wgt.data_ptr(), stream=L.stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_img.cpu().numpy().view(np.int32), img.view(np.int32))
        assert np.array_equal(d_lab.cpu().numpy().reshape(b, h, w), lab)
        assert np.array_equal(d_wgt.cpu().numpy().view(np.int32), wgt.view(np.int32))


def test_an_argument_error_launches_nothing():
    rs = np.random.RandomState(90)
    b, p, h, w = 2, 1, 8, 8
    image, wire, weight = _inputs(rs, b, p, h, w, None)
    bi, bw, bg = _Buf(image, 0), _Buf(wire, 0), _Buf(weight, 0)
    out_i, out_l, out_g = np.full(b * h * w, 1.5, np.float32), np.full(b * h * w, 77, np.int64), np.full(b * h * w, 2.5, np.float32)
    oi, ol, og = _Buf(out_i, 0), _Buf(out_l, 0), _Buf(out_g, 0)
    for params, ptr in (([(0, 0, 0, 0), (0, 0, 9, 0)], oi.ptr), ([(0, 0, 0, 0), (0, 2, 0, 0)], oi.ptr), ([(0, 0, 0, 0)] * 2, bi.ptr)):
        par = np.array(params, np.int32)
        rc = AL.lib().uba_augment_batch(bi.ptr, bw.ptr, bg.ptr, ptr, ol.ptr, og.ptr, b, p, h, w, 4, par.ctypes.data, 0, 0, 0.0, 0, 0.0,
                                        L.stream_ptr())
        msg = AL.lib().uba_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -1 and msg.startswith("uba_augment_batch"), (rc, msg)
        for buf, want in ((bi, image), (bw, wire), (bg, weight), (oi, out_i), (ol, out_l), (og, out_g)):
            buf.check(want, msg)
