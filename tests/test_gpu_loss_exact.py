"""libubresnet_loss.so on the device, exactly: ubl_focal_fwd and ubl_focal_bwd over whole buffers between guard margins, at the
smallest shapes at which each path can go wrong (sizes from the header's geometry), against tests/loss_ref.py.

Operands: predict is a true fp32 log-softmax of seeded logits with a few target-channel entries forced to 0 and a few below the
underflow of expf; target holds every class and ignore_index (one case: labels out of range); pixel and class weights are powers
of two, so the weight products and the weight sum are exact.  Counts and the bad-label word are exact; at gamma = 0 in "pixels"
mode the gradient is bit-equal to ubr_pixelwise_nll_bwd and the loss within 1 fp32 ulp of PixelWiseNLLLoss; for gamma in
{0.5, 1, 2, 5} every gradient element and the loss sum lie within loss_ref's bound; everything that is not the target channel of a
contributing pixel is +0.0."""
import functools

import numpy as np
import pytest
import torch

import kref
import loss_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _loss as K
    from ubresnet_amd import ops
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

DEV = "cuda"
IGN = -100
GAMMAS = [0.5, 1.0, 2.0, 5.0]
BIG_W = R.TRIP_PIXELS * R.MAX_GRID + 1004          # every workgroup takes a second trip, the last of them partly filled
# name -> (N, C, H, W, offset elements of every view, labels out of range)
CASES = {
    "1x3x4x4 less than a unit per lane": (1, 3, 4, 4, 0, False),
    "2x3x6x6 image boundary inside a workgroup": (2, 3, 6, 6, 0, True),
    "2x4x5x7 scalar form": (2, 4, 5, 7, 0, False),
    "1x16x8x8 most classes": (1, 16, 8, 8, 0, False),
    "1x1x8x8 one class": (1, 1, 8, 8, 0, False),
    "2x3x6x6 views off 16-byte alignment": (2, 3, 6, 6, 1, False),
    "1x3x1x%d second partial trip" % BIG_W: (1, 3, 1, BIG_W, 0, False),
}


class Guard:
    """n elements, `off` elements past a 64-element margin, another margin behind; begin() snapshots, check() asserts that
    nothing outside the n elements (written=False: nothing at all) changed"""

    def __init__(self, values, off=0):
        v = torch.as_tensor(values).reshape(-1)
        self.n, self.lo = v.numel(), 64 + off
        fill = float("nan") if v.is_floating_point() else -7
        self.full = torch.full((self.n + 128 + off,), fill, dtype=v.dtype, device=DEV)
        self.t = self.full[self.lo:self.lo + self.n]
        self.t.copy_(v)
        self.before = self.full.clone()

    def ptr(self):
        return self.t.data_ptr()

    def begin(self):
        self.before = self.full.clone()

    def check(self, what, written=False):
        w = torch.zeros(self.full.numel(), dtype=torch.bool, device=DEV)
        if written:
            w[self.lo:self.lo + self.n] = True
        kref.assert_untouched(self.full, self.before, w, what)


@functools.lru_cache(maxsize=None)
def _operands(name):
    """seeded host operands of a case (numpy), made once and never changed"""
    N, C, H, W, off, bad = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if C > 1:
        predict = torch.log_softmax(4.0 * torch.randn(N, C, H, W, generator=g, dtype=torch.float32), dim=1)
    else:
        predict = -torch.rand(N, C, H, W, generator=g, dtype=torch.float32) * 3.0         # (a log-softmax over one class is all zeros)
    flat = torch.randperm(N * H * W, generator=g)
    target = (torch.arange(N * H * W) % C)[flat].reshape(N, H, W)                         # every class
    hw = H * W
    pos = torch.randperm(N * hw, generator=g)
    k = max(2, N * hw // 16)
    target.view(-1)[pos[:k]] = IGN
    if bad:
        target.view(-1)[pos[k:k + 3]] = torch.tensor([C, -1, 1 << 40])
    # forced target-channel values: lp = 0 (q = 0), below the underflow of expf (p = 0), in its subnormal range
    forced = pos[k + 3:k + 9]
    for p, v in zip(forced.tolist(), (0.0, 0.0, -104.0, -110.0, -95.0, -1e-6)):
        n, r = divmod(p, hw)
        t = int(target.view(-1)[p])
        if 0 <= t < C:
            predict.view(N, C, hw)[n, t, r] = v
    pw = 2.0 ** torch.randint(-1, 3, (N, H, W), generator=g).float()
    cw = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float()
    return predict.numpy(), target.numpy(), pw.numpy(), cw.numpy()


@functools.lru_cache(maxsize=2)
def _terms(name, gamma):
    predict, target, pw, cw = _operands(name)
    return R.forward(predict, target, pw, cw, IGN, gamma, "pixels")


def _reference(name, gamma, mode):
    """loss_ref.forward of a case: the terms are computed once per (case, gamma) and shared by the three modes"""
    f = dict(_terms(name, gamma))
    f["denom"] = {"pixels": f["denom"], "valid": float(f["valid"]), "weights": f["weight_sum"]}[mode]
    f["loss"] = f["loss_sum"] / f["denom"] if f["denom"] != 0 else 0.0
    return f


class Device:
    """the operands of a case in guarded device buffers, and the two calls"""

    def __init__(self, name, classw=True):
        self.N, self.C, self.H, self.W, off, _ = CASES[name]
        predict, target, pw, cw = _operands(name)
        self.predict, self.target, self.pw = Guard(predict, off), Guard(target, off), Guard(pw, off)
        self.cw = Guard(cw) if classw else None
        self.g = Guard(np.full(predict.size, np.nan, np.float32), off)
        self.ws = torch.full((K.WORKSPACE_BYTES // 8 + 16,), float("nan"), dtype=torch.float64, device=DEV)
        self.ctl = Guard(np.full(K.CTL_WORDS, np.nan, np.float64))
        self.loss = Guard(np.full(1, np.nan, np.float32))
        self.g_loss = Guard(np.ones(1, np.float32))
        self.what = name

    def everything(self):
        return [b for b in (self.predict, self.target, self.pw, self.cw, self.g, self.ctl, self.loss, self.g_loss) if b is not None]

    def fwd(self, gamma, mode, stream=None):
        K.focal_fwd(self.predict.ptr(), self.target.ptr(), self.pw.ptr(), None if self.cw is None else self.cw.ptr(), self.N, self.C, self.H,
                    self.W, IGN, gamma, K.MODES[mode], self.ws[2:].data_ptr(), self.ctl.ptr(), self.loss.ptr(),
                    L.stream_ptr() if stream is None else stream)

    def bwd(self, gamma, stream=None):
        K.focal_bwd(self.g_loss.ptr(), self.ctl.ptr(), self.predict.ptr(), self.target.ptr(), self.pw.ptr(),
                    None if self.cw is None else self.cw.ptr(), self.N, self.C, self.H, self.W, IGN, gamma, self.g.ptr(),
                    L.stream_ptr() if stream is None else stream)

    def run(self, gamma, mode, g_loss=1.0):
        """forward and backward with every buffer's margins (and every input) checked -> (ctl dict, loss fp32, g [N,C,H,W] numpy)"""
        self.g_loss.t.fill_(g_loss)
        self.g.t.fill_(float("nan"))
        for b in self.everything():
            b.begin()
        ws_tail = self.ws[2 + K.grid(self.N * self.H * self.W) * K.ROW_WORDS:].clone()
        self.fwd(gamma, mode)
        self.bwd(gamma)
        torch.cuda.synchronize()
        for b in self.everything():
            b.check("%s gamma %g %s" % (self.what, gamma, mode), written=b in (self.g, self.ctl, self.loss))
        # the workspace: rows of the grid, nothing behind them, nothing in front
        assert bool(torch.isnan(self.ws[:2]).all()) and torch.equal(self.ws[2 + K.grid(self.N * self.H * self.W) * K.ROW_WORDS:].view(torch.int64),
                                                                    ws_tail.view(torch.int64))
        ctl = K.read_ctl(self.ctl.t.cpu().numpy().tobytes())
        return ctl, self.loss.t.cpu().numpy()[0], self.g.t.cpu().numpy().reshape(self.N, self.C, self.H, self.W)


def _check_counts(ctl, f, C, mode, what):
    assert ctl["valid"] == f["valid"] and ctl["bad"] == f["bad"] and ctl["mode"] == K.MODES[mode], what
    assert ctl["class_pixels"] == f["class_pixels"] + [0] * (16 - C), what
    assert ctl["weight_sum"] == f["weight_sum"], what                                   # powers of two: the fp64 sum is exact
    assert ctl["denom"] == f["denom"], what
    assert ctl["class_loss"][C:] == [0.0] * (16 - C), what


def test_the_cases_cover_the_paths_of_the_launch():
    assert (K.BLOCK, K.UNROLL, K.MAX_GRID) == (R.BLOCK, R.UNROLL, R.MAX_GRID)
    shapes = {k: v[:4] for k, v in CASES.items()}
    pixels = {k: n * h * w for k, (n, c, h, w) in shapes.items()}
    assert min(pixels.values()) == 16 < 4 * K.BLOCK                                     # less than one unit per lane
    assert [h * w % 4 for n, c, h, w in shapes.values()] == [0, 0, 3, 0, 0, 0, 0]      # one case is the scalar form by its extent,
    assert [v[4] for v in CASES.values()] == [0, 0, 0, 0, 0, 1, 0]                      # one by its alignment
    assert sorted(c for n, c, h, w in shapes.values())[0] == 1 and max(c for n, c, h, w in shapes.values()) == K.MAX_CLASSES
    big = max(pixels.values())
    assert K.grid(big) == K.MAX_GRID and K.TRIP_PIXELS * K.MAX_GRID < big < K.TRIP_PIXELS * (K.MAX_GRID + 1) and big % 4 == 0
    for name in CASES:
        predict, target, pw, cw = _operands(name)
        N, C, H, W = shapes[name]
        t = target.reshape(-1)
        assert set(range(C)) <= set(t.tolist()) and (t == IGN).sum() >= 2
        ok = (t >= 0) & (t < C)
        lp = np.take_along_axis(predict.reshape(N, C, H * W), np.clip(target, 0, C - 1).reshape(N, 1, H * W), axis=1).reshape(-1)[ok]
        assert (lp == 0).any() and (lp <= -104).any(), name
        assert set(np.log2(pw).reshape(-1).tolist()) <= {-1.0, 0.0, 1.0, 2.0} and set(np.log2(cw).tolist()) <= {-1.0, 0.0, 1.0}
    assert _reference("2x3x6x6 image boundary inside a workgroup", 2.0, "pixels")["bad"] == 3


@pytest.mark.parametrize("name", sorted(CASES))
def test_gamma_0_is_the_nll_loss_bit_for_bit(name):
    """"pixels" mode, g_loss = 1: the gradient equals ubr_pixelwise_nll_bwd's on the same operands bit for bit; the loss is within
    1 fp32 ulp of PixelWiseNLLLoss (whose fp64 atomics are unordered); with and without class weights"""
    N, C, H, W, off, _ = CASES[name]
    for classw in (True, False):
        d = Device(name, classw)
        ctl, loss, g = d.run(0.0, "pixels")
        f = R.forward(*_operands(name)[:3], _operands(name)[3] if classw else None, IGN, 0.0, "pixels")
        _check_counts(ctl, f, C, "pixels", name)
        shape = (N, C, H, W)
        predict = d.predict.t.view(shape)
        target, pw = d.target.t.view(N, H, W), d.pw.t.view(N, H, W)
        cw = d.cw.t if classw else None
        want = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
        ops.pixelwise_nll_bwd(d.g_loss.t, target.contiguous(), pw.contiguous(), cw, IGN, shape, want)
        torch.cuda.synchronize()
        kref.assert_bits(torch.from_numpy(g), want.cpu(), what="%s: gradient against ubr_pixelwise_nll_bwd" % name)
        if f["bad"] == 0:
            old = float(PixelWiseNLLLoss(weight=cw, ignore_index=IGN)(predict.contiguous(), target.contiguous(), pw.contiguous()).cpu())
            assert abs(float(loss) - old) <= float(np.spacing(np.float32(abs(old)))), (name, float(loss), old)
        assert abs(ctl["loss_sum"] - f["loss_sum"]) <= f["lim_sum"], name
        assert float(loss) == float(R.mean("pixels", ctl["loss_sum"], ctl["weight_sum"], ctl["valid"], N * H * W)[2])
    PixelWiseNLLLoss.flush()


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_focal_terms_and_gradients_lie_within_the_bound(name, gamma):
    N, C, H, W, off, _ = CASES[name]
    d = Device(name)
    for mode in R.MODES:
        what = "%s gamma %g %s" % (name, gamma, mode)
        f = _reference(name, gamma, mode)
        ctl, loss, g = d.run(gamma, mode, g_loss=0.5)
        _check_counts(ctl, f, C, mode, what)
        # the loss sum, the per-class sums, the mean
        err = abs(ctl["loss_sum"] - f["loss_sum"])
        print("%s: loss sum %.9g (reference %.9g), error / bound %.3f" % (what, ctl["loss_sum"], f["loss_sum"], err / f["lim_sum"]))
        assert err <= f["lim_sum"], what
        for c in range(C):
            assert abs(ctl["class_loss"][c] - f["class_loss"][c]) <= f["lim_sum"], what
        denom, inv, mean = R.mean(mode, ctl["loss_sum"], ctl["weight_sum"], ctl["valid"], N * H * W)
        assert (np.float32(ctl["inv_denom"]).view(np.uint32), np.float32(ctl["loss"]).view(np.uint32), np.float32(loss).view(np.uint32)) \
            == (inv.view(np.uint32), mean.view(np.uint32), mean.view(np.uint32)), what
        # every gradient element
        want, lim, hot = R.backward(0.5, f, gamma, C)
        gerr = np.abs(g.astype(np.float64) - want)
        ratio = float((gerr[hot] / lim[hot]).max())
        print("%s: worst gradient error / bound %.3f" % (what, ratio))
        assert np.isfinite(g).all() and ratio <= 1.0, what
        cold = g[~hot]
        assert not cold.any() and not np.signbit(cold).any(), "%s: something other than +0.0 off the target channel" % what
        assert np.count_nonzero(g) > 0.5 * f["valid"], what


@pytest.mark.parametrize("mode", R.MODES)
def test_an_all_ignored_batch_is_a_zero_loss_with_a_zero_gradient(mode):
    name = "2x3x6x6 image boundary inside a workgroup"
    d = Device(name)
    d.target.t.fill_(IGN)
    d.predict.t[5] = float("nan")                                                      # nothing of an ignored pixel is looked at
    ctl, loss, g = d.run(2.0, mode)
    assert ctl["valid"] == 0 and ctl["bad"] == 0 and ctl["loss_sum"] == 0.0 and ctl["weight_sum"] == 0.0
    assert float(loss) == 0.0 and not np.signbit(loss) and ctl["loss"] == 0.0
    assert ctl["denom"] == (72.0 if mode == "pixels" else 0.0) and ctl["inv_denom"] == (float(np.float32(1.0) / np.float32(72.0)) if mode == "pixels" else 0.0)
    assert not g.any() and not np.signbit(g).any()


def test_a_nan_log_probability_poisons_loss_and_gradient_at_its_pixel_only():
    name = "2x4x5x7 scalar form"
    N, C, H, W, _, _ = CASES[name]
    for gamma in (0.0, 2.0, 0.5):
        d = Device(name)
        target = _operands(name)[1]
        n, y, x = [int(v[0]) for v in np.nonzero(target == 2)]
        d.predict.t.view(N, C, H, W)[n, 2, y, x] = float("nan")
        ctl, loss, g = d.run(gamma, "valid")
        assert np.isnan(loss) and np.isnan(ctl["loss_sum"]) and np.isnan(ctl["class_loss"][2]) and np.isfinite(ctl["class_loss"][1])
        assert np.isnan(g[n, 2, y, x]) and np.isnan(g).sum() == 1


def test_two_forwards_leave_the_same_bits():
    name = "1x3x1x%d second partial trip" % BIG_W
    d = Device(name)
    d.fwd(0.5, "weights")
    torch.cuda.synchronize()
    first, rows = d.ctl.t.clone(), d.ws.clone()
    d.ctl.t.fill_(float("nan"))
    d.ws.fill_(float("nan"))
    d.fwd(0.5, "weights")
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int64), d.ctl.t.view(torch.int64)) and torch.equal(rows.view(torch.int64), d.ws.view(torch.int64))
    assert K.read_ctl(first.cpu().numpy().tobytes())["valid"] == _reference(name, 0.5, "weights")["valid"]


def test_a_captured_pair_replays_on_operands_changed_in_place():
    """no launch argument depends on anything the device decides: forward and backward capture as they are, and the replay
    computes from what the buffers hold then"""
    name, other = "2x3x6x6 image boundary inside a workgroup", "2x3x6x6 views off 16-byte alignment"
    N, C, H, W, _, _ = CASES[name]
    d = Device(name)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d.fwd(2.0, "valid")
        d.bwd(2.0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(d.ctl.t).all()) and bool(torch.isnan(d.g.t).all())        # the capture ran nothing
    for case in (name, other):
        predict, target, pw, cw = _operands(case)
        d.predict.t.copy_(torch.from_numpy(predict).reshape(-1))
        d.target.t.copy_(torch.from_numpy(target).reshape(-1))
        d.pw.t.copy_(torch.from_numpy(pw).reshape(-1))
        d.cw.t.copy_(torch.from_numpy(cw))
        d.g.t.fill_(float("nan"))
        for b in d.everything():
            b.begin()
        graph.replay()
        torch.cuda.synchronize()
        for b in d.everything():
            b.check("replay on %s" % case, written=b in (d.g, d.ctl, d.loss))
        got_ctl, got_g = d.ctl.t.clone(), d.g.t.clone()
        fresh = Device(name)
        for src, dst in ((d.predict, fresh.predict), (d.target, fresh.target), (d.pw, fresh.pw), (d.cw, fresh.cw)):
            dst.t.copy_(src.t)
        fresh.run(2.0, "valid")
        assert torch.equal(got_ctl.view(torch.int64), fresh.ctl.t.view(torch.int64)), case
        assert torch.equal(got_g.view(torch.int32), fresh.g.t.view(torch.int32)), case
        f = R.forward(predict, target, pw, cw, IGN, 2.0, "valid")
        ctl = K.read_ctl(got_ctl.cpu().numpy().tobytes())
        assert ctl["valid"] == f["valid"] and ctl["bad"] == f["bad"] and abs(ctl["loss_sum"] - f["loss_sum"]) <= f["lim_sum"], case
