"""libubresnet_dice.so on the device, exactly: ubk_dice_fwd and ubk_dice_bwd over whole buffers between guard margins, at the
smallest shapes at which each path can go wrong (sizes from the header's geometry), against tests/dice_ref.py within its bound.

Operands: predict is a true fp32 log-softmax of seeded logits with a few target-channel entries forced to 0, to -inf, below the
underflow of expf and into its subnormal range; target holds every class (one kind of case: all but the last) and ignore_index,
some cases labels out of range; pixel and class weights are powers of two, so S and the weighted pixel counts are exact.  Counts are
exact; the sums, T, K1, K0, the loss and every gradient element lie within dice_ref's bound; every channel of a pixel that does not
contribute holds +0.0; nothing is written outside g_predict, ctl, loss and the rows of the workspace."""
import functools

import numpy as np
import pytest
import torch

import dice_ref as R
import kref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _dice as K
    from ubresnet_amd import _lib as L

DEV = "cuda"
IGN = -100
BIG_W = R.TRIP_PIXELS * R.MAX_GRID + R.TRIP_PIXELS + 12     # grid cap x trip, one more trip, a few pixels: two trips, the last partial
# name -> (N, C, H, W, offset elements of every view, labels out of range, the last class absent)
CASES = {
    "2x3x8x8 4-pixel form, one partial trip": (2, 3, 8, 8, 0, False, False),
    "1x3x5x7 scalar form": (1, 3, 5, 7, 0, True, False),
    "2x3x8x8 views off 16-byte alignment": (2, 3, 8, 8, 1, False, False),
    "2x3x6x6 bad labels": (2, 3, 6, 6, 0, True, False),
    "2x4x6x6 an absent class": (2, 4, 6, 6, 0, False, True),
    "1x1x1x%d two trips" % BIG_W: (1, 1, 1, BIG_W, 0, False, False),
    "1x3x1x%d two trips" % BIG_W: (1, 3, 1, BIG_W, 0, False, False),
}
for _c in (1, 2, 4, 5, 16):
    CASES["1x%dx8x8 4-pixel form" % _c] = (1, _c, 8, 8, 0, False, False)
    CASES["1x%dx5x7 scalar form" % _c] = (1, _c, 5, 7, 0, False, False)
SMALL = sorted(k for k in CASES if "two trips" not in k)
BIG = sorted(k for k in CASES if "two trips" in k)
PARAMS = [(a, b, e) for (a, b) in ((.5, .5), (.3, .7), (0., 1.), (1., 0.), (0., 0.)) for e in (1.0, 1e-6)]


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
    N, C, H, W, off, bad, absent = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if C > 1:
        predict = torch.log_softmax(4.0 * torch.randn(N, C, H, W, generator=g, dtype=torch.float32), dim=1)
    else:
        predict = -torch.rand(N, C, H, W, generator=g, dtype=torch.float32) * 3.0         # (a log-softmax over one class is all zeros)
    hw, n = H * W, N * H * W
    live = C - 1 if absent else C
    target = (torch.arange(n) % live)[torch.randperm(n, generator=g)].reshape(N, H, W)   # every class (but the absent one)
    pos = torch.randperm(n, generator=g)
    k = max(2, n // 16)
    target.view(-1)[pos[:k]] = IGN
    if bad:
        target.view(-1)[pos[k:k + 3]] = torch.tensor([C, -1, 1 << 40])
    # forced target-channel values: lp = 0 (q = 0), -inf, below the underflow of expf (p = 0), in its subnormal range, nearly 0
    for p, v in zip(pos[k + 3:k + 9].tolist(), (0.0, float("-inf"), -104.0, -110.0, -95.0, -1e-6)):
        i, r = divmod(p, hw)
        t = int(target.view(-1)[p])
        if 0 <= t < C:
            predict.view(N, C, hw)[i, t, r] = v
    pw = 2.0 ** torch.randint(-1, 3, (N, H, W), generator=g).float()
    cw = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float()
    return predict.numpy(), target.numpy(), pw.numpy(), cw.numpy()


@functools.lru_cache(maxsize=None)
def _sums(name):
    """dice_ref.sums of a case, computed once and shared by every parameter set"""
    predict, target, pw, _ = _operands(name)
    return R.sums(predict, target, pw, IGN)


_WS = []


def _workspace():
    """one workspace for the whole module, as the criterion shares one per device; two words in front and 16 behind are guards"""
    if not _WS:
        _WS.append(torch.full((K.WORKSPACE_BYTES // 8 + 18,), float("nan"), dtype=torch.float64, device=DEV))
    return _WS[0]


class Device:
    """the operands of a case in guarded device buffers, and the two calls"""

    def __init__(self, name, classw=True):
        self.N, self.C, self.H, self.W, off = CASES[name][:5]
        predict, target, pw, cw = _operands(name)
        self.predict, self.target, self.pw = Guard(predict, off), Guard(target, off), Guard(pw, off)
        self.cw = Guard(cw) if classw else None
        self.g = Guard(np.full(predict.size, np.nan, np.float32), off)
        self.ws = _workspace()
        self.ctl = Guard(np.full(K.CTL_WORDS, np.nan, np.float64))
        self.loss = Guard(np.full(1, np.nan, np.float32))
        self.g_loss = Guard(np.ones(1, np.float32))
        self.what = name

    def everything(self):
        return [b for b in (self.predict, self.target, self.pw, self.cw, self.g, self.ctl, self.loss, self.g_loss) if b is not None]

    def fwd(self, alpha=0.5, beta=0.5, eps=1.0, present_only=True):
        K.dice_fwd(self.predict.ptr(), self.target.ptr(), self.pw.ptr(), None if self.cw is None else self.cw.ptr(), self.N, self.C, self.H,
                   self.W, IGN, alpha, beta, eps, present_only, self.ws[2:].data_ptr(), self.ctl.ptr(), self.loss.ptr(), L.stream_ptr())

    def bwd(self):
        K.dice_bwd(self.g_loss.ptr(), self.ctl.ptr(), self.predict.ptr(), self.target.ptr(), self.pw.ptr(), self.N, self.C, self.H, self.W, IGN,
                   self.g.ptr(), L.stream_ptr())

    def run(self, alpha=0.5, beta=0.5, eps=1.0, present_only=True, g_loss=1.0):
        """forward and backward with every buffer's margins (and every input) checked -> (ctl dict, loss fp32, g [N,C,H,W] numpy)"""
        self.g_loss.t.fill_(g_loss)
        self.g.t.fill_(float("nan"))
        self.ctl.t.fill_(float("nan"))
        for b in self.everything():
            b.begin()
        rows = K.grid(self.N * self.H * self.W) * K.ROW_WORDS
        self.ws.fill_(float("nan"))
        self.fwd(alpha, beta, eps, present_only)
        self.bwd()
        torch.cuda.synchronize()
        for b in self.everything():
            b.check("%s %s" % (self.what, (alpha, beta, eps, present_only)), written=b in (self.g, self.ctl, self.loss))
        # the workspace: the rows of the grid are written whole, nothing behind them, nothing in front
        assert bool(torch.isnan(self.ws[:2]).all()) and bool(torch.isnan(self.ws[2 + rows:]).all()), self.what
        assert not bool(torch.isnan(self.ws[2:2 + rows].view(-1, K.ROW_WORDS)[:, :K.ROW["PIXELS"]]).any()) or not np.isfinite(self.loss.t.item())
        ctl = K.read_ctl(self.ctl.t.cpu().numpy().tobytes())
        return ctl, self.loss.t.cpu().numpy()[0], self.g.t.cpu().numpy().reshape(self.N, self.C, self.H, self.W)


def _within(got, want, lim, what):
    got, want, lim = (np.asarray(v, dtype=np.float64) for v in (got, want, lim))
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        ratio = float(np.where(err == 0, 0.0, err / lim).max())
    print("%s: worst error / bound %.3f" % (what, ratio))
    assert np.isfinite(got).all() and ratio <= 1.0, what
    return ratio


def _check(name, f, ctl, loss, g, g_loss, what):
    """everything a forward and backward pair left against the reference dict f"""
    C = CASES[name][1]
    assert ctl["valid"] == f["valid"] and ctl["bad"] == f["bad"] and ctl["pixels"] == f["pixels"] + [0] * (16 - C), what
    for key in ("tp", "fp", "fn", "T", "k1", "k0"):
        assert ctl[key][C:] == [0.0] * (16 - C), "%s: %s of a class >= C" % (what, key)
    assert ctl["S"] == f["S"], what                                                     # powers of two: exact
    for key in ("tp", "fp", "fn"):
        _within(ctl[key][:C], f[key], f["d_" + key], "%s %s" % (what, key.upper()))
    _within(ctl["T"][:C], f["T"], f["lim_T"], what + " T")
    _within(ctl["k1"][:C], f["K1"], f["lim_K1"], what + " K1")
    _within(ctl["k0"][:C], f["K0"], f["lim_K0"], what + " K0")
    _within([loss], [f["loss"]], [f["lim_loss"]] if f["lim_loss"] > 0 else [1.0], what + " loss")
    assert np.float32(ctl["loss"]).view(np.uint32) == np.float32(loss).view(np.uint32), what
    assert all(k <= 0.0 for k in ctl["k1"]) and all(k >= 0.0 for k in ctl["k0"]), what
    want, lim, ok = R.backward(g_loss, f)
    hot = np.broadcast_to(ok[:, None], g.shape)
    _within(g[hot], want[hot], lim[hot], what + " gradient")
    assert not g.view(np.uint32)[~hot].any(), "%s: something other than +0.0 at a pixel that does not contribute" % what


def test_the_cases_cover_the_paths_of_the_launch():
    assert (K.BLOCK, K.UNROLL, K.MAX_GRID, K.REG_CLASSES) == (R.BLOCK, R.UNROLL, R.MAX_GRID, R.REG_CLASSES)
    shape = {k: v[:4] for k, v in CASES.items()}
    vec = {k: (h * w) % 4 == 0 and CASES[k][4] == 0 for k, (n, c, h, w) in shape.items()}
    # every instantiation of the forward: C = 1 .. REG_CLASSES and above, in both forms
    for form in (True, False):
        assert {min(c, K.REG_CLASSES + 1) for k, (n, c, h, w) in shape.items() if vec[k] == form} == set(range(1, K.REG_CLASSES + 2)), form
    assert max(c for n, c, h, w in shape.values()) == K.MAX_CLASSES
    assert any(CASES[k][4] == 1 and (shape[k][2] * shape[k][3]) % 4 == 0 for k in CASES)       # the scalar form by alignment alone
    assert K.grid(2 * 8 * 8) == 1 and 2 * 8 * 8 < K.TRIP_PIXELS                                # one partial trip
    for name in BIG:
        n, c, h, w = shape[name]
        trips = -(-n * h * w // K.TRIP_PIXELS)
        assert K.grid(n * h * w) == K.MAX_GRID and trips == K.MAX_GRID + 2 and 0 < n * h * w % K.TRIP_PIXELS < 64 and vec[name]
    assert sorted(shape[k][1] for k in BIG) == [1, 3]
    for name in CASES:
        predict, target, pw, cw = _operands(name)
        N, C, H, W, off, bad, absent = CASES[name]
        s = _sums(name)
        assert all(n > 0 for n in s["pixels"][:C - 1]) and (s["pixels"][C - 1] > 0) == (not absent) and (target == IGN).sum() >= 2, name
        assert s["bad"] == (3 if bad else 0), name
        lp = np.take_along_axis(predict.reshape(N, C, H * W), np.clip(target, 0, C - 1).reshape(N, 1, H * W), axis=1).reshape(-1)[s["ok"].reshape(-1)]
        assert (lp == 0).any() and np.isneginf(lp).any() and (lp == -104).any(), name
        assert set(np.log2(pw).reshape(-1).tolist()) <= {-1.0, 0.0, 1.0, 2.0} and set(np.log2(cw).tolist()) <= {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("name", SMALL)
def test_sums_finish_and_gradient_lie_within_the_bound(name):
    d = Device(name)
    cw = _operands(name)[3]
    for i, (alpha, beta, eps) in enumerate(PARAMS):
        for present_only in ((True, False) if CASES[name][6] or i == 0 else (True,)):
            what = "%s alpha %g beta %g eps %g present_only %d" % (name, alpha, beta, eps, present_only)
            f = R.complete(_sums(name), cw, alpha, beta, eps, present_only)
            ctl, loss, g = d.run(alpha, beta, eps, present_only, g_loss=0.5)
            _check(name, f, ctl, loss, g, 0.5, what)
            assert f["loss"] == 0.0 or np.count_nonzero(g) > 0.5 * f["valid"], what
    # without class weights
    d = Device(name, classw=False)
    ctl, loss, g = d.run(0.3, 0.7, 1.0, True)
    _check(name, R.complete(_sums(name), None, 0.3, 0.7, 1.0, True), ctl, loss, g, 1.0, name + " no class weights")


@pytest.mark.parametrize("name", BIG)
def test_workgroups_that_take_two_trips(name):
    d = Device(name)
    cw = _operands(name)[3]
    for alpha, beta, eps in ((0.5, 0.5, 1.0), (0.3, 0.7, 1e-6)):
        ctl, loss, g = d.run(alpha, beta, eps, True)
        _check(name, R.complete(_sums(name), cw, alpha, beta, eps, True), ctl, loss, g, 1.0, "%s alpha %g" % (name, alpha))
    assert ctl["valid"] > K.MAX_GRID * K.TRIP_PIXELS * 0.9


def test_an_absent_class_with_and_without_present_only():
    name = "2x4x6x6 an absent class"
    d = Device(name)
    cw = _operands(name)[3]
    on = d.run(0.5, 0.5, 1.0, True)[0]
    off = d.run(0.5, 0.5, 1.0, False)[0]
    assert on["pixels"][3] == 0 and on["tp"][3] == 0.0 and on["fn"][3] == 0.0 and on["fp"][3] > 0.0
    assert on["S"] == float(cw[:3].sum()) and off["S"] == float(cw.sum())
    assert on["k1"][3] == 0.0 and on["k0"][3] == 0.0 and off["k0"][3] > 0.0              # left out of the mean / pulls its false positives down
    assert on["T"][3] == off["T"][3] == 1.0 / (0.5 * on["fp"][3] + 1.0)
    # eps = 0 and no price on false positives: Dn == 0 -> T = 1 and zero coefficients, nothing is NaN
    ctl, loss, g = d.run(0.0, 1.0, 0.0, False)
    _check(name, R.complete(_sums(name), cw, 0.0, 1.0, 0.0, False), ctl, loss, g, 1.0, name + " Dn == 0")
    assert ctl["T"][3] == 1.0 and ctl["k1"][3] == 0.0 and ctl["k0"][3] == 0.0 and np.isfinite(loss) and np.isfinite(g).all()
    # eps = 0 with a price on them: T = 0, and the class costs its whole share
    ctl, loss, g = d.run(0.5, 0.5, 0.0, False)
    _check(name, R.complete(_sums(name), cw, 0.5, 0.5, 0.0, False), ctl, loss, g, 1.0, name + " eps 0")
    assert ctl["T"][3] == 0.0 and ctl["k0"][3] == 0.0 and loss >= float(cw[3] / cw.sum())


def test_zero_class_weights():
    name = "2x3x8x8 4-pixel form, one partial trip"
    d = Device(name)
    cw = _operands(name)[3].copy()
    cw[1] = 0.0
    d.cw.t.copy_(torch.from_numpy(cw))
    ctl, loss, g = d.run(0.3, 0.7, 1.0, True)
    _check(name, R.complete(_sums(name), cw, 0.3, 0.7, 1.0, True), ctl, loss, g, 1.0, name + " one zero class weight")
    assert ctl["k1"][1] == 0.0 and ctl["k0"][1] == 0.0 and 0.0 < ctl["T"][1] < 1.0 and not g[:, 1].any() and g[:, 0].any()
    d.cw.t.zero_()
    ctl, loss, g = d.run(0.3, 0.7, 1.0, False)
    assert ctl["S"] == 0.0 and np.float32(loss).view(np.uint32) == 0 and not g.view(np.uint32).any(), "all class weights zero: loss 0, gradient +0.0"
    assert ctl["k1"] == [0.0] * 16 and ctl["k0"] == [0.0] * 16 and ctl["valid"] == _sums(name)["valid"] and 0.0 < ctl["T"][0] < 1.0


@pytest.mark.parametrize("present_only", [True, False])
def test_an_all_ignored_batch_is_a_zero_loss_with_a_zero_gradient(present_only):
    name = "2x3x6x6 bad labels"
    d = Device(name)
    d.target.t.fill_(IGN)
    d.predict.t[5] = float("nan")                                                      # nothing of an ignored pixel is looked at
    ctl, loss, g = d.run(0.5, 0.5, 0.0, present_only)
    assert ctl["valid"] == 0 and ctl["bad"] == 0 and ctl["pixels"] == [0] * 16 and ctl["tp"] == ctl["fp"] == ctl["fn"] == [0.0] * 16
    assert np.float32(loss).view(np.uint32) == 0 and ctl["loss"] == 0.0 and not g.view(np.uint32).any()
    assert ctl["S"] == (0.0 if present_only else float(_operands(name)[3].sum())) and ctl["T"][:3] == [1.0] * 3     # Dn == 0 everywhere
    assert ctl["k1"] == [0.0] * 16 and ctl["k0"] == [0.0] * 16


def test_a_nan_log_probability_poisons_its_channel_and_no_other():
    name = "1x3x5x7 scalar form"
    N, C, H, W = CASES[name][:4]
    s = _sums(name)
    target = _operands(name)[1]
    n, y, x = [int(v[0]) for v in np.nonzero(target == 2)]
    for channel in (2, 0):                                                             # at the pixel's target channel; at another one
        d = Device(name)
        d.predict.t.view(N, C, H, W)[n, channel, y, x] = float("nan")
        ctl, loss, g = d.run(0.5, 0.5, 1.0, True)
        assert np.isnan(loss) and np.isnan(ctl["T"][channel]) and np.isnan(ctl["k1"][channel]) and np.isnan(ctl["k0"][channel])
        hot = s["ok"]
        assert np.isnan(g[:, channel][hot]).all(), "channel %d: NaN at every contributing pixel" % channel
        others = [c for c in range(C) if c != channel]
        assert np.isfinite(g[:, others]).all() and np.isfinite([ctl["T"][c] for c in others]).all() and g[:, others].any()
        assert not g.view(np.uint32)[np.broadcast_to(~hot[:, None], g.shape)].any()
        assert ctl["valid"] == s["valid"] and ctl["pixels"][:C] == s["pixels"]
    # a NaN in a pixel that does not contribute is never looked at
    d = Device(name)
    n, y, x = [int(v[0]) for v in np.nonzero(target == IGN)]
    d.predict.t.view(N, C, H, W)[n, :, y, x] = float("nan")
    ctl, loss, g = d.run(0.5, 0.5, 1.0, True)
    _check(name, R.complete(s, _operands(name)[3], 0.5, 0.5, 1.0, True), ctl, loss, g, 1.0, name + " NaN in an ignored pixel")


def test_two_calls_leave_the_same_bits_with_the_workspace_reused_in_between():
    name, other = "1x3x1x%d two trips" % BIG_W, "1x5x8x8 4-pixel form"
    d, o = Device(name), Device(other)
    assert d.ws is o.ws
    d.run(0.3, 0.7, 1e-6, True)
    first_ctl, first_g, first_loss = d.ctl.t.clone(), d.g.t.clone(), d.loss.t.clone()
    o.run(0.5, 0.5, 1.0, False)
    d.run(0.3, 0.7, 1e-6, True)
    assert torch.equal(first_ctl.view(torch.int64), d.ctl.t.view(torch.int64)) and torch.equal(first_loss.view(torch.int32), d.loss.t.view(torch.int32))
    assert torch.equal(first_g.view(torch.int32), d.g.t.view(torch.int32))
