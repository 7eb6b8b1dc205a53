"""Edge values through every store, load and compare path, bit for bit (GPU).

The exact suites (test_gpu_kernels_exact / _stream_exact / _param_exact / _frozen) draw every operand from
kref.exact_operands(): small dyadic numbers, so no store ever sees a rounding tie of the storage type, an overflow, a subnormal,
a signed zero, an infinity or a NaN.  Here the value under test enters a kernel's fp32 path through an fp32 PER-CHANNEL operand
(a conv bias, a BatchNorm shift, k1 of the apply pass, a frozen scale) while the data operands contribute exactly nothing (zeros)
or exactly one term, so the fp64 reference is the value itself and the expected store is value.float().to(dtype) -- torch's
conversion: round to nearest even, subnormals kept, NaN stays NaN.  One launch checks C values at every pixel, so every lane,
quad and fragment position of a store path sees every class (kref.edge_table).  Comparisons are on bit patterns
(kref.assert_bits); where the formula itself leaves the sign of a zero open (max(-0, +0), (+0) + (-0) under a fused or unfused
form) the sign of zero is not compared, and only there.

NaN at the compares (ReLU = max(v, 0), max-pool, the [bn(c) > 0] gates) is characterised: every case records what came out, and
asserts (a) that every kernel variant and dtype of one operation does the same thing and (b) that nothing outside the element's
own output changed.  Each case prints one table row (`EDGE | operation | kernel | dtype | classes | verdict`).
"""
import pytest
import torch

import kref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import ops
    from ubresnet_amd.ops import Affine

DEV = "cuda"
DTS = [torch.float32, torch.bfloat16, torch.float16]
TNAME = {torch.float32: "float", torch.bfloat16: "bf16_t", torch.float16: "f16_t"}
FLT_MAX = float(torch.finfo(torch.float32).max)
NONFINITE = kref.NAN_CLASSES + ("inf",)
SLOTS = 32


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """a faulted device fails every later launch: end the session instead of starting more work on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test, nothing more is launched: %s" % e, returncode=3)


def row(op, kernel, dt, classes, verdict):
    print("EDGE | %-34s | %-58s | %-6s | %-44s | %s" % (op, kernel, TNAME[dt], classes, verdict))


def chunks(v, n):
    """the table cut into vectors of n values (the last one wraps round)"""
    m = (v.numel() + n - 1) // n
    idx = torch.arange(m * n) % v.numel()
    return v[idx].view(m, n)


def cycle(v, shape, step=1):
    """a tensor of `shape` whose flat element i is v[(i * step) % len(v)]: neighbouring lanes hold different classes"""
    n = 1
    for s in shape:
        n *= s
    return v[(torch.arange(n) * step) % v.numel()].view(shape)


def t_edges(dt, exclude=()):
    """the edge table rounded to dt: every interesting bit pattern OF the storage type (fp32: the table itself)"""
    return kref.edge_values(dt, exclude=exclude).to(dt)


class Guard:
    """an NHWC output view inside a sentinel-filled kref.Buffers group: contiguous, or a channel slice of a wider pixel"""

    def __init__(self, shape, dt, sliced=False, gid="out"):
        N, H, W, C = shape
        ps, off = (C + 32, 16) if sliced else (C, 0)
        self.tv = kref.TV.make(shape, (H * W * ps, W * ps, ps, 1), dt, gid, off * kref.ESZ[dt])
        self.B = kref.Buffers([self.tv], DEV)
        if sliced:         # the buffer has to span the whole last pixel
            g = self.B.groups[gid]
            need = g["m"] + N * H * W * ps + 64
            if g["buf"].numel() < need:
                g["buf"] = torch.full((need,), float("nan"), dtype=dt, device=DEV)
                g["written"] = torch.zeros(need, dtype=torch.bool, device=DEV)
        self.t = self.B.view(self.tv)
        self.B.mark_written(self.tv)
        self.snap = self.B.snapshot()

    def check(self, what):
        self.B.check_sentinel(self.snap, what)


def statbuf(n):
    return torch.zeros(SLOTS * n, dtype=torch.float64, device=DEV)


# ----------------------------------------------------------------------------------------------------------------------
# ubr_conv store paths
# ----------------------------------------------------------------------------------------------------------------------
# id: (H, W, Cin for 16-bit types, Cin for fp32 (None: no such kernel), Cout, k, tile_hint, channel-sliced output, kernel symbol)
CONV_PATHS = {
    "igemm_fast": (16, 32, 32, 32, 32, 3, 7, False, "conv_igemm_kernel<%s, 2, 2, 1, false>"),
    "igemm_ragged_sliced": (12, 20, 32, 32, 32, 3, 7, True, "conv_igemm_kernel<%s, 2, 2, 1, false>"),
    "igemm_pipe": (16, 32, 64, 64, 64, 3, 5, False, "conv_igemm_kernel<%s, 2, 4, 1, true>"),
    "thin_upb2": (16, 32, 16, 8, 16, 3, 2, False, "conv_thin_kernel<%s, 4, 1, 2, 2, false, false, false, 0>"),
    "thin_upb4": (16, 32, 32, 16, 32, 3, 3, False, "conv_thin_kernel<%s, 4, 2, 2, 4, false, false, false, 0>"),
    "thin_row7": (16, 32, 16, None, 16, 7, 1, False, "conv_thin_kernel<%s, 8, 1, 2, 2, false, false, true, 0>"),
    "pc": (16, 32, 64, 64, 128, 3, 103, False, "conv_pc_kernel<%s, 4, 1, 9>"),
}
CONV_PARAMS = [(p, dt) for p in CONV_PATHS for dt in DTS if not (dt == torch.float32 and CONV_PATHS[p][3] is None)]
CONV_IDS = ["%s-%s" % (p, TNAME[dt]) for p, dt in CONV_PARAMS]


class ConvPath:
    def __init__(self, path, dt, seed=7):
        H, W, c16, c32, Cout, k, hint, sliced, sym = CONV_PATHS[path]
        self.H, self.W, self.Cout, self.k, self.hint, self.sliced, self.dt = H, W, Cout, k, hint, sliced, dt
        self.Cin = c32 if dt == torch.float32 else c16
        self.sym = sym % TNAME[dt]
        self.taps = ops.conv_taps(k, 1, k // 2)
        g = torch.Generator().manual_seed(seed)
        w = torch.randn(Cout, self.Cin, k, k, generator=g)          # finite, non-zero weights over a zero input
        self.wp = ops.pack_weights(w.to(DEV), dt, Cout, self.Cin, self.Cin * k * k, k * k, k * k)
        self.x = torch.zeros((1, H, W, self.Cin), dtype=dt, device=DEV)

    def run(self, bias, addend=None, act=0, bnb=None, stats=None):
        """-> (stored output on the CPU); bias fp32 CPU [Cout]; checks the kernel symbol and the sentinels"""
        out = Guard((1, self.H, self.W, self.Cout), self.dt, self.sliced)
        ops.conv(self.x, self.wp, out.t, self.taps, self.Cout, bias=bias.to(DEV), addend=addend, act=act, tile_hint=self.hint, bnb=bnb, stats=stats)
        torch.cuda.synchronize()
        self.name = ops.last_conv_kernel()
        out.check(self.name)
        return out.t.cpu()

    def expected(self, bias, addend=None, act=0):
        """the epilogue's fp32 statements on the CPU: v = acc(+0) + bias; relu; v += addend; relu; one rounding to dt"""
        v = (torch.zeros((1, self.H, self.W, self.Cout)) + bias.view(1, 1, 1, -1)).float()
        if act & 1:
            v = torch.where(v > 0, v, torch.zeros(()))
        if addend is not None:
            v = v + addend.cpu().float()
        if act & 2:
            v = torch.where(v > 0, v, torch.zeros(()))
        return v.to(self.dt)


@pytest.mark.parametrize("path,dt", CONV_PARAMS, ids=CONV_IDS)
def test_conv_store_of_edge_biases(path, dt):
    """x = 0, bias = the edge table, act = 0: every stored element equals bias.to(dt) in bits (a NaN comes out a NaN)"""
    cp = ConvPath(path, dt)
    for b in chunks(kref.edge_values(dt), cp.Cout):
        got = cp.run(b)
        assert cp.name == cp.sym, "%s: launched %s, wanted %s" % (path, cp.name, cp.sym)
        kref.assert_bits(got, cp.expected(b), what="%s bias store" % cp.name)
    row("conv store, bias=edge " + path, cp.name, dt, "all %d (ties, overflow, subnormal, 0, inf, NaN)" % len(kref.edge_names(dt)), "bit-equal")


@pytest.mark.parametrize("path,dt", CONV_PARAMS, ids=CONV_IDS)
def test_conv_addend_load_and_store_of_edge_values(path, dt):
    """x = 0, bias = 0, addend = every edge bit pattern of dt: load of T + store of T returns the same value ((+0) + (-0) = +0)"""
    cp = ConvPath(path, dt)
    ad = cycle(t_edges(dt), (1, cp.H, cp.W, cp.Cout), step=1).to(DEV)
    adv = torch.zeros((1, cp.H, cp.W, cp.Cout + 8), dtype=dt, device=DEV)         # the addend as a channel slice as well
    adv[..., :cp.Cout] = ad
    zero = torch.zeros(cp.Cout)
    got = cp.run(zero, addend=adv[..., :cp.Cout])
    assert cp.name == cp.sym
    kref.assert_bits(got, cp.expected(zero, ad), what="%s addend" % cp.name)
    row("conv addend=T edge " + path, cp.name, dt, "all T bit patterns of the table", "bit-equal")


@pytest.mark.parametrize("path,dt", CONV_PARAMS, ids=CONV_IDS)
def test_conv_activations_on_finite_and_infinite_edges(path, dt):
    """act = 1, 2, 3 with bias = finite and infinite edges and a finite T addend (no inf - inf); max(-0, +0) leaves the zero sign open"""
    cp = ConvPath(path, dt)
    ad = cycle(t_edges(dt, exclude=NONFINITE + ("flt_max", "overflow_tie")), (1, cp.H, cp.W, cp.Cout), step=3)
    ad = torch.where(torch.isfinite(ad), ad, torch.zeros((), dtype=dt)).to(DEV)
    for act in (1, 2, 3):
        for b in chunks(kref.edge_values(dt, exclude=kref.NAN_CLASSES), cp.Cout):
            got = cp.run(b, addend=ad, act=act)
            exp = cp.expected(b, ad, act)
            assert not bool(torch.isnan(exp.float()).any())
            kref.assert_bits(got, exp, zero_sign=False, what="%s act %d" % (cp.name, act))
    assert cp.name == cp.sym
    row("conv act=1,2,3 " + path, cp.name, dt, "finite + inf biases, finite T addend", "bit-equal")


BNB_PATHS = {
    "igemm_finish": ("igemm_fast", "conv_igemm_kernel<%s, 2, 2, 1, false>"),
    "thin_upb2_ext1": ("thin_upb2", "conv_thin_kernel<%s, 4, 1, 2, 2, false, false, false, 1>"),
    "thin_upb4_ext1": ("thin_upb4", "conv_thin_kernel<%s, 4, 2, 2, 4, false, false, false, 1>"),
    "thin_row7_ext1": ("thin_row7", "conv_thin_kernel<%s, 8, 1, 2, 2, false, false, true, 1>"),
}
BNB_PARAMS = [(p, dt) for p in BNB_PATHS for dt in DTS if not (dt == torch.float32 and CONV_PATHS[BNB_PATHS[p][0]][3] is None)]


@pytest.mark.parametrize("path,dt", BNB_PARAMS, ids=["%s-%s" % (p, TNAME[dt]) for p, dt in BNB_PARAMS])
def test_conv_bnb_sums_are_those_of_the_stored_gradient(path, dt):
    """bnb_c: the gate [bn(c) > 0] is open at ONE pixel per channel (c = 1 there, -1 elsewhere; mean 0, scale 1, shift 0, invstd 1),
    so both sums of a channel are its stored g = bias.to(dt) exactly, whatever the summation order: round4<T> against the real store.
    Finite edges, with the ties, the values that round to 0 and the ones that round to the largest finite (and to inf)."""
    base, sym = BNB_PATHS[path]
    cp = ConvPath(base, dt)
    npix, C = cp.H * cp.W, cp.Cout
    c = torch.full((1, cp.H, cp.W, C), -1.0, dtype=dt)
    pix = (7 * torch.arange(C) + 3) % npix
    c.view(npix, C)[pix, torch.arange(C)] = 1.0
    c = c.to(DEV)
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    for b in chunks(kref.edge_values(dt, exclude=NONFINITE), C):
        red = statbuf(2 * C)
        got = cp.run(b, bnb=(c, zero, one, zero, one), stats=red)
        assert cp.name == sym % TNAME[dt], "%s: launched %s" % (path, cp.name)
        exp = cp.expected(b)
        kref.assert_bits(got, exp, what="%s store" % cp.name)
        s = red.view(SLOTS, 2 * C).sum(0).cpu()
        g = b.to(dt).double()
        # (an overflowed g = inf sums to inf; 0 * anything never enters: the closed gate selects 0.f)
        for nm, a in (("sum g_y", s[:C]), ("sum g_y*xhat", s[C:])):
            assert torch.equal(a, g), "%s: %s: channel %d: got %r, stored g %r (bias %r)" % (
                cp.name, nm, int((a != g).nonzero()[0]), float(a[(a != g).nonzero()[0]]), float(g[(a != g).nonzero()[0]]), float(b[(a != g).nonzero()[0]]))
    row("conv bnb_c sums = stored g " + path, cp.name, dt, "finite edges: ties, ->0, ->max, ->inf, subnormal", "equal")


def test_conv_two_phase_launch_stores_edge_biases():
    """a 2-phase launch (two of the four phases of ConvTranspose2d(k4, s2, p1)): the phase pixels hold bias.to(dt), the others keep the sentinel"""
    for dt in DTS:
        Cin, Cout, H, W = 32, 32, 8, 16
        w = torch.randn(Cout, Cin, 4, 4, generator=torch.Generator().manual_seed(3))
        wp = ops.pack_weights(w.to(DEV), dt, Cout, Cin, Cin * 16, 16, 16)
        x = torch.zeros((1, H, W, Cin), dtype=dt, device=DEV)
        phases = [(0, rx, ops.transposed_phase_taps(4, 1, 1, 2, 0, rx)) for rx in range(2)]
        for b in chunks(kref.edge_values(dt), Cout):
            out = Guard((1, 2 * H, 2 * W, Cout), dt, sliced=True)
            before = out.t.clone()
            ops.conv_phases(x, wp, out.t[:, 0::2, 0::2, :], [t for p in phases for t in p[2]], Cout, phases=phases, y_full=out.t, bias=b.to(DEV))
            torch.cuda.synchronize()
            name = ops.last_conv_kernel()
            out.check(name)
            exp = (torch.zeros((1, H, 2 * W, Cout)) + b).to(dt)
            kref.assert_bits(out.t[:, 0::2].cpu(), exp, what="%s phases" % name)
            kref.assert_bits(out.t[:, 1::2].cpu(), before[:, 1::2].cpu(), what="%s rows of the phases not launched" % name)
        assert name.startswith(("conv_thin_kernel", "conv_igemm_kernel"))
        row("conv 2-phase store, bias=edge", name, dt, "all", "bit-equal")


# ----------------------------------------------------------------------------------------------------------------------
# loads: T-typed subnormal, largest-finite and infinite inputs through a 1x1 conv, with and without BatchNorm-on-load
# ----------------------------------------------------------------------------------------------------------------------
LOAD_PATHS = {"igemm": (32, 32, 32, 7, "conv_igemm_kernel"), "thin": (32, 16, 32, 3, "conv_thin_kernel"), "pc": (64, 64, 64, 103, "conv_pc_kernel")}


@pytest.mark.parametrize("dt", DTS, ids=[TNAME[d] for d in DTS])
@pytest.mark.parametrize("path", list(LOAD_PATHS))
def test_conv_loads_of_edge_inputs(path, dt):
    """1x1 conv: one-hot weights on finite T edges (out[co] = x[co]: subnormals survive the MFMA), strictly positive weights on
    infinities; raw, and through ubr_bnrelu with lo = 0 and lo = -FLT_MAX.  Reference: kref.conv_ref (fp64), rounded once."""
    c16, c32, _, hint, fam = LOAD_PATHS[path]
    Cin = c32 if dt == torch.float32 else c16
    Cout, H, W = (64 if path == "pc" else 32), 16, 32
    taps = [(0, 0, 0)]
    fin = t_edges(dt, exclude=NONFINITE + ("flt_max", "overflow_tie"))
    fin = fin[torch.isfinite(fin)]
    xfin = cycle(fin, (1, H, W, Cin), step=1)
    xinf = torch.ones((1, H, W, Cin), dtype=dt)
    p = torch.arange(H * W)
    xinf.view(H * W, Cin)[p, p % Cin] = torch.where(p % 2 == 0, float("inf"), float("-inf")).to(dt)
    w_hot = torch.zeros(Cout, Cin, 1, 1)
    w_hot[torch.arange(Cout), torch.arange(Cout) % Cin] = 1.0
    w_pos = torch.full((Cout, Cin, 1, 1), 0.5)
    one, zero = torch.ones(Cin), torch.zeros(Cin)
    for xin, w, tag in ((xfin, w_hot, "finite, one-hot"), (xinf, w_pos, "inf, positive weights")):
        wp = ops.pack_weights(w.to(DEV), dt, Cout, Cin, Cin, 1, 1)
        for lo in (None, 0.0, -FLT_MAX):
            xfr = None if lo is None else (zero, one, zero, torch.full((Cin,), lo))
            out = Guard((1, H, W, Cout), dt)
            ops.conv(xin.to(DEV), wp, out.t, taps, Cout, xf=None if xfr is None else Affine(*[t.to(DEV) for t in xfr]), tile_hint=hint)
            torch.cuda.synchronize()
            name = ops.last_conv_kernel()
            assert name.startswith(fam), name
            out.check(name)
            # (the transformed operand is rounded to dt before it enters the MFMA: max(-inf, -FLT_MAX) is -inf again in bf16 / f16)
            xr = kref._xform(xin, xfr).float().to(dt)
            ref, _ = kref.conv_ref(xr, kref.pack_dense(w, range(1)), taps, Cout, H, W, want_abs=False)
            kref.assert_bits(out.t.cpu(), ref.float().to(dt), zero_sign=False, what="%s %s lo=%r" % (name, tag, lo))
    row("conv 1x1 loads (+bnrelu lo=0,-FLT_MAX) " + path, name, dt, "T subnormal, max finite, +-inf", "bit-equal")


# ----------------------------------------------------------------------------------------------------------------------
# log-softmax epilogue: logit spreads past the expf underflow point
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=[TNAME[d] for d in DTS])
def test_conv_logsoftmax_epilogue_past_the_expf_underflow(dt):
    N, H, W, Cin, Cout = 1, 16, 32, 16, 4
    w = torch.randn(Cout, Cin, 7, 7, generator=torch.Generator().manual_seed(5))
    wp = ops.pack_weights(w.to(DEV), dt, Cout, Cin, Cin * 49, 49, 49)
    x = torch.zeros((N, H, W, Cin), dtype=dt, device=DEV)
    for logits in ([0.0, -90.0, -104.0, -120.0], [100.0, -10.0, -5.0, 99.5], [-200.0, -200.0, -200.5, -330.0], [3.0e4, -3.0e4, 0.0, 2.9e4]):
        b = torch.tensor(logits)
        y = torch.full((N, Cout, H, W), float("nan"), device=DEV)
        ops.conv(x, wp, y, ops.conv_taps(7, 1, 3), Cout, bias=b.to(DEV), logsoftmax=True)
        torch.cuda.synchronize()
        ref, lim = kref.logsoftmax_ref(b.double().view(1, 1, 1, Cout).expand(N, H, W, Cout))
        kref.assert_within(y.permute(0, 2, 3, 1).cpu(), ref, lim, "%s logits %r" % (ops.last_conv_kernel(), logits))
    row("conv log-softmax epilogue", ops.last_conv_kernel(), dt, "spreads 120, 530, 6e4 (expf underflows)", "within kref.logsoftmax_ref")


# ----------------------------------------------------------------------------------------------------------------------
# streaming kernels (2 x 8 x 16 pixels, C = 16 and 96, contiguous and channel-sliced)
# ----------------------------------------------------------------------------------------------------------------------
SHAPE = (2, 8, 16)
STREAM = [(C, dt, sl) for C in (16, 96) for dt in DTS for sl in (False, True)]
STREAM_IDS = ["C%d-%s-%s" % (C, TNAME[dt], "sliced" if sl else "dense") for C, dt, sl in STREAM]


def dev(*ts):
    return [t.to(DEV) for t in ts]


def sliced_in(t, sl):
    """the input tensor t (NHWC, on the device) as a dense tensor or as a channel slice of a wider one"""
    if not sl:
        return t.to(DEV).contiguous()
    C = t.shape[-1]
    buf = torch.full(t.shape[:3] + (C + 16,), float("nan"), dtype=t.dtype, device=DEV)
    buf[..., 8:8 + C] = t.to(DEV)
    return buf[..., 8:8 + C]


def relu32(v):
    return torch.where(v > 0, v, torch.zeros(()))


@pytest.mark.parametrize("C,dt,sl", STREAM, ids=STREAM_IDS)
def test_block_tail_forward_stores_and_mask(C, dt, sl):
    """c2 = 0, mean = 0, scale = 1, shift = edge values, identity shortcut 0: out = relu(relu(shift) + 0) rounded once; the mask byte
    is [STORED output > 0] -- a value > 0 in fp32 that is stored as 0 has its bit clear.  Plain, masked and finalize-fused forms;
    then the data operand: c2 = T edges with shift = 0."""
    N, H, W = SHAPE
    cpu_ = kref.CPU[dt]
    z = torch.zeros((N, H, W, C), dtype=dt)
    vals = kref.edge_values(dt, exclude=kref.NAN_CLASSES)
    vecs = [(z, s) for s in chunks(vals, C)] + [(cycle(t_edges(dt, exclude=kref.NAN_CLASSES), (N, H, W, C)), torch.zeros(C))]
    had_lost = False
    for c2h, shift in vecs:
        exp = relu32(relu32(c2h.float() + shift) + 0.0).to(dt)
        lost = (relu32(c2h.float() + shift) > 0) & (exp.float() == 0)
        had_lost |= bool(lost.any())
        expm = kref.mask_pack(exp.float() > 0, cpu_)
        c2, sc = sliced_in(c2h, sl), sliced_in(z, sl)
        zero, one, sh = dev(torch.zeros(C), torch.ones(C), shift)
        for form in ("plain", "masked", "fin"):
            out = Guard((N, H, W, C), dt, sl)
            mask = torch.full((N * H * W * (C // cpu_) + 64,), 0xAA, dtype=torch.uint8, device=DEV) if form != "plain" else None
            if form == "fin":
                bn = torch.nn.BatchNorm2d(C, eps=1.0).to(DEV)      # zero statistics: mean 0, var 0, invstd = 1/sqrt(eps) = 1, scale = gamma = 1
                with torch.no_grad():
                    bn.bias.copy_(sh)
                vec = [torch.empty(C, device=DEV) for _ in range(4)]
                fin = ops.bn_fwd_fin(statbuf(2 * C), bn, *vec)
                ops.block_tail_fwd_fin(c2, fin, sc, None, float(N * H * W), out.t, mask)
            else:
                ops.block_tail_fwd(c2, zero, one, sh, sc, None, None, None, out.t, mask)
            torch.cuda.synchronize()
            out.check("block_tail_fwd " + form)
            kref.assert_bits(out.t.cpu(), exp, zero_sign=False, what="block_tail_fwd %s out" % form)
            if mask is not None:
                n = expm.numel()
                kref.assert_bits(mask[:n].cpu(), expm, what="block_tail_fwd %s mask = [stored out > 0]" % form)
                assert bool((mask[n:] == 0xAA).all()), "mask written past its end"
    assert had_lost or dt == torch.float32, "no value that is positive in fp32 and stored as 0"
    row("block_tail_fwd / _masked / _fin" + " C%d %s" % (C, "sliced" if sl else "dense"), "tail_fwd_kernel<%s, false, *>" % TNAME[dt], dt, "finite + inf shifts, T edges in c2; stored 0 <- fp32 > 0", "bit-equal, mask = [stored > 0]")


@pytest.mark.parametrize("C,dt,sl", STREAM, ids=STREAM_IDS)
def test_bn_backward_apply_forms_store_edge_values(C, dt, sl):
    """g = 0, k1 = -value, k2 = 0, scale = 1, open gate: g_c = scale * (g_y - k1 - xhat * k2) = value, rounded once -- ubr_bn_bwd_apply and
    _apply_fin (k1 = sum / count from the stripes); ubr_bn_bwd_frozen with g = 1 and scale = value (finite).  Then the data operand:
    g = T edges, k = 0.  Then a gate whose bn(c) is a positive fp32 subnormal: open, g_y = g."""
    N, H, W = SHAPE
    npix = N * H * W
    z = torch.zeros((N, H, W, C), dtype=dt)
    zc, oc = torch.zeros(C), torch.ones(C)
    c = sliced_in(z, sl)

    def launch(form, g, scale, shift, k1, relu=True):
        out = Guard((N, H, W, C), dt, sl)
        ga = sliced_in(g, sl)
        sc, sh, mean, inv, k1d, k2d = dev(scale, shift, zc, oc, k1, zc)
        if form == "apply":
            ops.bn_bwd_apply(ga, None, c, sc, sh, mean, inv, relu, k1d, k2d, out.t)
        elif form == "apply_fin":
            red = statbuf(2 * C)
            red[:C] = k1.double().to(DEV)
            dgam, dbet = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
            ops.bn_bwd_apply_fin(ga, None, c, sc, sh, mean, inv, relu, red, 1.0, dgam, dbet, out.t)
        else:
            ops.bn_bwd_frozen(ga, None, c, sc, sh, mean, inv, relu, None, out.t)
        torch.cuda.synchronize()
        out.check("bn_bwd " + form)
        return out.t.cpu()

    for v in chunks(kref.edge_values(dt), C):
        exp = (torch.zeros((N, H, W, C)) + v).to(dt)
        for form in ("apply", "apply_fin"):
            kref.assert_bits(launch(form, z, oc, oc, -v), exp, zero_sign=False, what="bn_bwd_%s k1 = -edge" % form)
    for v in chunks(kref.edge_values(dt, exclude=NONFINITE), C):
        exp = (torch.zeros((N, H, W, C)) + v).to(dt)
        kref.assert_bits(launch("frozen", torch.ones_like(z), v, oc, zc), exp, zero_sign=False, what="bn_bwd_frozen scale = edge")
    g = cycle(t_edges(dt), (N, H, W, C))
    for form in ("apply", "apply_fin", "frozen"):
        kref.assert_bits(launch(form, g, oc, oc, zc), g, zero_sign=False, what="bn_bwd_%s g = T edges" % form)
        # the gate: bn(c) = 0 * 1 + 2^-140 > 0
        tiny = torch.full((C,), 2.0 ** -140)
        kref.assert_bits(launch(form, g, oc, tiny, zc), g, zero_sign=False, what="bn_bwd_%s gate at a positive fp32 subnormal" % form)
        kref.assert_bits(launch(form, g, oc, -tiny, zc), torch.zeros_like(g), zero_sign=False, what="bn_bwd_%s gate at a negative fp32 subnormal" % form)
    row("bn_bwd_apply / _apply_fin / _frozen" + " C%d %s" % (C, "sliced" if sl else "dense"), "bn_bwd_kernel / bn_bwd_frozen_kernel <%s>" % TNAME[dt], dt, "all (k1), finite (frozen scale), T edges (g), subnormal gate", "bit-equal")
    assert npix == 256


@pytest.mark.parametrize("C,dt,sl", STREAM, ids=STREAM_IDS)
def test_block_tail_backward_forms_store_edge_values(C, dt, sl):
    """the three tail backward forms on an identity block: go = 0, out > 0, k1_2 = -value -> g_c2 = value and g_sc = g_z = 0; frozen: go = 1,
    scale2 = value -> g_c2 = value, g_sc = 1; then go = T edges with an open and a subnormal gate: g_c2 = g_sc = go"""
    N, H, W = SHAPE
    cpu_ = kref.CPU[dt]
    z = torch.zeros((N, H, W, C), dtype=dt)
    ones = torch.ones_like(z)
    zc, oc = torch.zeros(C), torch.ones(C)
    c2, outp = sliced_in(z, sl), sliced_in(ones, sl)
    allbits = torch.full((N * H * W * (C // cpu_),), 0xFF, dtype=torch.uint8, device=DEV)

    def launch(form, go, scale, shift, k1):
        g1, g2 = Guard((N, H, W, C), dt, sl, "gc2"), Guard((N, H, W, C), dt, sl, "gsc")
        god = sliced_in(go, sl)
        sc, sh, mean, inv, k1d, k2d = dev(scale, shift, zc, oc, k1, zc)
        if form in ("apply", "apply_masked"):
            ops.block_tail_bwd_apply(god, None, outp, c2, sc, sh, mean, inv, k1d, k2d, None, None, None, None, None, None, g1.t, g2.t,
                                     relu_mask=allbits if form == "apply_masked" else None)
        elif form == "apply_fin":
            red = statbuf(2 * C)
            red[:C] = k1.double().to(DEV)
            dgam, dbet = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
            ops.block_tail_bwd_apply_fin(god, None, allbits, c2, sc, sh, mean, inv, red, dgam, dbet, None, None, None, None, None, None, None, 1.0, g1.t, g2.t)
        else:
            ops.block_tail_bwd_frozen(god, None, allbits, c2, sc, sh, mean, inv, statbuf(2 * C), None, None, None, None, None, g1.t, g2.t)
        torch.cuda.synchronize()
        g1.check("block_tail_bwd " + form)
        g2.check("block_tail_bwd " + form)
        return g1.t.cpu(), g2.t.cpu()

    for v in chunks(kref.edge_values(dt), C):
        exp = (torch.zeros((N, H, W, C)) + v).to(dt)
        for form in ("apply", "apply_masked", "apply_fin"):
            gc2, gsc = launch(form, z, oc, oc, -v)
            kref.assert_bits(gc2, exp, zero_sign=False, what="block_tail_bwd_%s k1 = -edge" % form)
            kref.assert_bits(gsc, z, zero_sign=False, what="block_tail_bwd_%s g_sc" % form)
    for v in chunks(kref.edge_values(dt, exclude=NONFINITE), C):
        gc2, gsc = launch("frozen", ones, v, oc, zc)
        kref.assert_bits(gc2, (torch.zeros((N, H, W, C)) + v).to(dt), zero_sign=False, what="block_tail_bwd_frozen scale2 = edge")
        kref.assert_bits(gsc, ones, what="block_tail_bwd_frozen g_sc")
    g = cycle(t_edges(dt), (N, H, W, C))
    tiny = torch.full((C,), 2.0 ** -140)
    for form in ("apply", "apply_masked", "apply_fin", "frozen"):
        for sh, e2 in ((oc, g), (tiny, g), (-tiny, torch.zeros_like(g))):
            gc2, gsc = launch(form, g, oc, sh, zc)
            kref.assert_bits(gc2, e2, zero_sign=False, what="block_tail_bwd_%s go = T edges, shift %r" % (form, float(sh[0])))
            kref.assert_bits(gsc, g, zero_sign=False, what="block_tail_bwd_%s g_sc = go" % form)
    row("block_tail_bwd_apply / _masked / _fin / _frozen" + " C%d %s" % (C, "sliced" if sl else "dense"), "tail_bwd_kernel / tail_bwd_frozen_kernel <%s>" % TNAME[dt], dt, "all (k1), finite (scale2), T edges (go), subnormal gate", "bit-equal")


def pool_input(dt, C, nan=False):
    """2 x 8 x 16 x C of T edges (no NaN, zeros positive: max(+0, -0) has no defined winner) with an all -inf region, a +inf pixel and
    a block of equal subnormals (a first-maximum tie)"""
    N, H, W = SHAPE
    x = cycle(t_edges(dt, exclude=kref.NAN_CLASSES), (N, H, W, C), step=5)
    x = torch.where(x == 0, torch.zeros((), dtype=dt), x)
    x[0, 0:5, 0:5, :] = float("-inf")
    x[0, 6, 3, :] = float("inf")
    x[1, 3:8, 8:16, :] = kref.edge_values(dt, classes=("t_subnormal_min" if dt != torch.float32 else "f32_subnormal_min",))[0].to(dt)
    x[1, 0:3, 8:16, :] = float("-inf")
    x[1, :, 6:8, :] = float("-inf")
    if nan:
        x[0, 7, 10, :] = float("nan")       # the FIRST tap in scan order of one window, a later tap of others
        x[1, 5, 2, :] = float("nan")
    return x


@pytest.mark.parametrize("C,dt,sl", STREAM, ids=STREAM_IDS)
def test_maxpool_selects_and_copies_bits(C, dt, sl):
    """ubr_maxpool_fwd (pooled, xcopy, argmax) and ubr_maxpool_bwd are select / copy: equal bits, sign of zero included; windows that
    are all -inf, hold +inf, or tie among equal subnormals (first maximum wins)"""
    N, H, W = SHAPE
    xh = pool_input(dt, C)
    x = sliced_in(xh, sl)
    for stride in (2, 1):
        ref, am, _ = kref.maxpool_ref(xh, None, stride)
        OH, OW = ref.shape[1], ref.shape[2]
        assert bool((ref == float("-inf")).any()) and bool((ref == float("inf")).any())
        for with_am in (True, False):
            pooled = Guard((N, OH, OW, C), dt, sl, "pooled")
            xc = Guard((N, H, W, C), dt, sl, "xcopy") if stride == 2 else None
            amax = torch.full((N, OH, OW, C), 77, dtype=torch.uint8, device=DEV) if with_am else None
            ops.maxpool_fwd(x, None, pooled.t, xc.t if xc else None, stride, argmax=amax)
            torch.cuda.synchronize()
            what = "maxpool_fwd stride %d%s" % (stride, ", argmax" if with_am else "")
            pooled.check(what)
            kref.assert_bits(pooled.t.cpu(), ref.float().to(dt), what=what + " pooled")
            if xc:
                xc.check(what)
                kref.assert_bits(xc.t.cpu(), xh, what=what + " xcopy")
            if with_am:
                # (kref.maxpool_ref leaves the arg-max of an all -inf window open; the kernel, like ATen, names its first tap inside the image)
                live = ref > float("-inf")
                a = amax.cpu()
                kref.assert_bits(torch.where(live, a, torch.zeros((), dtype=torch.uint8)), torch.where(live, am, torch.zeros((), dtype=am.dtype)).to(torch.uint8), what=what + " argmax")
                first = 4 - 3 * (torch.arange(OH).view(1, -1, 1, 1) > 0).long() - (torch.arange(OW).view(1, 1, -1, 1) > 0).long()
                assert bool((a[~live].long() == first.expand_as(a)[~live]).all()), what + ": arg-max of an all -inf window is not its first tap"
    # backward: every window's maximum is its centre (1 at even pixels, 0 elsewhere), so each input pixel receives at most one gradient
    xb = torch.zeros((N, H, W, C), dtype=dt)
    xb[:, 0::2, 0::2, :] = 1.0
    _, am, _ = kref.maxpool_ref(xb, None, 2)
    gp = cycle(t_edges(dt), (N, H // 2, W // 2, C), step=3)
    ref = kref.maxpool_bwd_ref(gp, am, (H, W), 2).float().to(dt)
    xbd, gpd = sliced_in(xb, sl), sliced_in(gp, sl)
    amd = torch.empty((N, H // 2, W // 2, C), dtype=torch.uint8, device=DEV)
    ops.maxpool_fwd(xbd, None, torch.empty((N, H // 2, W // 2, C), dtype=dt, device=DEV), None, 2, argmax=amd)
    for a in (None, amd):
        gx = Guard((N, H, W, C), dt, sl, "gx")
        ops.maxpool_bwd(xbd, None, gpd, None, gx.t, 2, argmax=a)
        torch.cuda.synchronize()
        gx.check("maxpool_bwd")
        kref.assert_bits(gx.t.cpu(), ref, zero_sign=False, what="maxpool_bwd%s" % (" from argmax" if a is not None else ""))
    row("maxpool_fwd (pooled, xcopy, argmax) / maxpool_bwd" + " C%d %s" % (C, "sliced" if sl else "dense"), "maxpool_fwd_kernel / maxpool_bwd*_kernel <%s>" % TNAME[dt], dt, "T edges, all -inf window, +inf, subnormal tie", "bit-equal")


@pytest.mark.parametrize("dt", DTS, ids=[TNAME[d] for d in DTS])
def test_stem_expand_copies_and_rounds_once(dt):
    N, Cin, H, W = 2, 2, 8, 16
    x = cycle(kref.edge_values(dt), (N, Cin, H, W), step=7)
    out = Guard((N, H, W, 16 * Cin), dt, True)
    ops.stem_expand(x.to(DEV), out.t)
    torch.cuda.synchronize()
    out.check("stem_expand")
    kref.assert_bits(out.t.cpu(), kref.stem_expand_ref(x).float().to(dt), what="stem_expand")
    row("stem_expand", "stem_expand_kernel<%s>" % TNAME[dt], dt, "all", "bit-equal")


# ----------------------------------------------------------------------------------------------------------------------
# NaN at ReLU / max / gates: characterised; the variants of one operation must agree, nothing else may change
# ----------------------------------------------------------------------------------------------------------------------
def classify(t):
    """what a NaN turned into: 'NaN', '0', or the values seen"""
    f = t.float().reshape(-1)
    if bool(torch.isnan(f).all()):
        return "NaN"
    if bool((f == 0).all()):
        return "0"
    return "mixed:" + ",".join("%g" % v for v in f.unique()[:4].tolist())


def test_nan_at_conv_relu_is_the_same_in_every_kernel_variant():
    """bias = NaN (x = 0): act = 0 stores NaN; act = 1, 2, 3 go through max(v, 0), which returns the operand that is a number.
    (a) igemm, PIPE, thin, ROW7 and pc kernels and all dtypes agree; (b) the sentinels around the output hold."""
    seen = {}
    for path, dt in CONV_PARAMS:
        cp = ConvPath(path, dt)
        b = torch.full((cp.Cout,), float("nan"))
        b[1::2] = 1.5                                   # NaN in every other channel only: the neighbours must not change
        for act in (0, 1, 2, 3):
            got = cp.run(b, act=act)                    # (run() checks the sentinels)
            assert bool((got[..., 1::2].float() == 1.5).all()), "%s act %d: a NaN channel changed its neighbour" % (cp.name, act)
            seen.setdefault(act, {})[(path, TNAME[dt])] = classify(got[..., 0::2])
        row("NaN bias at conv ReLU " + path, cp.name, dt, "NaN", "act0 %s | act1 %s | act2 %s | act3 %s" % tuple(seen[a][(path, TNAME[dt])] for a in (0, 1, 2, 3)))
    for act, d in seen.items():
        assert len(set(d.values())) == 1, "act %d: kernel variants disagree on NaN: %r" % (act, d)
    assert set(seen[0].values()) == {"NaN"}


def test_nan_at_block_tail_and_gates_is_the_same_in_every_variant():
    """NaN through ubr_vmax (block tail forward; plain, masked, fused finalize) and through the [bn(c) > 0] gates of the backward forms"""
    N, H, W = SHAPE
    res = {}
    for dt in DTS:
        for C in (16, 96):
            cpu_ = kref.CPU[dt]
            z = torch.zeros((N, H, W, C), dtype=dt, device=DEV)
            shift = torch.full((C,), float("nan"))
            shift[1::2] = 0.25
            zero, one, sh = dev(torch.zeros(C), torch.ones(C), shift)
            for form in ("plain", "masked", "fin"):
                out = Guard((N, H, W, C), dt, True)
                mask = torch.zeros((N * H * W * (C // cpu_),), dtype=torch.uint8, device=DEV) if form != "plain" else None
                if form == "fin":
                    bn = torch.nn.BatchNorm2d(C, eps=1.0).to(DEV)
                    with torch.no_grad():
                        bn.bias.copy_(sh)
                    fin = ops.bn_fwd_fin(statbuf(2 * C), bn, *[torch.empty(C, device=DEV) for _ in range(4)])
                    ops.block_tail_fwd_fin(z, fin, z, None, float(N * H * W), out.t, mask)
                else:
                    ops.block_tail_fwd(z, zero, one, sh, z, None, None, None, out.t, mask)
                torch.cuda.synchronize()
                out.check("tail " + form)
                o = out.t.cpu()
                assert bool((o[..., 1::2].float() == 0.25).all())
                r = classify(o[..., 0::2])
                if mask is not None:
                    kref.assert_bits(mask.cpu(), kref.mask_pack(o.float() > 0, cpu_), what="mask = [stored out > 0] with NaN shifts")
                res.setdefault("tail_fwd", {})[(form, TNAME[dt], C)] = r
            # gates: c = NaN in the even channels -> bn(c) = NaN, [NaN > 0] is false: g_y = 0; k = 0, scale = 1
            c = torch.zeros((N, H, W, C), dtype=dt)
            c[..., 0::2] = float("nan")
            c = c.to(DEV)
            g = torch.ones((N, H, W, C), dtype=dt, device=DEV)
            allbits = torch.full((N * H * W * (C // cpu_),), 0xFF, dtype=torch.uint8, device=DEV)
            for form in ("bn_apply", "bn_frozen", "tail_apply", "tail_apply_masked", "tail_frozen"):
                o1, o2 = Guard((N, H, W, C), dt, True, "a"), Guard((N, H, W, C), dt, True, "b")
                if form == "bn_apply":
                    ops.bn_bwd_apply(g, None, c, one, one, zero, one, True, zero, zero, o1.t)
                elif form == "bn_frozen":
                    ops.bn_bwd_frozen(g, None, c, one, one, zero, one, True, None, o1.t)
                elif form == "tail_frozen":
                    ops.block_tail_bwd_frozen(g, None, allbits, c, one, one, zero, one, statbuf(2 * C), None, None, None, None, None, o1.t, o2.t)
                else:
                    ops.block_tail_bwd_apply(g, None, g, c, one, one, zero, one, zero, zero, None, None, None, None, None, None, o1.t, o2.t,
                                             relu_mask=allbits if form == "tail_apply_masked" else None)
                torch.cuda.synchronize()
                o1.check(form)
                o2.check(form)
                o = o1.t.cpu()
                assert bool((o[..., 1::2].float() == 1.0).all()), form
                res.setdefault("gate " + form.split("_")[0] + ("_frozen" if "frozen" in form else "_apply"), {})[(form, TNAME[dt], C)] = classify(o[..., 0::2])
    for op, d in res.items():
        for dt in DTS:
            vals = sorted({v for k, v in d.items() if k[1] == TNAME[dt]})
            row("NaN at " + op, ", ".join(sorted({k[0] for k in d})), dt, "NaN shift / NaN c", " ".join(vals))
        assert len(set(d.values())) == 1, "%s: variants disagree on NaN: %r" % (op, d)


def test_nan_at_maxpool_is_the_same_with_and_without_argmax():
    """a NaN pixel as the first tap of a window and as a later tap: the forward with the saved arg-max (strict > scan) and without it
    (fmaxf chain) must store the same pooled bits; windows without the NaN pixel are the reference's"""
    N, H, W = SHAPE
    for dt in DTS:
        for C in (16, 96):
            xh = pool_input(dt, C, nan=True)
            x = xh.to(DEV)
            clean = pool_input(dt, C)
            for stride in (2, 1):
                ref, _, _ = kref.maxpool_ref(clean, None, stride)
                touched, _, _ = kref.maxpool_ref(torch.isnan(xh.float()).double(), None, stride)
                outs = []
                for with_am in (True, False):
                    OH, OW = ref.shape[1], ref.shape[2]
                    pooled = Guard((N, OH, OW, C), dt, True)
                    amax = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=DEV) if with_am else None
                    ops.maxpool_fwd(x, None, pooled.t, None, stride, argmax=amax)
                    torch.cuda.synchronize()
                    pooled.check("maxpool NaN")
                    o = pooled.t.cpu()
                    exp = ref.float().to(dt)
                    keep = touched == 0
                    kref.assert_bits(torch.where(keep, o, torch.zeros((), dtype=dt)), torch.where(keep, exp, torch.zeros((), dtype=dt)), what="windows without a NaN")
                    outs.append(o)
                # what the windows holding a NaN became: the maximum of their other taps (NaN skipped), NaN, or something else
                skip = kref.maxpool_ref(torch.where(torch.isnan(xh.float()), torch.full((), float("-inf"), dtype=dt), xh), None, stride)[0].float().to(dt)
                sel = touched > 0

                def became(o):
                    if bool((kref.bits(o)[sel] == kref.bits(skip)[sel]).all()):
                        return "max of the other taps"
                    return "NaN" if bool(torch.isnan(o.float()[sel]).all()) else "NaN where it is the first tap" if bool(torch.isnan(o.float()[sel]).any()) else "other"
                verdict = "windows with a NaN tap: arg-max form -> %s; plain form -> %s" % (became(outs[0]), became(outs[1]))
                row("NaN at maxpool_fwd stride %d C%d" % (stride, C), "maxpool_fwd_kernel<%s, %d, false, true|false, false>" % (TNAME[dt], stride), dt,
                    "NaN as first tap / as a later tap", verdict)
                kref.assert_bits(outs[0], outs[1], what="maxpool_fwd stride %d %s: with and without argmax on a NaN input" % (stride, TNAME[dt]))
                # the contract, shared with the pool slice of ubr_aspp_front: a NaN tap is skipped
                kref.assert_bits(outs[0], skip, what="maxpool_fwd stride %d %s: a NaN tap is skipped" % (stride, TNAME[dt]))


def test_nan_pixel_in_a_whole_train_step_is_visible():
    """UResNet 1x1x64x64 fp32, train mode, ONE NaN input pixel: the step completes; the corruption must be visible -- a non-finite loss,
    or a non-finite running_mean of the stem's BatchNorm"""
    from oracle import uresnet_oracle as O
    from ubresnet_amd import synthetic
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
    x, lab, wgt = synthetic.make_batch(1, 64, 64, 1000)
    xt, lt, wt = torch.from_numpy(x).clone(), torch.from_numpy(lab), torch.from_numpy(wgt)
    xt[0, 0, 31, 17] = float("nan")
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    out = m(xt.to(DEV))
    loss = PixelWiseNLLLoss()(out, lt.to(DEV), wt.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    bns = [(n, b) for n, b in m.named_modules() if isinstance(b, torch.nn.modules.batchnorm._BatchNorm)]
    bad_mean = [n for n, b in bns if not bool(torch.isfinite(b.running_mean).all())]
    bad_var = [n for n, b in bns if not bool(torch.isfinite(b.running_var).all())]
    bad_grad = [n for n, p in m.named_parameters() if p.grad is not None and not bool(torch.isfinite(p.grad).all())]
    stem = bns[0]
    frac = float(torch.isnan(out).float().mean())
    row("train step, one NaN input pixel", "UResNet 1x1x64x64", torch.float32, "NaN",
        "loss %r | NaN log-probs %.4f | running_mean non-finite at %d of %d sites (stem %s: %s) | running_var %d | non-finite grads %d of %d"
        % (float(loss), frac, len(bad_mean), len(bns), stem[0], "yes" if stem[0] in bad_mean else "no", len(bad_var), len(bad_grad), len(list(m.parameters()))))
    assert not bool(torch.isfinite(loss)) or stem[0] in bad_mean, "a NaN input pixel left a finite loss %r and a finite stem running_mean" % float(loss)


# ----------------------------------------------------------------------------------------------------------------------
# ubr_aspp_front (C = 32), tile crop / stitch, ubr_logsoftmax_bwd
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=[TNAME[d] for d in DTS])
def test_aspp_front_branch_stores_and_pool_slice(dt):
    """edge biases through the four conv branches (x = 0: out = relu(0 + bias), rounded once); T edges through the max-pool slice
    (zero weights: the branches store relu(0) = 0; the slice is a selection, equal bits); then infinities, an all -inf window and a
    NaN pixel in the pool slice, where the slice must agree with ubr_maxpool_fwd's rule: a NaN tap is skipped"""
    N, H, W, Cn = 1, 16, 32, 32
    cpu_ = kref.CPU[dt]
    wr = torch.randn((28, Cn // cpu_, 16, cpu_), generator=torch.Generator().manual_seed(11)).to(dt).to(DEV)
    wz = torch.zeros_like(wr)
    xz = torch.zeros((N, H, W, Cn), dtype=dt, device=DEV)
    for b in chunks(kref.edge_values(dt, exclude=kref.NAN_CLASSES), 64):
        out = Guard((N, H, W, 64 + Cn), dt, True)
        ops.aspp_front(xz, wr, b.to(DEV), out.t)
        torch.cuda.synchronize()
        out.check("aspp_front")
        o = out.t.cpu()
        kref.assert_bits(o[..., :64], relu32(torch.zeros((N, H, W, 64)) + b).to(dt), zero_sign=False, what="aspp_front branch stores")
        kref.assert_bits(o[..., 64:], torch.zeros((N, H, W, Cn), dtype=dt), what="aspp_front pool slice of zeros")
    fin = t_edges(dt, exclude=NONFINITE + ("flt_max", "overflow_tie"))
    fin = fin[torch.isfinite(fin)]
    xfin = cycle(torch.where(fin == 0, torch.zeros((), dtype=dt), fin), (N, H, W, Cn), step=5)
    xinf = xfin.clone()
    xinf[0, 0:5, 0:5, :] = float("-inf")
    xinf[0, 9, 20, :] = float("inf")
    xnan = xinf.clone()
    xnan[0, 12, 7, :] = float("nan")
    zb = torch.zeros(64, device=DEV)
    for xin, tag in ((xfin, "finite"), (xinf, "inf"), (xnan, "NaN")):
        out = Guard((N, H, W, 64 + Cn), dt, True)
        ops.aspp_front(sliced_in(xin, True), wz, zb, out.t)
        torch.cuda.synchronize()
        out.check("aspp_front " + tag)
        o = out.t.cpu()
        clean = torch.where(torch.isnan(xin.float()), torch.full((), float("-inf"), dtype=dt), xin)
        kref.assert_bits(o[..., 64:], kref.maxpool_ref(clean, None, 1)[0].float().to(dt), what="aspp_front pool slice, %s input" % tag)
        if tag == "finite":
            kref.assert_bits(o[..., :64], torch.zeros((N, H, W, 64), dtype=dt), zero_sign=False, what="aspp_front branches under zero weights")
    row("aspp_front C=32: 4 branches + pool slice", "aspp_front_kernel<%s>" % TNAME[dt], dt, "finite + inf biases; T edges, +-inf, all -inf window, NaN tap (skipped)", "bit-equal")


def test_crop_and_stitch_tiles_copy_bits():
    """pure copies of fp32 planes: every edge bit pattern, the sign of zero and the NaN payload class included"""
    import ctypes as C
    import numpy as np
    from ubresnet_amd import _lib as L
    dt = torch.float32
    P, rows, cols, th, tw, Cn = 2, 20, 24, 16, 16, 3
    desc = lambda tiles: (C.c_int32 * (len(tiles) * len(tiles[0])))(*[int(v) for t in tiles for v in t])
    view = cycle(kref.edge_values(dt), (P, rows, cols), step=3).to(DEV)
    ctiles = [(0, 0, 0, 0, 16, 0, 16), (1, 8, 16, 0, 16, 0, 16), (0, 16, 16, 0, 16, 0, 16)]                         # the last two overhang the view: zero fill
    n = len(ctiles) * th * tw
    cbuf = torch.full((n + 128,), 7.0, device=DEV)
    L.check(L.lib().ubr_crop_tiles(view.data_ptr(), P, rows, cols, desc(ctiles), len(ctiles), th, tw, cbuf[64:].data_ptr(), L.stream_ptr()), "crop_tiles")
    torch.cuda.synchronize()
    ref = torch.from_numpy(kref.crop_tiles_ref(view.cpu().numpy(), ctiles, th, tw))
    kref.assert_bits(cbuf[64:64 + n].cpu().view(ref.shape), ref, what="crop_tiles")
    assert bool((cbuf[:64] == 7.0).all()) and bool((cbuf[64 + n:] == 7.0).all())
    scores = cycle(kref.edge_values(dt), (2, Cn, th, tw), step=5).to(DEV)
    stiles = [(0, 0, 0, 0, 16, 0, 12), (1, 4, 8, 2, 16, 0, 16)]
    m = P * Cn * rows * cols
    sbuf = torch.full((m + 128,), 7.0, device=DEV)
    L.check(L.lib().ubr_stitch_tiles(scores.data_ptr(), Cn, th, tw, desc(stiles), len(stiles), sbuf[64:].data_ptr(), P, rows, cols, L.stream_ptr()), "stitch_tiles")
    torch.cuda.synchronize()
    ref = torch.from_numpy(kref.stitch_tiles_ref(scores.cpu().numpy(), stiles, np.full((P, Cn, rows, cols), 7.0, dtype=np.float32)))
    kref.assert_bits(sbuf[64:64 + m].cpu().view(ref.shape), ref, what="stitch_tiles")
    assert bool((sbuf[:64] == 7.0).all()) and bool((sbuf[64 + m:] == 7.0).all())
    row("crop_tiles / stitch_tiles", "crop_tiles_kernel / stitch_tiles_kernel", dt, "all fp32 classes", "bit-equal")


@pytest.mark.parametrize("dt", DTS, ids=[TNAME[d] for d in DTS])
def test_logsoftmax_backward_past_the_expf_underflow(dt):
    """log-probabilities down to log 2^-160 = -110.9 (expf gives a subnormal at -90, then 0): within kref.logsoftmax_bwd_ref's bound"""
    N, Cn, H, W = 2, 4, 8, 16
    pv = torch.tensor([1.0 - 2.0 ** -10, 2.0 ** -10, 2.0 ** -130, 2.0 ** -160], dtype=torch.float64)
    p = pv[(torch.arange(Cn).view(1, Cn, 1, 1) + torch.arange(W).view(1, 1, 1, W)) % Cn].expand(N, Cn, H, W).contiguous()
    g = kref.exact_operands((N, Cn, H, W), torch.float32, density=0.9, seed=31, exp=-3).double()
    out = Guard((N, H, W, 16), dt, True)
    ops.logsoftmax_bwd(g.float().to(DEV), p.log().float().to(DEV), out.t)
    torch.cuda.synchronize()
    out.check("logsoftmax_bwd")
    ref, lim = kref.logsoftmax_bwd_ref(g, p, dt)
    o = out.t.cpu()
    kref.assert_within(o[..., :Cn], ref, lim, "logsoftmax_bwd")
    kref.assert_bits(o[..., Cn:], torch.zeros((N, H, W, 16 - Cn), dtype=dt), what="logsoftmax_bwd padding channels")
    row("logsoftmax_bwd", "logsoftmax_bwd_kernel<%s>" % TNAME[dt], dt, "log p = -90.1 (subnormal expf), -110.9 (expf = 0)", "within kref.logsoftmax_bwd_ref")
