"""Float64 restatements of the two MFMA entry points of include/ubresnet_hip.h -- one ubr_conv launch (ops.conv /
ops.conv_phases) and one weight gradient (ops.wgrad) -- written from the descriptor, not from F.conv2d, of the elementwise
formulas of its streaming kernels (block tail, BatchNorm backward, max-pool, head and loss), plus the checks the kernel tests
compare with and the sentinel-guarded replay buffers they share.  A helper module for the tests (imported by name; not a conftest).

Exact operands.  exact_operands() draws sparse small dyadic values m * 2^e, m in {-2,-1,0,1,2}, with whole all-zero
16x16 tiles as on LArTPC crops.  With per-channel transforms picked from scale in {0.5,1,2}, shift in {-1,0,1} and an
integer `sub`, every operand a kernel feeds its MFMAs is a small dyadic number, exact in bf16, f16 and fp32, every
product is exact, and every partial sum is an integer multiple of one power of two `unit`.  If, for an output, the
sum of the absolute values of its terms (the same op on |operands|, returned alongside every reference as `absref`)
stays below 2^24 * unit, then EVERY fp32 summation order -- any split-K, slab order, MFMA shape or tile walk -- gives
the exact value, and the stored output must equal the fp64 reference after one round-to-nearest-even to the output
type (ET<bf16_t> converts with v_cvt_pk_bf16_f32, RNE; torch's .to() is RNE too).  The check is then bit for bit: a
dropped, doubled or shifted tap, tile, channel slice or pixel is off by whole units.  assert_exact() asserts the
budget before it compares; it never assumes it.

Where the budget cannot hold (outputs with huge fan-in, the fp32 statistics over a whole 512x512 batch, the
log-softmax epilogue) assert_bounded() / assert_stats() check a stated error bound instead (constants below).
"""
import math

import torch

U32 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
UNIT_ROUNDOFF = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
CPU = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}          # channels per 16-byte unit
NEG_BIG = -3.0e38
STAT_SLOTS, RED_SLOTS = 32, 8

# assert_bounded(): |got - ref| <= C_OUT * u_out * |ref| + C_ACC * K * 2^-24 * absref.
#   The kernel's fp32 value v^ of an output with K terms carries |v^ - ref| <= gamma_K * absref (any summation order,
#   gamma_K = K u / (1 - K u) <= 1.01 K u for K u < 0.01); the store rounds once more: |round(v^) - v^| <= u_out |v^|
#   <= u_out (|ref| + gamma_K absref).  With u_out <= 2^-8 the sum is below C_OUT u_out |ref| + C_ACC K u absref.
C_OUT = 1.0
C_ACC = 1.03

# Conv statistics (ubr_conv_desc.stats).  Finding, from the epilogues of conv_igemm_kernel / conv_pc_kernel /
# conv_thin_kernel (csrc/ubr_conv.hip, `finish` and the fast epilogue): the forward statistics sum the fp32 value
# v = act(conv + bias (+ addend)) BEFORE it is rounded to the stored type (s1 += v; s2 += v*v); only the
# BatchNorm-backward form (bnb_c) rounds first (round4<T> -> g, then bnb_accumulate).  The sums are fp32 per lane:
# one lane adds one pixel of every 16-pixel row fragment it owns (a chain, in pixel order, of at most
# N*OH*ceil(OW/16) terms, however the workgroups are laid out -- the persistent conv_pc_kernel flushes only when its
# cout tile changes), then wave_quadrow_sum16 adds the 16 lanes of a row in 4 butterfly levels (csrc/ubr_common.h),
# and from there on everything is fp64 (per-workgroup fp64 adds, fp64 atomics into the slots).  So each fp32 partial
# is a sum of at most L = N*OH*ceil(OW/16) + 4 rounding steps deep, and per channel
#     |s1 - sum v|   <= gamma_L * sum |v|          (+ fp64: 2^-50 * sum |v|)
#     |s2 - sum v^2| <= gamma_{L+1} * sum v^2      (one more rounding: v*v in fp32)
# The same L bounds the BatchNorm-backward sums (same lane chain, sum g_y and sum g_y*xhat; xhat = d*invstd is one
# more rounding, covered by the +1).  stats_eps() returns these epsilons.


# Reduce passes of the streaming kernels (csrc/ubr_elem.hip: bn_bwd_kernel / tail_bwd_kernel with APPLY = false, channel_sum_kernel).
# Finding: a thread keeps ONE 16-byte channel unit and adds its pixels' terms (g_y, and g_y*xhat = g_y * fl((c - mean)*invstd)) into
# fp32 registers, a chain of ceil(npix * CU / (256 * workgroups)) terms -- 8 to 64 at the network's shapes, since pick_blocks() gives
# a thread 8 pixels and caps the grid at 512 workgroups (channel_sum: one pixel per thread, capped at 1024).  With a power-of-two
# unit count below 64 (every U-ResNet layer), flush_sums_pow2 then adds the 64/CU lanes of a wave that hold the same unit in
# log2(64/CU) fp32 butterfly levels; from the per-wave LDS rows on everything is fp64 (four rows added per workgroup, one fp64 atomic
# per channel into stripe blockIdx % UBR_RED_SLOTS).  With CU >= 64 there is no butterfly, and for other unit counts (C = 80, 96) and
# in channel_sum the per-thread fp32 partial goes straight into fp64 LDS atomics.  So an fp32 partial is at most
# L = ceil(npix*CU/(256*workgroups)) + log2(64/CU) roundings deep; a bounded check would use gamma(L + 1) * sum |terms| per channel (the
# +1: xhat is rounded once).  On exact operands no bound is needed: assert_sums_exact() asserts that the sum of |terms| of a whole
# channel stays below 2^24 units of the term grid, so every fp32 partial of any grid is exact, and compares for equality.


# Log-softmax epilogue (ubr_conv_desc.epilogue = 1; the head's 7x7 conv, thin or generic kernel): over the n = Cout <= 16 exact fp32 logits v of a
# pixel the kernel forms m = max v (exact), e = sum_r expf(v_r - m), lse = m + logf(e), out = v - lse, all in fp32.  With
# expf / logf within 2 ulp (<= 4u relative; u = 2^-24):
#   d_r = fl(v_r - m) = (v_r - m)(1 + d), |d| <= u: exp(d_r) = exp(v_r - m)(1 + u|v_r - m|); as x e^-x <= 1/e, these add
#     at most (n/e) u e to e;  expf: 4u per term;  the sum of n terms in [0, 1]: (n - 1) u e.   So e^ = e (1 + t),
#     |t| <= (1.4 n + 4) u  (first order; e >= 1 since the max term is 1).
#   logf(e^) = log e + log(1 + t) + 4u |log e|, log e <= ln n:  |error| <= (1.4 n + 4 + 4 ln n) u.
#   lse = fl(m + logf(e^)): + u |lse|;  out = fl(v - lse): + u |out|.
# Hence |got - ref| <= u (|ref| + |lse| + 1.4 n + 4 + 4 ln n), times C_ACC for the second-order terms: logsoftmax_ref().


def logsoftmax_ref(v):
    """v: fp64 exact logits, channels last -> (log-softmax fp64, per-element bound of the fused epilogue; see above)"""
    n = v.shape[-1]
    m = v.amax(-1, keepdim=True)
    lse = m + torch.log(torch.exp(v - m).sum(-1, keepdim=True))
    ref = v - lse
    return ref, C_ACC * U32 * (ref.abs() + lse.abs() + 1.4 * n + 4 + 4 * math.log(n))


# The same epilogue on logits that are not exact (tests/stage_shadow.py: the head's conv11 on realistic operands).  The kernel's fp32
# logits v^ differ from the fp64 logits v of the recorded inputs by |v^_c - v_c| <= pre_c (accumulation + on-load affine, the term
# ref_conv forms for every conv).  Log-softmax is out_c = v_c - lse(v); lse is a maximum-like function: its gradient is the softmax
# p (p_r >= 0, sum p_r = 1), so |lse(v^) - lse(v)| <= max_r |v^_r - v_r| and
#     |out_c(v^) - out_c(v)| <= |v^_c - v_c| + max_r |v^_r - v_r| <= 2 max_r pre_r.
# The epilogue's own error, logsoftmax_ref()'s bound, applies to the logits the kernel has; evaluated on v instead of v^ its
# |ref| + |lse| term moves by at most 3 max pre * u, second order, covered by C_ACC.  The output is stored as fp32: that rounding is
# the u |out| of the bound above.  Hence logsoftmax_bound(): the epilogue bound + 2 max_r pre_r per pixel.
def logsoftmax_bound(v, pre):
    """v: fp64 logits, pre: bound of the fp32 logits' error, both channels last -> (log-softmax fp64, bound of the fused epilogue's output)"""
    ref, lim = logsoftmax_ref(v)
    return ref, lim + 2.0 * pre.amax(-1, keepdim=True)


def stats_chain(N, OH, OW):
    return N * OH * ((OW + 15) // 16) + 4


def gamma(k):
    ku = k * U32
    return ku / (1.0 - ku) if ku < 0.5 else float("inf")


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
def exact_operands(shape, dtype, density=0.25, seed=0, exp=0, zero_tiles=0.5, tile=16, device="cpu", maxmag=2):
    """values m * 2^exp, m uniform in {-maxmag..-1, 1..maxmag} where nonzero; `density` of the entries nonzero; for a 4-D NHWC
    shape, a fraction `zero_tiles` of the tile x tile pixel blocks is all zero (every channel)."""
    g = torch.Generator(device=device).manual_seed(seed)
    m = torch.randint(1, maxmag + 1, shape, generator=g, device=device, dtype=torch.int32)
    sgn = torch.randint(0, 2, shape, generator=g, device=device, dtype=torch.int32) * 2 - 1
    keep = torch.rand(shape, generator=g, device=device) < density
    v = torch.where(keep, (m * sgn).float(), torch.zeros((), device=device))
    if len(shape) == 4 and zero_tiles > 0:
        N, H, W, _ = shape
        th, tw = (H + tile - 1) // tile, (W + tile - 1) // tile
        z = torch.rand((N, th, tw), generator=g, device=device) < zero_tiles
        z = z.repeat_interleave(tile, 1).repeat_interleave(tile, 2)[:, :H, :W]
        v = v.masked_fill(z.unsqueeze(-1), 0.0)
    return (v * 2.0 ** exp).to(dtype)


def exact_affine(C, seed, device="cpu", relu=True, sub_exp=0):
    """(sub, scale, shift, lo) fp32 vectors for which max((v - sub)*scale + shift, lo) is exact on exact operands:
    sub in {-1,0,1}*2^sub_exp, scale in {0.5,1,2}, shift in {-1,0,1}; lo = 0 (ReLU) or NEG_BIG (none), or a vector"""
    g = torch.Generator().manual_seed(seed)
    sub = (torch.randint(-1, 2, (C,), generator=g).float() * 2.0 ** sub_exp)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    shift = torch.randint(-1, 2, (C,), generator=g).float()
    if isinstance(relu, torch.Tensor):
        lo = relu.float().cpu()
    else:
        lo = torch.full((C,), 0.0 if relu else NEG_BIG)
    return tuple(t.to(device) for t in (sub, scale, shift, lo))


# ------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------
def unpack_weights(wp, Cin, Cout):
    """packed image [ntaps][Kpad/CPU][Mpad][CPU] (ubr_pack_weights) -> fp64 [ntaps][Cin][Cout]"""
    T, KU, Mp, cpu = wp.shape
    return wp.double().permute(0, 1, 3, 2).reshape(T, KU * cpu, Mp)[:, :Cin, :Cout]


def pack_dense(W, taps_idx, fwd=True):
    """PyTorch weight [Cout][Cin][kh][kw] (fwd) or [Cin][Cout][kh][kw] (dgrad / ConvTranspose2d orientation, fwd=False)
    -> dense fp64 [ntaps][K][M] with K the summed channel, tap image index i = tap index i of the window"""
    Wd = W.double()
    if fwd:
        Wd = Wd.permute(1, 0, 2, 3)          # [Cin][Cout][kh][kw]
    K, M = Wd.shape[0], Wd.shape[1]
    flat = Wd.reshape(K, M, -1)
    return flat[:, :, list(taps_idx)].permute(2, 0, 1).contiguous()


def _xform(x, xf):
    v = x.double()
    if xf is not None:
        sub, scale, shift, lo = (t.double().to(v.device) for t in xf)
        C = v.shape[-1]
        v = torch.maximum((v - sub[:C]) * scale[:C] + shift[:C], lo[:C])
    return v


def _gather(xt, taps, S, iy0, ix0, OH, OW):
    """yield (tap number, view [N,OH,OW,C] of the zero-padded input at oy*S+iy0+dy, ox*S+ix0+dx)"""
    N, H, W, C = xt.shape
    dys = [t[0] for t in taps]
    dxs = [t[1] for t in taps]
    pt = max(0, -(iy0 + min(dys)))
    pb = max(0, (OH - 1) * S + iy0 + max(dys) - (H - 1))
    pl = max(0, -(ix0 + min(dxs)))
    pr = max(0, (OW - 1) * S + ix0 + max(dxs) - (W - 1))
    xp = torch.nn.functional.pad(xt, (0, 0, pl, pr, pt, pb))
    for i, (dy, dx) in enumerate(zip(dys, dxs)):
        y0, x0 = iy0 + dy + pt, ix0 + dx + pl
        yield i, xp[:, y0:y0 + (OH - 1) * S + 1:S, x0:x0 + (OW - 1) * S + 1:S, :]


# ------------------------------------------------------------------------------------------------------------------
# ubr_conv
# ------------------------------------------------------------------------------------------------------------------
def conv_ref(x, W, taps, Cout, OH, OW, S=1, iy0=0, ix0=0, xf=None, bias=None, addend=None, addend_mask=None, act=0,
             want_abs=True):
    """fp64 value of what ONE ubr_conv launch computes, and the same op on |operands| (the budget):
        out(oy,ox,co) = act( bias[co] + addend*bit + sum_t sum_ci xform(x)(oy*S+iy0+dy[t], ox*S+ix0+dx[t], ci) * W[wt[t]][ci][co] )
    x: NHWC [N,H,W,Cin]; W: fp64 [ntaps_img][Cin][Cout] (unpack_weights of the packed image); taps [(dy,dx,wt)];
    xf: (sub, scale, shift, lo) or None (zero padding AFTER the transform); addend: NHWC [N,OH,OW,Cout];
    addend_mask: uint8 [N*OH*OW*Cout/CPU] bits (channel e of unit u = bit e of byte u); act: bit 0 ReLU before the addend,
    bit 1 ReLU after it.  Returns (ref, absref), fp64 [N,OH,OW,Cout]."""
    xt = _xform(x, xf)
    N = xt.shape[0]
    Cin = xt.shape[3]
    Wd = W.double().to(xt.device)
    acc = torch.zeros((N, OH, OW, Cout), dtype=torch.float64, device=xt.device)
    accabs = torch.zeros_like(acc) if want_abs else None
    for i, v in _gather(xt, taps, S, iy0, ix0, OH, OW):
        wt = Wd[taps[i][2], :Cin, :Cout]
        acc += torch.matmul(v, wt)
        if want_abs:
            accabs += torch.matmul(v.abs(), wt.abs())
    if bias is not None:
        b = bias.double().to(acc.device)[:Cout]
        acc += b
        if want_abs:
            accabs += b.abs()
    if act & 1:
        acc = acc.clamp_min(0)
    if addend is not None:
        a = addend.double().to(acc.device)
        if addend_mask is not None:
            a = a * mask_bits(addend_mask, a.shape, CPU[addend.dtype]).to(acc.device)
        acc = acc + a
        if want_abs:
            accabs = accabs + a.abs()
    if act & 2:
        acc = acc.clamp_min(0)
    return acc, accabs


def mask_bits(mask, shape, cpu):
    N, OH, OW, C = shape
    m = mask[:N * OH * OW * (C // cpu)].view(N, OH, OW, C // cpu, 1).to(torch.int32)
    bits = (m >> torch.arange(cpu, device=mask.device, dtype=torch.int32)) & 1
    return bits.reshape(N, OH, OW, C).double()


def conv_phases_ref(x, W, phases, Cout, OH, OW, xf=None, bias=None, addend_full=None):
    """fp64 value of a phased launch (ops.conv_phases): phase (ry, rx, taps) writes y_full[:, ry::2, rx::2] (OH x OW each);
    addend_full (optional) has y_full's shape.  Returns (ref, absref) of y_full's shape; positions no phase writes are NaN."""
    N = x.shape[0]
    ref = torch.full((N, 2 * OH, 2 * OW, Cout), float("nan"), dtype=torch.float64, device=x.device)
    ab = ref.clone()
    for ry, rx, tp in phases:
        ad = addend_full[:, ry::2, rx::2, :] if addend_full is not None else None
        r, a = conv_ref(x, W, tp, Cout, OH, OW, xf=xf, bias=bias, addend=ad)
        ref[:, ry::2, rx::2, :] = r
        ab[:, ry::2, rx::2, :] = a
    return ref, ab


def round_to(ref, dtype):
    """one RNE rounding of an fp64 value that is exact in fp32 (the budget) to the stored type"""
    return ref.float().to(dtype)


def conv_stats_ref(v, bnb=None, dtype=None):
    """per-channel reference sums of ubr_conv_desc.stats over the output grid: (s1, s2, a1, a2) fp64 [C] with a = sum of |terms|.
    Forward statistics: s1 = sum v, s2 = sum v^2 of the fp32 value BEFORE it is stored (see the note at the top).
    bnb = (c, mean, scale, shift, invstd): BatchNorm-backward sums of the STORED output g = round(v):
    s1 = sum g*[bn(c) > 0], s2 = sum g*[bn(c) > 0] * (c - mean)*invstd, bn(c) = (c - mean)*scale + shift."""
    C = v.shape[-1]
    if bnb is None:
        f = v.reshape(-1, C)
        return f.sum(0), (f * f).sum(0), f.abs().sum(0), (f * f).sum(0)
    c, mean, scale, shift, invstd = bnb
    g = round_to(v, dtype).double().reshape(-1, C)
    cd = c.double().reshape(-1, C).to(g.device)
    d = cd - mean.double().to(g.device)
    bn = d * scale.double().to(g.device) + shift.double().to(g.device)
    gy = torch.where(bn > 0, g, torch.zeros((), dtype=g.dtype, device=g.device))
    t2 = gy * (d * invstd.double().to(g.device))
    return gy.sum(0), t2.sum(0), gy.abs().sum(0), t2.abs().sum(0)


# ------------------------------------------------------------------------------------------------------------------
# ubr_wgrad (+ ubr_wgrad_reduce)
# ------------------------------------------------------------------------------------------------------------------
def wgrad_ref(x, g, taps, S=1, iy0=0, ix0=0, xf=None, want_abs=True):
    """dW[t][co][ci] = sum_{n,oy,ox} g(n,oy,ox,co) * xform(x)(n, oy*S+iy0+dy[t], ox*S+ix0+dx[t], ci), fp64 [ntaps][Cout][Cin],
    and the same op on |operands|.  taps: [(dy, dx, anything)]."""
    xt = _xform(x, xf)
    gd = g.double().to(xt.device)
    N, GH, GW, Cout = gd.shape
    Cin = xt.shape[3]
    g2 = gd.reshape(-1, Cout).t()
    ga = g2.abs() if want_abs else None
    out = torch.empty((len(taps), Cout, Cin), dtype=torch.float64, device=xt.device)
    ab = torch.empty_like(out) if want_abs else None
    for i, v in _gather(xt, taps, S, iy0, ix0, GH, GW):
        v2 = v.reshape(-1, Cin)
        out[i] = _mm_long(g2, v2)
        if want_abs:
            ab[i] = _mm_long(ga, v2.abs())
    return out, ab


def _mm_long(a, b, chunk=1 << 14):
    """a [M, P] @ b [P, K] for a long P (every pixel of a batch) as a batch of P/chunk products summed in fp64: a GEMM library
    runs a 16 x 4M x 16 product on a handful of workgroups (values are exact either way)"""
    P = a.shape[1]
    if P <= 4 * chunk:
        return a @ b
    nb = (P + chunk - 1) // chunk
    pad = nb * chunk - P
    a = torch.nn.functional.pad(a, (0, pad)).view(a.shape[0], nb, chunk).transpose(0, 1)
    b = torch.nn.functional.pad(b, (0, 0, 0, pad)).view(nb, chunk, b.shape[1])
    return torch.bmm(a, b).sum(0)


def wgrad_scatter(dW, dst_numel, taps, sm, sk, Cout_valid, Cin_valid, dst_offset=0, init=None):
    """ubr_wgrad_reduce's scatter: dst[dst_offset + co*sm + ci*sk + tapidx[t]] (+)= dW[t][co][ci] for co < Cout_valid,
    ci < Cin_valid.  init: the destination before the launch (fp64, accumulate); returns (value, touched-mask) flat fp64 / bool"""
    dev = dW.device
    out = torch.zeros(dst_numel, dtype=torch.float64, device=dev) if init is None else init.double().to(dev).clone()
    touched = torch.zeros(dst_numel, dtype=torch.bool, device=dev)
    co = torch.arange(Cout_valid, device=dev).view(-1, 1)
    ci = torch.arange(Cin_valid, device=dev).view(1, -1)
    for t, tp in enumerate(taps):
        idx = (dst_offset + co * sm + ci * sk + tp[2]).reshape(-1)
        out.index_add_(0, idx, dW[t, :Cout_valid, :Cin_valid].reshape(-1))
        touched[idx] = True
    return out, touched


# ------------------------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------------------------
def budget_ok(absref, unit):
    return float(absref.max()) < 2.0 ** 24 * unit if absref.numel() else True


def assert_exact(got, ref, dtype, absref=None, unit=None, what=""):
    """got (stored, `dtype`) must equal round_to(ref, dtype) element for element (+0 == -0).  With absref / unit, first
    asserts the budget max(absref) < 2^24 * unit that makes every fp32 summation order exact, and that ref is on the grid."""
    if absref is not None:
        assert unit is not None
        amax = float(absref.max()) if absref.numel() else 0.0
        assert amax < 2.0 ** 24 * unit, "%s: budget %.6g units >= 2^24: not an exact case" % (what, amax / unit)
        q = ref / unit
        fin = torch.isfinite(q)
        assert torch.equal(q[fin], q[fin].round()), "%s: reference not on the 2^%d grid" % (what, round(math.log2(unit)))
    exp = round_to(ref, dtype).to(got.device)
    g = got.float()
    e = exp.float()
    bad = ~((g == e) | (torch.isnan(g) & torch.isnan(e)))
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        nb = int(bad.sum())
        bud = (" budget %.6g units" % (float(absref[tuple(idx)]) / unit)) if absref is not None else ""
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, expected %r (fp64 %r)%s"
                             % (what, nb, bad.numel(), tuple(idx), float(g[tuple(idx)]), float(e[tuple(idx)]),
                                float(ref[tuple(idx)]), bud))


def bound(ref, absref, dtype, K):
    return C_OUT * UNIT_ROUNDOFF[dtype] * ref.abs() + C_ACC * K * U32 * absref


def assert_bounded(got, ref, absref, dtype, K, what=""):
    """|got - ref| <= C_OUT * u_out * |ref| + C_ACC * K * 2^-24 * absref per element (K: terms per output)"""
    ref = ref.to(got.device)
    assert_within(got, ref, bound(ref, absref.to(got.device), dtype, K), what)


def assert_within(got, ref, lim, what=""):
    """|got - ref| <= lim per element"""
    ref, lim = ref.to(got.device), lim.to(got.device)
    err = (got.double() - ref).abs()
    bad = ~(err <= lim)
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d elements outside the bound; first at %s: got %r, fp64 %r, |err| %.3e > %.3e"
                             % (what, int(bad.sum()), tuple(idx), float(got[tuple(idx)]), float(ref[tuple(idx)]),
                                float(err[tuple(idx)]), float(lim[tuple(idx)])))


# ------------------------------------------------------------------------------------------------------------------
# replay buffers (shared by test_gpu_kernels_exact.py and test_gpu_stream_exact.py)
# ------------------------------------------------------------------------------------------------------------------
ESZ = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2}
_ITY = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class TV:
    """an NHWC tensor view as a recorded call saw it: shape, strides, dtype, storage group and byte address"""

    def __init__(self, t, gid=None):
        self.shape, self.stride, self.dtype = tuple(t.shape), tuple(t.stride()), t.dtype
        self.ptr = t.data_ptr()
        self.gid = gid if gid is not None else t.untyped_storage().data_ptr()

    @classmethod
    def make(cls, shape, stride, dtype, gid, ptr):
        t = cls.__new__(cls)
        t.shape, t.stride, t.dtype, t.gid, t.ptr = tuple(shape), tuple(stride), dtype, gid, ptr
        return t

    def extent(self):
        return 1 + sum((n - 1) * s for n, s in zip(self.shape, self.stride))

    def key(self, base):
        return (self.shape, self.stride, str(self.dtype), self.ptr - base)


class Buffers:
    """one sentinel-filled buffer per storage group, big enough for the group's views, same 256-byte alignment"""

    def __init__(self, views, device="cuda"):
        self.groups = {}
        for v in views:
            g = self.groups.setdefault(v.gid, {"dtype": v.dtype, "lo": v.ptr, "hi": v.ptr})
            assert g["dtype"] == v.dtype, "views of one storage with different element types"
            g["lo"] = min(g["lo"], v.ptr)
            g["hi"] = max(g["hi"], v.ptr + v.extent() * ESZ[v.dtype])
        for g in self.groups.values():
            esz = ESZ[g["dtype"]]
            g["m"] = (256 + g["lo"] % 256) // esz
            n = g["m"] + (g["hi"] - g["lo"]) // esz + 256 // esz
            g["buf"] = torch.full((n,), float("nan"), dtype=g["dtype"], device=device)
            g["written"] = torch.zeros(n, dtype=torch.bool, device=device)

    def _strided(self, what, v):
        g = self.groups[v.gid]
        return g[what].as_strided(v.shape, v.stride, g["m"] + (v.ptr - g["lo"]) // ESZ[v.dtype])

    def view(self, v):
        return self._strided("buf", v)

    def mark_written(self, v):
        self._strided("written", v).fill_(True)

    def snapshot(self):
        return {k: g["buf"].clone() for k, g in self.groups.items()}

    def check_sentinel(self, snap, what):
        for k, g in self.groups.items():
            assert_untouched(g["buf"], snap[k], g["written"], what)


def assert_untouched(buf, before, written, what=""):
    """every element of `buf` outside the boolean map `written` (None: nothing may change) still holds `before`'s bits"""
    ity = _ITY[buf.element_size()]
    bad = buf.reshape(-1).view(ity) != before.reshape(-1).view(ity)
    if written is not None:
        bad &= ~written.reshape(-1)
    assert not bool(bad.any()), "%s: wrote %d elements outside its output view(s)" % (what, int(bad.sum()))


def stats_eps(L):
    """(eps1, eps2) of the per-channel statistics bound for an fp32 partial chain of L (see the note at the top)"""
    return gamma(L) + 2.0 ** -50, gamma(L + 1) + 2.0 ** -50


def assert_stats(s, refs, L, unit=None, unit2=None, what=""):
    """s: fp64 [2C] = the slots summed; refs = conv_stats_ref(...).  Exact when both budgets hold (sum |terms| < 2^24 units
    of the term grid, v^2 exact in fp32), else |s - ref| <= eps * sum |terms| per channel.  Returns 'exact' / 'bounded'."""
    s1r, s2r, a1, a2 = (t.to(s.device) for t in refs)
    C = s1r.numel()
    s1, s2 = s[:C], s[C:2 * C]
    if unit2 is None and unit is not None:
        unit2 = unit * unit
    exact = unit is not None and float(a1.max()) < 2.0 ** 24 * unit and float(a2.max()) < 2.0 ** 24 * unit2
    if exact:
        for nm, a, b in (("sum", s1, s1r), ("sum of squares", s2, s2r)):
            if not torch.equal(a, b):
                c = int((a != b).nonzero()[0])
                raise AssertionError("%s: stats %s of channel %d: got %r, exact %r" % (what, nm, c, float(a[c]), float(b[c])))
        return "exact"
    e1, e2 = stats_eps(L)
    for nm, a, b, ab, e in (("sum", s1, s1r, a1, e1), ("sum of squares", s2, s2r, a2, e2)):
        err = (a - b).abs()
        bad = ~(err <= e * ab)
        if bool(bad.any()):
            c = int(bad.nonzero()[0])
            raise AssertionError("%s: stats %s of channel %d: got %r, fp64 %r, |err| %.3e > %.2e * %.3e"
                                 % (what, nm, c, float(a[c]), float(b[c]), float(err[c]), e, float(ab[c])))
    return "bounded"


# ------------------------------------------------------------------------------------------------------------------
# streaming kernels (csrc/ubr_elem.hip, csrc/ubr_head.hip): the elementwise formulas of include/ubresnet_hip.h in fp64
# ------------------------------------------------------------------------------------------------------------------
def _vec(v, ref):
    return v.double().to(ref.device)


def _bn(c, mean, scale, shift):
    return (c.double() - _vec(mean, c)) * _vec(scale, c) + _vec(shift, c)


def tail_fwd_ref(c2, mean2, scale2, shift2, sc, mean_b=None, scale_b=None, shift_b=None):
    """out = relu( relu(bn2(c2)) + shortcut ), shortcut = bnpass(sc) (mean_b given) or sc; fp64 NHWC"""
    r2 = _bn(c2, mean2, scale2, shift2).clamp_min(0)
    sh = sc.double() if mean_b is None else _bn(sc, mean_b, scale_b, shift_b)
    return (r2 + sh).clamp_min(0)


def mask_pack(positive, cpu):
    """bool [..., C] -> uint8 [npix * C/cpu]: bit e of byte (pixel, unit) = channel e of the unit (the block tail's ReLU mask)"""
    C = positive.shape[-1]
    b = positive.reshape(-1, C // cpu, cpu).to(torch.int32)
    w = (1 << torch.arange(cpu, device=positive.device, dtype=torch.int32))
    return (b * w).sum(-1).to(torch.uint8).reshape(-1)


def mask_unpack(mask, shape, cpu):
    """uint8 [>= npix * C/cpu] -> bool of `shape` (NHWC)"""
    return mask_bits(mask, shape, cpu) > 0


def fma64(a, b, c):
    """round(a*b + c) of fp64 tensors with ONE rounding, as v_fma_f64 does: the product's rounding error exactly (Veltkamp split,
    Dekker), the sum by TwoSum; the last addition can double-round only on a tie at the 2^-106 level"""
    def split(x):
        t = x * 134217729.0
        h = t - (t - x)
        return h, x - h
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def bn_finalize_ref(s1, s2, count, gamma, beta, eps, rmean=None, rvar=None, momentum=0.1, fused=False):
    """ubr_bn_finalize's arithmetic in fp64 from the summed statistics: (scale, shift, mean, invstd, running_mean, running_var),
    every vector rounded to fp32 once as the kernel stores it.  momentum: the factor in fp64 (the kernel widens its fp32 argument;
    for cumulative averaging the caller passes float32(1 / (batches tracked + 1))).
    fused: the two contractions C++ allows and hipcc makes in bn_finalize_kernel -- var = fma(-m, m, s2/count) and
    running = fma(new, momentum, fl((1 - momentum) * running)); either form is a correct evaluation of the kernel's statements."""
    s1, s2 = s1.double(), s2.double()
    m = s1 / count
    var = (fma64(-m, m, s2 / count) if fused else s2 / count - m * m).clamp_min(0)
    inv = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    scale = (_vec(gamma, s1) * inv).float()
    out = [scale, beta.float().to(s1.device), m.float(), inv.float(), None, None]
    if rmean is not None:
        unb = var * count / (count - 1.0) if count > 1.0 else var
        if fused:
            mom = torch.full_like(m, momentum)
            out[4] = fma64(m, mom, (1.0 - momentum) * _vec(rmean, s1)).float()
            out[5] = fma64(unb, mom, (1.0 - momentum) * _vec(rvar, s1)).float()
        else:
            out[4] = ((1.0 - momentum) * _vec(rmean, s1) + momentum * m).float()
            out[5] = ((1.0 - momentum) * _vec(rvar, s1) + momentum * unb).float()
    return tuple(out)


def bn_bwd_ref(ga, ga2, c, scale, shift, mean, invstd, relu):
    """-> (g_y, xhat) fp64: g_y = (ga + ga2) * [bn(c) > 0] (relu) and xhat = (c - mean) * invstd"""
    g = ga.double() if ga2 is None else ga.double() + ga2.double()
    d = c.double() - _vec(mean, c)
    if relu:
        g = torch.where(d * _vec(scale, c) + _vec(shift, c) > 0, g, torch.zeros((), dtype=g.dtype, device=g.device))
    return g, d * _vec(invstd, c)


def tail_bwd_ref(go, go2, positive, c2, scale2, shift2, mean2, invstd2, cb=None, mean_b=None, invstd_b=None):
    """backward operands of a block tail: positive = [out > 0] (bool NHWC, from `out` or from the mask bits).
    -> (g_z, g_y2, xhat2, xhat_b): g_z = (go + go2)*positive (gradient into the shortcut branch), g_y2 = g_z*[bn2(c2) > 0]"""
    g = go.double() if go2 is None else go.double() + go2.double()
    zero = torch.zeros((), dtype=g.dtype, device=g.device)
    gz = torch.where(positive, g, zero)
    d2 = c2.double() - _vec(mean2, c2)
    gy2 = torch.where(d2 * _vec(scale2, c2) + _vec(shift2, c2) > 0, gz, zero)
    xhb = None if cb is None else (cb.double() - _vec(mean_b, cb)) * _vec(invstd_b, cb)
    return gz, gy2, d2 * _vec(invstd2, c2), xhb


def reduce_ref(gy, xhat=None):
    """per-channel sums of a reduce pass and the sums of |terms| (the budget): (sum g_y, sum g_y*xhat, a1, a2), fp64 [C]"""
    C = gy.shape[-1]
    g = gy.reshape(-1, C)
    if xhat is None:
        return g.sum(0), None, g.abs().sum(0), None
    t = g * xhat.reshape(-1, C)
    return g.sum(0), t.sum(0), g.abs().sum(0), t.abs().sum(0)


def apply_ref(gy, xhat, scale, k1, k2):
    """pass 2: g_c = scale * (g_y - k1 - xhat*k2)"""
    return _vec(scale, gy) * (gy - _vec(k1, gy) - xhat * _vec(k2, gy))


def bn_bwd_frozen_ref(ga, ga2, c, scale, shift, mean, invstd, relu):
    """backward through a = relu(bn(c)) (or bn(c)) at a FROZEN site -- mean / invstd are constants of the pass, so no sum stands
    between the incoming gradient and the data gradient:  g_c = scale * g_y,  dbeta = sum g_y,  dgamma = sum g_y * xhat.
    -> (g_c fp64 NHWC, (dbeta, sum |terms|), (dgamma, sum |terms|)), the sums fp64 [C]"""
    gy, xh = bn_bwd_ref(ga, ga2, c, scale, shift, mean, invstd, relu)
    s, sx, a1, a2 = reduce_ref(gy, xh)
    return _vec(scale, gy) * gy, (s, a1), (sx, a2)


def tail_bwd_frozen_ref(go, go2, positive, c2, scale2, shift2, mean2, invstd2, cb=None, scale_b=None, mean_b=None, invstd_b=None):
    """backward of a block tail out = relu(relu(bn2(c2)) + shortcut) whose BatchNorm sites are all frozen; positive = [out > 0]:
        g_z = (go + go2) * positive,   g_y2 = g_z * [bn2(c2) > 0],   g_c2 = scale2 * g_y2,   dbeta2 = sum g_y2,  dgamma2 = sum g_y2 * xhat2
        bypass block (shortcut = bnpass(cb)): g_sc = scale_b * g_z,  dbeta_b = sum g_z,  dgamma_b = sum g_z * xhat_b;   identity: g_sc = g_z
    -> (g_c2, g_sc, [(dbeta2, abs), (dgamma2, abs)], [(dbeta_b, abs), (dgamma_b, abs)] or None)"""
    gz, gy2, xh2, xhb = tail_bwd_ref(go, go2, positive, c2, scale2, shift2, mean2, invstd2, cb, mean_b, invstd_b)
    s, sx, a1, a2 = reduce_ref(gy2, xh2)
    if cb is None:
        return _vec(scale2, gy2) * gy2, gz, [(s, a1), (sx, a2)], None
    sb, sxb, b1, b2 = reduce_ref(gz, xhb)
    return _vec(scale2, gy2) * gy2, _vec(scale_b, gz) * gz, [(s, a1), (sx, a2)], [(sb, b1), (sxb, b2)]


def assert_sums_exact(got, ref, absref, unit, what=""):
    """a striped fp64 sum against its reference: asserts the budget (sum of |terms| of a channel < 2^24 units of the term grid:
    every fp32 partial of every summation order is then exact, see the note on the reduce passes at the top) and equality"""
    assert budget_ok(absref, unit), "%s: budget %.6g units >= 2^24: not an exact case" % (what, float(absref.max()) / unit)
    ref = ref.to(got.device)
    if not torch.equal(got, ref):
        c = int((got != ref).nonzero()[0])
        raise AssertionError("%s: channel %d: got %r, exact %r (%d of %d channels differ)"
                             % (what, c, float(got[c]), float(ref[c]), int((got != ref).sum()), ref.numel()))


def pool_out(n, stride):
    return (n - 1) // stride + 1


def maxpool_ref(x, xf, stride):
    """nn.MaxPool2d(3, stride, 1) of xform(x): (pooled, argmax, transformed input), fp64 / int64 tap index ky*3+kx of the FIRST
    maximum in scan order among the taps inside the image (strict > update, as ATen's CPU kernel)"""
    v = _xform(x, xf)
    N, H, W, C = v.shape
    OH, OW = pool_out(H, stride), pool_out(W, stride)
    vp = torch.nn.functional.pad(v, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    best = torch.full((N, OH, OW, C), float("-inf"), dtype=torch.float64, device=v.device)
    am = torch.full((N, OH, OW, C), -1, dtype=torch.int64, device=v.device)
    for t in range(9):
        ky, kx = t // 3, t % 3
        w = vp[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride, :]
        upd = (w > best) | ((am < 0) & (w > float("-inf")))
        best = torch.where(upd, w, best)
        am = torch.where(upd, torch.full_like(am, t), am)
    return best, am, v


def maxpool_bwd_ref(g_pooled, argmax, in_hw, stride, g_extra=None):
    """gx = g_extra + scatter of g_pooled through the arg-max taps; fp64 [N,H,W,C]"""
    H, W = in_hw
    gp = g_pooled.double()
    N, OH, OW, C = gp.shape
    acc = torch.zeros((N, H + 2, W + 2, C), dtype=torch.float64, device=gp.device)
    for t in range(9):
        ky, kx = t // 3, t % 3
        acc[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride, :] += \
            torch.where(argmax.to(gp.device) == t, gp, torch.zeros((), dtype=gp.dtype, device=gp.device))
    gx = acc[:, 1:H + 1, 1:W + 1, :]
    return gx + g_extra.double() if g_extra is not None else gx.clone()


def stem_expand_ref(x):
    """NCHW [N,Cin,H,W] -> NHWC [N,H,W,16*Cin]: channel 16*ci+kx = plane ci shifted by kx-3 columns (kx < 7), zero otherwise"""
    N, Cin, H, W = x.shape
    out = torch.zeros((N, H, W, 16 * Cin), dtype=torch.float64, device=x.device)
    xp = torch.nn.functional.pad(x.double(), (3, 3))
    for ci in range(Cin):
        for kx in range(7):
            out[..., 16 * ci + kx] = xp[:, ci, :, kx:kx + W]
    return out


# ubr_logsoftmax_bwd: per pixel, in fp32, s = sum_c g_c (exact on dyadic g), o_c = g_c - expf(lp_c) * s, stored as T.
# The test hands the kernel lp^ = fl32(log p) of a dyadic probability p and compares with g - p*s in fp64.  With u = 2^-24:
#   lp^ = log p + e0, |e0| <= u |log p|:  exp(lp^) = p (1 + e0 + ...);   expf within 2 ulp: relative 4u (kref's convention
#   above);  so e^ = p (1 + d), |d| <= u (|log p| + 4) to first order.   fl(e^ * s): + u |p s|.   fl(g - .): + u |o|.
#   Hence |o^ - o| <= u (|p s| (|log p| + 5) + |o|), times C_ACC for the second-order terms; a 16-bit T rounds once more:
#   + u_T (|o| + that).  Channels >= C of the 16 stored are written as exact zeros.
def logsoftmax_bwd_ref(g, p, dtype):
    """g, p: fp64 NCHW (gradient w.r.t. log-probabilities; the probabilities) -> (g_logits fp64 NHWC [N,H,W,C], bound)"""
    s = g.sum(1, keepdim=True)
    ref = g - p * s
    lim = C_ACC * U32 * ((p * s).abs() * (p.log().abs() + 5.0) + ref.abs())
    if dtype != torch.float32:
        lim = lim + UNIT_ROUNDOFF[dtype] * (ref.abs() + lim)
    return ref.permute(0, 2, 3, 1), lim.permute(0, 2, 3, 1)


def nll_ref(predict, target, pixelweights, classw, ignore_index):
    """PixelWiseNLLLoss: (sum over pixels of -predict[b,t,h,w]*classw[t]*pixelweights (the caller divides by b*h*w), the sum of
    |terms|, the number of labels outside [0,C) other than ignore_index, the mask of contributing pixels, the per-pixel weight)"""
    N, C, H, W = predict.shape
    ok = (target != ignore_index) & (target >= 0) & (target < C)
    bad = int(((target != ignore_index) & ~ok).sum())
    t = target.clamp(0, C - 1)
    w = pixelweights.double() * (classw.double().to(t.device)[t] if classw is not None else 1.0)
    terms = torch.where(ok, -predict.double().gather(1, t.unsqueeze(1)).squeeze(1) * w, torch.zeros((), dtype=torch.float64, device=t.device))
    return terms.sum(), terms.abs().sum(), bad, ok, w


def nll_bwd_ref(g_loss, target, pixelweights, classw, ignore_index, C):
    """g_predict [N,C,H,W] fp32: -(g_loss / (b*h*w)) * pixelweights * classw[t] at channel t of contributing pixels, zero elsewhere.
    The kernel forms gl = g_loss / float(total) in fp32 (one correctly rounded division; fp64 division rounded to fp32 is the same
    value) and scales it by the two weights, which the tests pick as powers of two"""
    N, H, W = target.shape
    ok = (target != ignore_index) & (target >= 0) & (target < C)
    gl = (torch.tensor(float(g_loss), dtype=torch.float64) / float(torch.tensor(float(N * H * W), dtype=torch.float32))).float().double()
    w = pixelweights.double() * (classw.double().to(target.device)[target.clamp(0, C - 1)] if classw is not None else 1.0)
    val = torch.where(ok, -gl.to(target.device) * w, torch.zeros((), dtype=torch.float64, device=target.device))
    out = torch.zeros((N, C, H, W), dtype=torch.float64, device=target.device)
    out.scatter_(1, target.clamp(0, C - 1).unsqueeze(1), val.unsqueeze(1))
    return out


def confusion_ref(logp, target):
    """cm[true*C + pred] with pred = FIRST arg-max over channels; labels outside [0,C) are not counted"""
    N, C, H, W = logp.shape
    best = logp[:, 0]
    pred = torch.zeros_like(target)
    for c in range(1, C):
        upd = logp[:, c] > best
        best = torch.where(upd, logp[:, c], best)
        pred = torch.where(upd, torch.full_like(pred, c), pred)
    ok = (target >= 0) & (target < C)
    return torch.bincount((target[ok] * C + pred[ok]).reshape(-1), minlength=C * C)


def pick_blocks(npix, CU, max_blocks=2048, min_iters=1):
    """the documented grid rule of the streaming kernels (csrc/ubr_elem.hip): workgroups of 256 threads, a multiple of
    CU / gcd(256, CU), one thread per `min_iters` units of work, capped -- for the table rows only"""
    mult = CU // math.gcd(256, CU)
    want = (npix * CU + 255) // 256
    if min_iters > 1:
        want = (want + min_iters - 1) // min_iters
    want = max(1, min(want, max_blocks))
    return (want + mult - 1) // mult * mult


# ------------------------------------------------------------------------------------------------------------------
# parameter-side launches: weight images, BatchNorm fold / finalizes, flat optimizer steps, tile crop and stitch
# (tests/test_gpu_param_exact.py; self-tests in tests/test_cpu_kref.py)
# ------------------------------------------------------------------------------------------------------------------
def bits(t):
    """the raw bit pattern of a floating tensor as integers (so that -0.0 != +0.0 and NaN == NaN)"""
    return t.contiguous().view(_ITY[t.element_size()])


def pack_ref(src_f32, M, Mpad, Kvalid, Kpad, sm, sk, taps, dtype, oscale=None, src_offset=0):
    """ubr_pack_weights / ubr_pack_item: dst[t][ku][m][e] = (T) (oscale[m] *) src[src_offset + m*sm + (ku*CPU+e)*sk + taps[t]],
    zero for m >= M and k >= Kvalid.  The gather is fp64; the scale is ONE fp32 multiply (the fp64 product of two fp32 numbers is
    exact, so .float() is that rounding); then one rounding to `dtype` (torch's .to(): round to nearest even, subnormals kept)."""
    cpu = CPU[dtype]
    src = src_f32.reshape(-1)
    assert src.dtype == torch.float32 and Mpad % 16 == 0 and Kpad % cpu == 0 and M <= Mpad and Kvalid <= Kpad
    dev = src.device
    m = torch.arange(M, device=dev).view(1, 1, M)
    k = torch.arange(Kvalid, device=dev).view(1, Kvalid, 1)
    t = torch.tensor(list(taps), dtype=torch.int64, device=dev).view(-1, 1, 1)
    v = src.double()[src_offset + m * sm + k * sk + t]                    # [T][Kvalid][M]
    if oscale is not None:
        v = (v * oscale.double().to(dev).view(1, 1, -1)[..., :M]).float().double()
    full = torch.zeros((t.numel(), Kpad, Mpad), dtype=torch.float64, device=dev)
    full[:, :Kvalid, :M] = v
    return full.float().to(dtype).view(t.numel(), Kpad // cpu, cpu, Mpad).permute(0, 1, 3, 2).contiguous()


def ulp32(x):
    """spacing of fp32 numbers at |x| (fp64 tensor): 2^(e-24) for |x| in [2^(e-1), 2^e), never below 2^-149"""
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, torch.full_like(e, -125), e).clamp_min(-125)
    return torch.ldexp(torch.ones_like(x), e - 24)


def f32(v):
    """the fp32 value a C `float` argument receives, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


def bn_fold_ref(gamma, beta, rmean, rvar, eps, conv_bias=None):
    """ubr_bn_fold_item in fp64: scale = gamma / sqrt(running_var + eps), bias = (conv_bias - running_mean) * scale + beta.
    -> (scale rounded to fp32, bias fp64, bound on |stored bias - bias|): half an fp32 ulp for the store plus 2^-50 of the terms,
    because the device may fuse the multiply-add, so the last fp64 bits are not fixed.  An fp32 evaluation misses the bound."""
    s = gamma.double() / torch.sqrt(rvar.double() + f32(eps))
    b = conv_bias.double() if conv_bias is not None else torch.zeros_like(s)
    t = (b - rmean.double()) * s
    bias = t + beta.double()
    return s.float(), bias, 0.5 * ulp32(bias) + 2.0 ** -50 * (t.abs() + beta.double().abs())


def stripe_sum(buf, slots, stride, n):
    """sum_{sl < slots} buf[sl*stride + i], i < n, added in stripe order in fp64 (the finalize / cast kernels' loop)"""
    a = torch.zeros(n, dtype=torch.float64, device=buf.device)
    for sl in range(slots):
        a = a + buf[sl * stride: sl * stride + n]
    return a


def bn_eval_affine_ref(gamma, rvar, eps):
    """fp64 (invstd, scale) of ubr_bn_eval_affine, which works in fp32: fl(rvar + eps), sqrtf, 1/ (three roundings: gamma(3) on
    invstd) and one more multiply (gamma(4) on scale)"""
    inv = 1.0 / torch.sqrt(rvar.double() + f32(eps))
    return inv, gamma.double() * inv


def bn_bwd_finalize_ref(red, C, count, dgamma0=None, dbeta0=None, accumulate=False, slots=STAT_SLOTS):
    """ubr_bn_bwd_finalize from the stripes [slots][2C] (sum g_y | sum g_y*xhat): (dgamma, dbeta, k1, k2) as stored (fp32).
    accumulate adds the fp32-rounded sum onto the old fp32 value: one more fp32 rounding.  count None: the frozen form, k = 0."""
    s = stripe_sum(red.reshape(-1), slots, 2 * C, 2 * C)
    sg, sgx = s[:C], s[C:]
    dg, db = sgx.float(), sg.float()
    if accumulate:
        dg, db = (dgamma0.double() + dg.double()).float(), (dbeta0.double() + db.double()).float()
    if count is None:
        return dg, db, torch.zeros_like(dg), torch.zeros_like(dg)
    return dg, db, (sg / count).float(), (sgx / count).float()


def cast_ref(src, stride, slots, n, scale=1.0, dst0=None, accumulate=False):
    """ubr_cast_f64_to_f32: dst[i] (+)= fl32(scale * sum_slots src[slot*stride + i])"""
    v = (stripe_sum(src.reshape(-1), slots, stride, n) * float(scale)).float()
    return (dst0.double() + v.double()).float() if accumulate else v


# Flat optimizer steps (csrc/ubr_head.hip: adam_kernel, sgd_kernel).  The references are torch.optim's single-tensor formulas in
# fp64 from the kernel's fp32 inputs; with them comes a running-error bound |fp32 result - fp64 value| <= bound, built from
# gamma(k), k = the number of fp32 roundings on the path of a term, applied to the ABSOLUTE values of the terms (so that the
# cancellation in gr - m is covered).  A fused multiply-add drops a rounding, never adds one: the counts assume none is fused, so
# the bound holds either way.  Common to both: gr = wd*p + g*grad_scale: each term is rounded by its multiply and by the add, k = 2.
def _grad_term(p, g, wd, gs):
    gr = g * gs + wd * p
    return gr, (g * gs).abs() + (wd * p).abs()


def adam_ref(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, round_bc=True):
    """one torch.optim.Adam step (L2 weight decay, no amsgrad) -> ((param, exp_avg, exp_avg_sq) fp64, (bounds) fp64).
    round_bc: the bias corrections as ubr_adam_step forms them -- pow in double, 1 - beta1^step and sqrt(1 - beta2^step) rounded to
    fp32 (False: kept in double, which is torch.optim's arithmetic)."""
    lr, b1, b2, eps, wd, gs = (f32(x) for x in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    bc1, sbc2 = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    if round_bc:
        bc1, sbc2 = f32(bc1), f32(sbc2)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    gr, A_gr = _grad_term(p, g, wd, gs)
    c1, c2 = 1.0 - b1, 1.0 - b2
    m1 = m + c1 * (gr - m)
    v1 = b2 * v + c2 * gr * gr
    den = torch.sqrt(v1) / sbc2 + eps
    step_size = lr / bc1
    r = m1 / den
    p1 = p - step_size * r
    # exp_avg: k = 6 on the term c1*gr (gr 2, the subtraction, fl(1 - beta1), the multiply, the add), fewer on m and c1*m
    E_m = gamma(6) * (m.abs() + c1 * (A_gr + m.abs()))
    # exp_avg_sq: k = 9 on the term c2*gr*gr (gr twice: 4, fl(1 - beta2), two multiplies, the add), 2 on beta2*v
    A_v = b2 * v.abs() + c2 * A_gr * A_gr
    E_v = gamma(9) * A_v
    # param: running error through sqrtf (1), / sqrt_bc2 (1), + eps (1), exp_avg / denom (1), step_size = fl(lr / bc1) (1),
    # the multiply (1) and the subtraction (1): k = 4 on the update term, 1 on p, plus what E_m and E_v carry in
    sq = torch.sqrt(v1)
    E_s = torch.minimum(torch.sqrt(E_v), E_v / sq.clamp_min(1e-300))             # |sqrt(a) - sqrt(b)| <= min(sqrt|a-b|, |a-b|/sqrt(b))
    q = sq / sbc2
    E_q = (E_s / sbc2) * (1.0 + gamma(2)) + gamma(2) * q
    E_den = E_q + gamma(1) * (q + eps + E_q)
    lo = (den - E_den).clamp_min(1e-300)
    E_r = (E_m + r.abs() * E_den) / lo
    E_r = E_r + gamma(1) * (r.abs() + E_r)
    E_t = step_size * (E_r * (1.0 + gamma(2)) + gamma(2) * r.abs())
    E_p = E_t + gamma(1) * (p.abs() + step_size * r.abs() + E_t)
    return (p1, m1, v1), (E_p, E_m, E_v)


def sgd_ref(p, g, buf, lr, momentum, dampening, weight_decay, nesterov, first_step, grad_scale=1.0):
    """one torch.optim.SGD step -> ((param, momentum buffer or None) fp64, (bounds)).  buf None iff momentum == 0; on the first
    step the buffer is the gradient and is NOT read."""
    lr, mom, damp, wd, gs = (f32(x) for x in (lr, momentum, dampening, weight_decay, grad_scale))
    p, g = p.double(), g.double()
    gr, A_gr = _grad_term(p, g, wd, gs)
    k_gr, b1, E_b = 2, None, None
    if momentum != 0:
        if first_step:
            b1, A_b, k_b = gr, A_gr, 2                     # momentum buffer, first step: the gradient itself, k = 2
        else:
            b = buf.double()
            c = 1.0 - damp
            b1 = mom * b + c * gr
            A_b = (mom * b).abs() + c * A_gr
            k_b = 5                                        # momentum buffer: k = 5 on c*gr (gr 2, fl(1 - dampening), multiply, add)
        E_b = gamma(k_b) * A_b
        if nesterov:
            gr, A_gr, k_gr = gr + mom * b1, A_gr + mom * A_b, k_b + 2      # momentum*buf: buf's k, the multiply, the add
        else:
            gr, A_gr, k_gr = b1, A_b, k_b
    p1 = p - lr * gr
    # param: k = k_gr + 2 on the update term (the multiply by lr and the subtraction: at most 9), 1 on p
    E_p = gamma(1) * p.abs() + gamma(k_gr + 2) * lr * A_gr
    return (p1, b1), (E_p, E_b)


def crop_tiles_ref(view, desc, th, tw):
    """ubr_crop_tiles with plain index loops: view numpy [P][rows][cols], desc rows (plane, r0, c0, ...) -> [ntiles][th][tw];
    pixels of a tile beyond the view are zero"""
    import numpy as np
    P, rows, cols = view.shape
    out = np.zeros((len(desc), th, tw), dtype=view.dtype)
    for t, d in enumerate(desc):
        for y in range(th):
            sy = d[1] + y
            if sy >= rows:
                break
            n = max(0, min(tw, cols - d[2]))
            out[t, y, :n] = view[d[0], sy, d[2]:d[2] + n]
    return out


def stitch_tiles_ref(scores, desc, out):
    """ubr_stitch_tiles with plain index loops, in place on `out` numpy [P][C][rows][cols]: tile pixels inside the keep window
    (kr0, kr1, kc0, kc1, tile coordinates) go to out[plane][c][r0 + y][c0 + x] where that lies inside the view"""
    P, C, rows, cols = out.shape
    for t, d in enumerate(desc):
        p, r0, c0, kr0, kr1, kc0, kc1 = d
        for y in range(kr0, kr1):
            if r0 + y >= rows:
                break
            for x in range(kc0, kc1):
                if c0 + x >= cols:
                    break
                out[p, :, r0 + y, c0 + x] = scores[t, :, y, x]
    return out


# ------------------------------------------------------------------------------------------------------------------
# edge values of the storage types (self-test in tests/test_cpu_kref.py)
# ------------------------------------------------------------------------------------------------------------------
# exact_operands() never puts a kernel's store on a rounding tie, past the largest finite value of the storage type, on a
# subnormal, a signed zero, an infinity or a NaN.  edge_table() lists such fp32 values by CLASS, built from bit patterns:
# the midpoint of two neighbours of T is the fp64 mean of the two (exact in fp32: T has at most 11 significant bits), its
# fp32 neighbours are the bit pattern +- 1.  Every class comes in both signs.  The reference rounding is torch's .to(T):
# round to nearest even, subnormals kept, NaN stays NaN.
FLT_MAX_BITS = 0x7f7fffff
_T_INFO = {      # (bit patterns b of T whose midpoint with b + 1 is listed: even b, odd b; largest finite; largest subnormal; smallest normal)
    torch.bfloat16: ((0x3f80, 0x2f82, 0x4a7e, 0x0002, 0x7f00), (0x3f81, 0x2f83, 0x4a7f, 0x0003, 0x7f01), 0x7f7f, 0x007f, 0x0080),
    torch.float16: ((0x3c00, 0x1402, 0x6bfe, 0x0002, 0x7800), (0x3c01, 0x1403, 0x6bff, 0x0003, 0x7801), 0x7bff, 0x03ff, 0x0400),
}
NAN_CLASSES = ("nan", "nan_low_payload")


def _from_bits32(b):
    return torch.tensor([x - (1 << 32) if x >= (1 << 31) else x for x in b], dtype=torch.int64).to(torch.int32).view(torch.float32)


def _t_value(b, dtype):
    """the fp32 value of bit pattern b of the 16-bit type"""
    return float(torch.tensor([b], dtype=torch.int32).to(torch.int16).view(dtype).float())


def _bits_of(x):
    return int(torch.tensor([x], dtype=torch.float32).view(torch.int32)) & 0xffffffff


def edge_table(dtype):
    """[(class name, fp32 bit pattern)] of the edge values of storage type `dtype`, positive sign first, then every entry
    again with the sign bit set (names prefixed '-')"""
    rows = [("f32_subnormal_min", 0x00000001), ("f32_subnormal", 0x00012345), ("f32_subnormal_max", 0x007fffff),
            ("zero", 0x00000000), ("inf", 0x7f800000), ("nan", 0x7fc00000), ("flt_max", FLT_MAX_BITS)]
    if dtype != torch.float32:
        even, odd, tmax, submax, normmin = _T_INFO[dtype]
        for nm, bs in (("tie_even", even), ("tie_odd", odd)):
            for b in bs:
                mid = (torch.tensor(_t_value(b, dtype), dtype=torch.float64) + _t_value(b + 1, dtype)) / 2
                assert float(mid.float().double()) == float(mid)
                mb = _bits_of(float(mid))
                rows += [(nm, mb), (nm + "_above", mb + 1), (nm + "_below", mb - 1)]
        top = _t_value(tmax, dtype)
        ovf = _bits_of(top + (top - _t_value(tmax - 1, dtype)) / 2)           # largest finite + half a T-ulp
        smin = _t_value(1, dtype)
        rows += [("t_max", _bits_of(top)), ("overflow_tie", ovf), ("overflow_below", ovf - 1),
                 ("t_subnormal_min", _bits_of(smin)), ("t_subnormal_half", _bits_of(smin / 2)), ("t_subnormal_half_above", _bits_of(smin / 2) + 1),
                 ("t_subnormal_max", _bits_of(_t_value(submax, dtype))), ("t_normal_min", _bits_of(_t_value(normmin, dtype))),
                 # a NaN whose payload lies in the low 16 bits only: truncation, or adding 0x7fff before it, gives infinity
                 ("nan_low_payload", 0x7f800001)]
    return rows + [("-" + n, b | 0x80000000) for n, b in rows]


def edge_values(dtype, classes=None, exclude=()):
    """fp32 tensor of the edge values of `dtype` (edge_table order); classes / exclude filter by class name without the sign"""
    rows = [(n, b) for n, b in edge_table(dtype) if (classes is None or n.lstrip("-") in classes) and n.lstrip("-") not in exclude]
    return _from_bits32([b for _, b in rows])


def tie_bases(dtype):
    """{class: T bit patterns b whose midpoint with b + 1 the table lists} (for the self-test: neighbours from bit patterns)"""
    return {"tie_even": _T_INFO[dtype][0], "tie_odd": _T_INFO[dtype][1]}


def edge_names(dtype, classes=None, exclude=()):
    return [n for n, _ in edge_table(dtype) if (classes is None or n.lstrip("-") in classes) and n.lstrip("-") not in exclude]


def assert_bits(got, expected, zero_sign=True, what=""):
    """equal bit patterns element for element: +0 != -0 (unless zero_sign is False, for a formula that leaves the sign of a zero
    open), any NaN matches any NaN and nothing else"""
    assert got.shape == expected.shape and got.dtype == expected.dtype, "%s: %s %s vs %s %s" % (what, tuple(got.shape), got.dtype, tuple(expected.shape), expected.dtype)
    e = expected.to(got.device)
    if got.is_floating_point():
        gn, en = torch.isnan(got), torch.isnan(e)
        same = bits(got) == bits(e)
        if not zero_sign:
            same = same | ((got == 0) & (e == 0))
        bad = ~((same & ~gn & ~en) | (gn & en))
    else:
        bad = got != e
    if bool(bad.any()):
        idx = tuple(bad.nonzero()[0].tolist())
        if got.is_floating_point():
            gb, eb = int(bits(got)[idx]), int(bits(e)[idx])
        else:
            gb, eb = int(got[idx]), int(e[idx])
        m = (1 << (8 * got.element_size())) - 1
        raise AssertionError("%s: %d of %d elements differ in bits; first at %s: got %r (0x%x), expected %r (0x%x)"
                             % (what, int(bad.sum()), bad.numel(), idx, float(got[idx]), gb & m, float(e[idx]), eb & m))


# ------------------------------------------------------------------------------------------------------------------
# launches replayed on operands that are NOT exact (tests/stage_shadow.py: the stages of a pass at realistic magnitudes, every
# launch against fp64 of its own recorded inputs).  No new constant: every bound below is gamma(k) -- k fp32 roundings on the
# path of a term, applied to the sum of the ABSOLUTE values of the terms -- plus one rounding to the stored type, i.e.
# bound(ref, absref, dtype, k) above, plus half the smallest subnormal of the stored type (TINY: a store can miss by that much
# however small the value is; for f16 that is 2^-25, which gradients do reach).
# ------------------------------------------------------------------------------------------------------------------
# ET<T>::pack / ET<T>::st (csrc/ubr_common.h) convert with plain casts, (__bf16)v and (_Float16)v: v_cvt_pk_bf16_f32 / v_cvt_f16_f32,
# round to nearest even with gradual underflow (the f16 denormal mode of a HIP kernel is on by default; nothing in the build turns
# it off), so a store misses by at most half the subnormal spacing.  A store that flushed subnormals would miss by up to 2^-14 in
# f16 and fall outside these bounds.  TINY is added only where an output has a nonzero term: an output all of whose terms are
# zero is exactly zero, and its bound is zero.
TINY = {torch.float32: 2.0 ** -150, torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}


def affine_terms(v, mean, scale, shift):
    """(bn, sum of |terms|, d) of bn = fma(fl(v - mean), scale, shift) in fp64.  The kernels form it with TWO fp32 roundings (the
    difference, the fused multiply-add), so |bn^ - bn| <= gamma(2) * (|d*scale| + |shift|)."""
    d = v.double() - _vec(mean, v)
    p = d * _vec(scale, v)
    return p + _vec(shift, v), p.abs() + _vec(shift, v).abs(), d


def gate_open(bn, terms):
    """elements whose ReLU gate [bn > 0] the fp32 evaluation may decide either way: |bn| within its own error gamma(2) * terms"""
    return bn.abs() <= gamma(2) * terms


def xf_operand_err(x, xf, dtype):
    """An MFMA operand formed on load: t = max(fma(fl(x - sub), scale, shift), lo) in fp32 (ubr_bnrelu: two roundings, the max is
    1-Lipschitz), then packed to the compute type T (ET<T>::pack: one rounding, relative u_T, or TINY).  Per element
        |x^ - t| <= u_T |t| + (1 + u_T) gamma(2) (|(x - sub) scale| + |shift|) + TINY.
    A conv / weight gradient then carries sum |w| * that on top of its accumulation bound (conv_ref of this tensor with |W|).
    -> fp64 tensor of x's shape; zero without a transform (operands are read as stored)."""
    if xf is None:
        return torch.zeros(x.shape, dtype=torch.float64)
    sub, scale, shift, lo = xf
    C = x.shape[-1]
    bn, terms, _ = affine_terms(x, sub[:C], scale[:C], shift[:C])
    t = torch.maximum(bn, _vec(lo, x)[:C])
    u = UNIT_ROUNDOFF[dtype]
    return u * t.abs() + (1.0 + u) * gamma(2) * terms + TINY[dtype] * (terms > 0)


# The stem's pool (maxpool_fwd_kernel with XF, XCOPY, AMAX): every tap is t^ = max(fma(fl(x - sub), scale, shift), lo) in fp32, the
# window maximum m^ and its tap index are taken on those fp32 values (strict >, first maximum), and both xcopy = pack(t^) and
# pooled = pack(m^) are stored ONCE.
#   * xcopy: |t^ - t| <= pre and one store: stored_bound(t, pre, T), with pre = xf_operand_err (which, being the bound of a PACKED
#     operand, already holds one rounding to T: the bound is that much wider than the arithmetic needs, never narrower).
#   * pooled: |max_i a_i - max_i b_i| <= max_i |a_i - b_i| over the taps inside the image: the window maximum of the taps' bounds.
#     Rounding is monotone, so pack(max t^) = max pack(t^): pooled is bit for bit the xcopy element at the arg-max tap.
#   * arg-max: the kernel chose tap i because t^_i >= t^_j for the fp64 maximum j, so t_i >= t^_i - e_i >= t^_j - e_i >= t_j - e_j - e_i:
#     the chosen tap's fp64 value lies within e_i + e_j of the window maximum, e the fp32 errors before the store.  The element bound
#     lim_i holds u_T |t_i| on top of e_i, which at these types is orders of magnitude above e_j of a neighbouring tap of the same
#     channel (same scale, same shift, |x| of the same size): 2 lim_i is the window the check allows.
def pool_xf_bound(x, xf, stride, dtype):
    """-> (pooled, lim_pooled, argmax of the fp64 values, t, lim_t): t = transformed input (= xcopy's reference), fp64; bounds as above"""
    pooled, am, t = maxpool_ref(x, xf, stride)
    lim_t = stored_bound(t, xf_operand_err(x, xf, dtype), dtype)
    lim_p, _, _ = maxpool_ref(lim_t, None, stride)
    return pooled, lim_p, am, t, lim_t


def window_take(v, am, stride):
    """v [N,H,W,C] at tap am (ky*3+kx of MaxPool2d(3, stride, 1)) of every window -> ([N,OH,OW,C] values, inside: the tap names a
    pixel of the image)"""
    N, H, W, C = v.shape
    OH, OW = pool_out(H, stride), pool_out(W, stride)
    am = am.long()
    oy = torch.arange(OH).view(1, OH, 1, 1) * stride - 1 + am // 3
    ox = torch.arange(OW).view(1, 1, OW, 1) * stride - 1 + am % 3
    inside = (am >= 0) & (am < 9) & (oy >= 0) & (oy < H) & (ox >= 0) & (ox < W)
    n = torch.arange(N).view(N, 1, 1, 1).expand_as(am)
    c = torch.arange(C).view(1, 1, 1, C).expand_as(am)
    return v[n, oy.clamp(0, H - 1), ox.clamp(0, W - 1), c], inside


# Matrix-core products of f16 SUBNORMAL operands.  The accumulation bounds above charge gamma(K) on the sum of |g x|, i.e. they take
# every product to be exact and every fp32 addition to round relative to the values added.  That holds for bf16 (no operand of
# the network's range is subnormal: bf16 shares fp32's exponent range) and for normal f16 operands (11 x 11 significand bits fit
# fp32).  An f16 subnormal has no hidden bit: its significand is 0.m at the FIXED exponent 2^-14, and a multiplier that does not
# normalise its inputs delivers the product positioned at the NOMINAL exponent 2^-14 * 2^e(x), whatever the value of 0.m; the
# fp32 alignment of the dot product then keeps 24 bits below that nominal exponent, not below the product's own leading bit.
# Measured on the MI355X (v_mfma_f32_16x16x32_f16, whole ASPP_ResNet pass at 2 x 32 x 64 in f16, enc_layer5 at 1 x 2 pixels):
# g = 37 * 2^-24, x = 1177 * 2^-15 and g = 9 * 2^-24, x = 1514 * 2^-10 sum to 479581 * 2^-39, a 19-bit number; the hardware
# returned 479580 * 2^-39 -- the bit at 2^-39 lies 25 places below the nominal 2^-14 of the second product.  Every deviation seen
# is one such power of two (2^-41 .. 2^-37); products of subnormals whose bits all lie inside the window are exact
# (k * 2^-24 times 11-bit x: 786432 outputs, none off).  So for the ERROR terms an f16 operand counts with its nominal magnitude
# max(|v|, 2^-14); a zero operand still gives an exact zero product and adds nothing.  This is the hardware's arithmetic on the
# bytes the kernel hands it (ubr_wgrad.hip stages g raw), not a defect of the kernel: the derivation was wrong, and it is the
# derivation that changes.  Normal operands are unaffected (max(|v|, 2^-14) = |v|), so are bf16 and fp32.
F16_MIN_NORMAL = 2.0 ** -14


def nominal_abs(v, dtype):
    """|v| as a matrix-core error term sees it: an f16 subnormal counts as the smallest normal; zero stays zero.  v: fp64 / stored"""
    a = v.double().abs()
    if dtype != torch.float16:
        return a
    return torch.where(a > 0, a.clamp_min(F16_MIN_NORMAL), a)


def tail_fwd_bound(c2, mean2, scale2, shift2, sc, dtype, mean_b=None, scale_b=None, shift_b=None):
    """(ref, lim) of one block-tail forward launch (tail_fwd_kernel): relu(bn2) and the shortcut's BatchNorm carry two roundings
    each, their sum a third, the ReLUs none: |o^ - o| <= gamma(3) * (terms of bn2 + terms of the shortcut), then the store."""
    ref = tail_fwd_ref(c2, mean2, scale2, shift2, sc, mean_b, scale_b, shift_b)
    _, t2, _ = affine_terms(c2, mean2, scale2, shift2)
    tb = sc.double().abs() if mean_b is None else affine_terms(sc, mean_b, scale_b, shift_b)[1]
    return ref, bound(ref, t2 + tb, dtype, 3) + TINY[dtype] * (t2 + tb > 0)


def reduce_chain(npix, C, dtype):
    """upper bound of the depth of an fp32 partial of a reduce pass (see the note on the reduce passes at the top): the per-thread
    chain ceil(npix * CU / (256 * workgroups)) with the grid of pick_blocks(npix, CU, 512, 8), plus at most 6 butterfly levels"""
    CU = C // CPU[dtype]
    blocks = pick_blocks(npix, CU, 512, 8)
    return (npix * CU + 256 * blocks - 1) // (256 * blocks) + 6


def reduce_bound(gy, xhat, L, open_gate=None, extra=0):
    """per-channel (s, sx, lim_s, lim_sx) of a reduce pass on inexact operands: fp32 partials L deep (reduce_chain), g_y*xhat with
    the two roundings of xhat = fl(fl(c - mean) * invstd) and its own product (+3), `extra` roundings that g_y itself carries (a
    second gradient operand added in fp32: 1), then fp64 (2^-50).  Where the gate of an element is open (gate_open) the kernel may
    have taken the other branch: the whole term is added to the bound."""
    C = gy.shape[-1]
    g, x = gy.reshape(-1, C), xhat.reshape(-1, C)
    t = g * x
    l1 = (gamma(L + extra) + 2.0 ** -50) * g.abs().sum(0)
    l2 = (gamma(L + 3 + extra) + 2.0 ** -50) * t.abs().sum(0)
    if open_gate is not None:
        o = open_gate.reshape(-1, C).double()
        l1, l2 = l1 + (o * g.abs()).sum(0), l2 + (o * t.abs()).sum(0)
    return g.sum(0), t.sum(0), l1, l2


def apply_bound(gy, xhat, scale, k1, k2, dtype, extra=0):
    """(ref, lim) of an apply pass g_c = scale * (g_y - k1 - xhat*k2): xhat two roundings, its product with k2, two differences,
    the product with scale: at most 6 on any term (+ `extra` of g_y, + 1 where k1 / k2 are formed in the kernel from the stripes:
    the caller passes it in `extra`), on the terms |scale| (|g_y| + |k1| + |xhat k2|); then the store."""
    ref = apply_ref(gy, xhat, scale, k1, k2)
    terms = _vec(scale, gy).abs() * (gy.abs() + _vec(k1, gy).abs() + (xhat * _vec(k2, gy)).abs())
    return ref, bound(ref, terms, dtype, 6 + extra) + TINY[dtype] * (terms > 0)


def stored_bound(ref, pre, dtype):
    """bound after the store of an fp32 value v^ with |v^ - ref| <= pre: the store rounds once, |round(v^) - v^| <= u_out |v^| <=
    u_out (|ref| + pre), or misses by TINY in the subnormal range: u_out (|ref| + pre) + pre + TINY (zero where ref and pre are)"""
    return C_OUT * UNIT_ROUNDOFF[dtype] * (ref.abs() + pre) + pre + TINY[dtype] * ((ref.abs() + pre) > 0)


def conv_stats_bound(ref, pre, N, OH, OW):
    """forward statistics (sum v^, sum v^^2 over the output grid) of an fp32 conv value with |v^ - ref| <= pre, per channel:
    -> (fp64 [2C] reference sums of ref, bound).  The chain bound stats_eps(stats_chain) applies to the sums of the values the
    kernel actually has; those differ from ref's by at most sum pre, and sum |v^^2 - v^2| <= sum (2 |v| pre + pre^2):
        |s1 - sum v|   <= e1 sum |v|  + (1 + e1) sum pre
        |s2 - sum v^2| <= e2 sum v^2  + (1 + e2) sum (2 |v| pre + pre^2)"""
    C = ref.shape[-1]
    s1, s2, a1, a2 = conv_stats_ref(ref)
    e1, e2 = stats_eps(stats_chain(N, OH, OW))
    p, v = pre.reshape(-1, C), ref.reshape(-1, C).abs()
    return torch.cat([s1, s2]), torch.cat([e1 * a1 + (1 + e1) * p.sum(0), e2 * a2 + (1 + e2) * (2 * v * p + p * p).sum(0)])


def bn_eval_affine_bound(gamma_, rvar, eps):
    """ubr_bn_eval_affine in fp32 against bn_eval_affine_ref (fp64): invstd = 1 / sqrtf(fl(rvar + eps)) is three roundings, scale =
    gamma * invstd a fourth (the counts tests/test_gpu_param_exact.py uses): -> ((invstd, lim), (scale, lim)), lim = gamma(k) |ref|"""
    inv, sc = bn_eval_affine_ref(gamma_, rvar, eps)
    return (inv, gamma(3) * inv.abs()), (sc, gamma(4) * sc.abs())
