"""CPU: the float64 kernel references of tests/kref.py restate the PyTorch ops they stand for, and their checks have
teeth -- each injected fault of the kind a tiled kernel makes (a tap dropped at a border pixel, a channel slice of one
tile scaled, a tile missing from a statistics sum, a tile counted twice in a weight gradient) fails the check."""
import pytest
import torch
import torch.nn.functional as F

import kref
from ubresnet_amd import ops

D = torch.float64


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def operands(N, C, H, W, seed, **kw):
    return kref.exact_operands((N, H, W, C), torch.float64, seed=seed, **kw)


@pytest.mark.parametrize("k,dil", [(1, 1), (3, 1), (3, 3), (3, 5), (7, 1), (7, 3)])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_ref_equals_conv2d(k, stride, dil):
    N, Cin, Cout, H, W = 2, 8, 12, 19, 23
    pad = dil * (k // 2)
    x = operands(N, Cin, H, W, 1, zero_tiles=0.3, tile=8)
    w = kref.exact_operands((Cout, Cin, k, k), D, seed=2, density=0.5)
    b = kref.exact_operands((Cout,), D, seed=3, density=1.0)
    xf = kref.exact_affine(Cin, 4)
    ref = F.conv2d(nchw(kref._xform(x, xf)), w, b, stride, pad, dil)
    OH, OW = ref.shape[2], ref.shape[3]
    ad = operands(N, Cout, OH, OW, 5)
    got, ab = kref.conv_ref(x, kref.pack_dense(w, range(k * k)), ops.conv_taps(k, dil, pad), Cout, OH, OW, S=stride,
                            xf=xf, bias=b, addend=ad, act=2)
    assert torch.equal(got, nhwc(ref + nchw(ad)).clamp_min(0))
    # the abs twin bounds the value and is the same op on |operands|
    assert bool((ab >= got.abs()).all())
    ref_abs = F.conv2d(nchw(kref._xform(x, xf)).abs(), w.abs(), b.abs(), stride, pad, dil) + nchw(ad).abs()
    assert torch.equal(ab, nhwc(ref_abs))


@pytest.mark.parametrize("k,dil", [(1, 1), (3, 1), (3, 3), (7, 1)])
def test_conv_ref_dgrad_taps_equal_autograd(k, dil):
    N, Cin, Cout, H, W = 2, 8, 16, 17, 21
    pad = dil * (k // 2)
    x = operands(N, Cin, H, W, 11).requires_grad_(True)
    w = kref.exact_operands((Cout, Cin, k, k), D, seed=12, density=0.6)
    y = F.conv2d(nchw(x), w, None, 1, pad, dil)
    g = operands(N, Cout, H, W, 13)
    y.backward(nchw(g))
    got, _ = kref.conv_ref(g, kref.pack_dense(w, range(k * k), fwd=False), ops.conv_dgrad_taps_s1(k, dil, pad), Cin, H, W)
    assert torch.equal(got, x.grad)


def test_conv_ref_transposed_phases_equal_conv_transpose2d():
    N, Cin, Cd, H, W = 2, 16, 8, 7, 9
    x = operands(N, Cin, H, W, 21)
    w = kref.exact_operands((Cin, Cd, 4, 4), D, seed=22, density=0.6)
    b = kref.exact_operands((Cd,), D, seed=23, density=1.0)
    ref = nhwc(F.conv_transpose2d(nchw(x), w, b, 2, 1))
    Wd = kref.pack_dense(w, range(16), fwd=False)
    phases = [(ry, rx, ops.transposed_phase_taps(4, 1, 1, 2, ry, rx)) for ry in range(2) for rx in range(2)]
    assert all(len(p[2]) == 4 for p in phases)
    for ry, rx, tp in phases:
        got, _ = kref.conv_ref(x, Wd, tp, Cd, H, W, bias=b)
        assert torch.equal(got, ref[:, ry::2, rx::2, :]), (ry, rx)
    got, _ = kref.conv_phases_ref(x, Wd, phases, Cd, H, W, bias=b)
    assert torch.equal(got, ref)
    # the data gradient of a stride-2 3x3 conv, phase by phase (phase (1,1) of a 1x1 conv has no taps)
    w3 = kref.exact_operands((Cin, Cd, 3, 3), D, seed=24, density=0.6)
    xr = operands(N, Cd, 2 * H, 2 * W, 25).requires_grad_(True)
    y = F.conv2d(nchw(xr), w3, None, 2, 1)
    g = nhwc(y.detach()) * 0 + operands(N, Cin, y.shape[2], y.shape[3], 26)
    y.backward(nchw(g))
    ph3 = [(ry, rx, ops.transposed_phase_taps(3, 1, 1, 2, ry, rx)) for ry in range(2) for rx in range(2)]
    got, _ = kref.conv_phases_ref(g, kref.pack_dense(w3, range(9), fwd=False), ph3, Cd, H, W)
    assert torch.equal(got, xr.grad)


@pytest.mark.parametrize("k,stride,dil", [(1, 1, 1), (1, 2, 1), (3, 1, 1), (3, 2, 1), (3, 1, 3), (3, 1, 5), (7, 1, 1), (4, 2, 1)])
def test_wgrad_ref_equals_conv2d_weight(k, stride, dil):
    N, Cin, Cout, H, W = 2, 8, 16, 18, 22
    pad = dil * (k // 2) if k != 4 else 1
    x = operands(N, Cin, H, W, 31)
    xf = kref.exact_affine(Cin, 32, relu=True)
    xt = nchw(kref._xform(x, xf))
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    g = operands(N, Cout, OH, OW, 33)
    ref = torch.nn.grad.conv2d_weight(xt, (Cout, Cin, k, k), nchw(g), stride, pad, dil)
    taps = ops.conv_taps(k, dil, pad)
    dW, ab = kref.wgrad_ref(x, g, taps, S=stride, xf=xf)
    for t, (_, _, wi) in enumerate(taps):
        assert torch.equal(dW[t], ref[:, :, wi // k, wi % k]), t
    assert bool((ab >= dW.abs()).all())
    # scatter into the PyTorch layout (and a tap subset into a larger window, accumulating)
    flat, touched = kref.wgrad_scatter(dW, Cout * Cin * k * k, taps, Cin * k * k, k * k, Cout, Cin)
    assert bool(touched.all()) and torch.equal(flat.view(Cout, Cin, k, k), ref)
    flat2, touched2 = kref.wgrad_scatter(dW[::2], Cout * Cin * k * k + 5, taps[::2], Cin * k * k, k * k, Cout - 3, Cin, dst_offset=5,
                                         init=torch.ones(Cout * Cin * k * k + 5, dtype=D))
    assert int(touched2.sum()) == (Cout - 3) * Cin * len(taps[::2])
    assert float(flat2[~touched2].sub(1).abs().max()) == 0.0


def _exact_case(dt=torch.bfloat16, N=2, H=64, W=64, Cin=16, Cout=32, seed=41):
    x = kref.exact_operands((N, H, W, Cin), dt, seed=seed, density=0.3, zero_tiles=0.25)
    w = kref.exact_operands((9, Cin, Cout), dt, seed=seed + 1, density=0.5, exp=-1)
    ref, ab = kref.conv_ref(x, w.double(), ops.conv_taps(3, 1, 1), Cout, H, W)
    return x, w, ref, ab


def test_exact_check_passes_the_reference_and_asserts_its_budget():
    x, w, ref, ab = _exact_case()
    got = kref.round_to(ref, torch.bfloat16)
    kref.assert_exact(got, ref, torch.bfloat16, ab, 2.0 ** -1, "reference itself")
    with pytest.raises(AssertionError, match="budget"):
        kref.assert_exact(got, ref, torch.bfloat16, ab * 2.0 ** 24, 2.0 ** -1, "over budget")


def test_fault_tap_dropped_at_one_border_pixel_is_caught():
    x, w, ref, ab = _exact_case()
    taps = ops.conv_taps(3, 1, 1)
    # pick a border pixel and a tap whose contribution there is not zero
    n, oy = 1, 0
    for ox in range(ref.shape[2]):
        for t, (dy, dx, wi) in enumerate(taps):
            iy, ix = oy + dy, ox + dx
            if 0 <= iy < x.shape[1] and 0 <= ix < x.shape[2]:
                c = x[n, iy, ix].double() @ w[wi].double()
                if bool((c != 0).any()):
                    break
        else:
            continue
        break
    bad = ref.clone()
    bad[n, oy, ox] -= c
    with pytest.raises(AssertionError, match="differ"):
        kref.assert_exact(kref.round_to(bad, torch.bfloat16), ref, torch.bfloat16, ab, 2.0 ** -1, "dropped tap")
    # the bounded tier catches it too
    with pytest.raises(AssertionError, match="outside the bound"):
        kref.assert_bounded(kref.round_to(bad, torch.bfloat16), ref, ab, torch.bfloat16, 9 * 16, "dropped tap")


def test_fault_channel_slice_of_one_tile_scaled_is_caught():
    x, w, ref, ab = _exact_case()
    got = kref.round_to(ref, torch.bfloat16)
    tile = (0, 8, slice(32, 64), slice(16, 32))          # one 32-pixel tile row, one 16-channel slice
    assert bool((got[tile] != 0).any())
    bad = got.clone()
    bad[tile] = (got[tile].double() * (1 + 2.0 ** -7)).to(torch.bfloat16)
    assert not torch.equal(bad, got)
    with pytest.raises(AssertionError, match="differ"):
        kref.assert_exact(bad, ref, torch.bfloat16, ab, 2.0 ** -1, "scaled slice")


@pytest.mark.parametrize("exact", [True, False])
def test_fault_tile_missing_from_stats_is_caught(exact):
    N, H, W, C = 2, 64, 64, 16
    v = kref.exact_operands((N, H, W, C), D, seed=51, density=0.4, zero_tiles=0.2, maxmag=2 if exact else 2048)
    refs = kref.conv_stats_ref(v)
    s = torch.cat([refs[0], refs[1]])
    L = kref.stats_chain(N, H, W)
    unit = 1.0
    assert kref.assert_stats(s, refs, L, unit) == ("exact" if exact else "bounded")
    tile = v[1, 16, 32:64]                                 # one 32-pixel tile row
    assert bool((tile != 0).any())
    bad = s.clone()
    bad[:C] -= tile.sum(0)
    bad[C:] -= (tile * tile).sum(0)
    with pytest.raises(AssertionError, match="stats"):
        kref.assert_stats(bad, refs, L, unit)
    # the BatchNorm-backward form: same check on its own sums
    c = kref.exact_operands((N, H, W, C), D, seed=52, density=0.8, zero_tiles=0)
    bnb = (c, torch.zeros(C, dtype=D), torch.ones(C, dtype=D), torch.zeros(C, dtype=D), torch.full((C,), 0.5, dtype=D))
    rb = kref.conv_stats_ref(v, bnb, torch.float32)
    sb = torch.cat([rb[0], rb[1]])
    kref.assert_stats(sb, rb, L, unit, unit * 0.5)
    gy = torch.where(c[1, 16, 32:64] > 0, tile, torch.zeros((), dtype=D))
    assert bool((gy != 0).any())
    bad = sb.clone()
    bad[:C] -= gy.sum(0)
    with pytest.raises(AssertionError, match="stats"):
        kref.assert_stats(bad, rb, L, unit, unit * 0.5)


def test_fault_wgrad_tile_counted_twice_is_caught():
    N, H, W, Cin, Cout = 2, 48, 64, 16, 32
    x = kref.exact_operands((N, H, W, Cin), torch.bfloat16, seed=61, density=0.3)
    g = kref.exact_operands((N, H, W, Cout), torch.bfloat16, seed=62, density=0.3, zero_tiles=0.1)
    taps = ops.conv_taps(3, 1, 1)
    dW, ab = kref.wgrad_ref(x, g, taps)
    one = torch.zeros_like(g)
    one[0, 16:24, 32:64] = g[0, 16:24, 32:64]               # one 8 x 32 tile of the pixel walk
    extra, _ = kref.wgrad_ref(x, one, taps)
    assert bool((extra != 0).any())
    got = (dW + extra).float()
    kref.assert_exact(dW.float(), dW, torch.float32, ab, 1.0, "reference itself")
    with pytest.raises(AssertionError, match="differ"):
        kref.assert_exact(got, dW, torch.float32, ab, 1.0, "tile twice")


# ------------------------------------------------------------------------------------------------------------------
# streaming-kernel references (block tail, BatchNorm backward, max-pool, head) against float64 PyTorch
# ------------------------------------------------------------------------------------------------------------------
def _site(C, seed):
    """(mean, var, gamma, beta, eps) of a BatchNorm site with exact invstd: eps 0.25, var in {0, 0.75, 3.75}"""
    g = torch.Generator().manual_seed(seed)
    pick = lambda vals: torch.tensor(vals, dtype=D)[torch.randint(0, len(vals), (C,), generator=g)]
    return pick([-1., 0., 1.]), pick([0., 0.75, 3.75]), pick([0.5, 1., 2.]), pick([-1., 0., 1.]), 0.25


def _vectors(site):
    mean, var, gamma, beta, eps = site
    inv = 1.0 / torch.sqrt(var + eps)
    return mean, gamma * inv, beta, inv


def _bn_eval(x_nchw, site):
    mean, var, gamma, beta, eps = site
    return F.batch_norm(x_nchw, mean, var, gamma, beta, False, 0.0, eps)


@pytest.mark.parametrize("byp", [False, True])
def test_tail_refs_equal_autograd(byp):
    """forward, the two reduce sums and the apply formula of a block tail against autograd through TRAIN-mode batch_norm:
    with k1 = sum(g_y)/n and k2 = sum(g_y*xhat)/n, scale*(g_y - k1 - xhat*k2) is batch_norm's input gradient"""
    N, H, W, C = 2, 9, 11, 8
    n = N * H * W
    c2 = operands(N, C, H, W, 71, density=0.7, zero_tiles=0).requires_grad_(True)
    sc = operands(N, C, H, W, 72, density=0.7, zero_tiles=0, exp=-1).requires_grad_(True)
    go, go2 = operands(N, C, H, W, 73, density=0.6, zero_tiles=0, exp=-1), operands(N, C, H, W, 74, density=0.6, zero_tiles=0, exp=-1)
    g2, b2 = _site(C, 75)[2:4]
    gb, bb = _site(C, 76)[2:4]
    eps = 1e-5
    bn2 = F.batch_norm(nchw(c2), None, None, g2, b2, True, 0.0, eps)
    sh = F.batch_norm(nchw(sc), None, None, gb, bb, True, 0.0, eps) if byp else nchw(sc)
    out = F.relu(F.relu(bn2) + sh)
    out.backward(nchw(go + go2))

    def vec(x, gamma, beta):
        f = x.detach().reshape(-1, C)
        mean, var = f.mean(0), f.var(0, unbiased=False)
        inv = 1.0 / torch.sqrt(var + eps)
        return mean, gamma * inv, beta, inv
    m2, s2, t2, i2 = vec(c2, g2, b2)
    mb, sb, tb, ib = vec(sc, gb, bb) if byp else (None,) * 4
    ref = kref.tail_fwd_ref(c2.detach(), m2, s2, t2, sc.detach(), mb, sb, tb)
    assert torch.allclose(ref, nhwc(out.detach()), rtol=0, atol=1e-12)
    positive = ref > 0
    gz, gy2, xh2, xhb = kref.tail_bwd_ref(go, go2, positive, c2.detach(), s2, t2, m2, i2, sc.detach() if byp else None, mb, ib)
    s, sx, a1, a2 = kref.reduce_ref(gy2, xh2)
    assert torch.equal(s, gy2.reshape(-1, C).sum(0)) and bool((a1 >= s.abs()).all()) and bool((a2 >= sx.abs()).all())
    g_c2 = kref.apply_ref(gy2, xh2, s2, s / n, sx / n)
    assert torch.allclose(g_c2, c2.grad, rtol=0, atol=1e-10)
    if byp:
        sb_, sxb, _, _ = kref.reduce_ref(gz, xhb)
        assert torch.allclose(kref.apply_ref(gz, xhb, sb, sb_ / n, sxb / n), sc.grad, rtol=0, atol=1e-10)
    else:
        assert torch.equal(gz, sc.grad)
    # the mask bits are [stored output > 0], and unpack inverts pack
    bits = kref.mask_pack(positive, 8)
    assert bits.numel() == n * C // 8 and torch.equal(kref.mask_unpack(bits, positive.shape, 8), positive)


@pytest.mark.parametrize("relu", [False, True])
def test_bn_bwd_ref_equals_autograd(relu):
    N, H, W, C = 2, 7, 13, 8
    n = N * H * W
    c = operands(N, C, H, W, 81, density=0.8, zero_tiles=0).requires_grad_(True)
    ga, ga2 = operands(N, C, H, W, 82, density=0.6, zero_tiles=0, exp=-1), operands(N, C, H, W, 83, density=0.6, zero_tiles=0, exp=-1)
    gamma, beta = _site(C, 84)[2:4]
    y = F.batch_norm(nchw(c), None, None, gamma, beta, True, 0.0, 1e-5)
    (F.relu(y) if relu else y).backward(nchw(ga + ga2))
    f = c.detach().reshape(-1, C)
    inv = 1.0 / torch.sqrt(f.var(0, unbiased=False) + 1e-5)
    gy, xh = kref.bn_bwd_ref(ga, ga2, c.detach(), gamma * inv, beta, f.mean(0), inv, relu)
    s, sx, _, _ = kref.reduce_ref(gy, xh)
    assert torch.allclose(kref.apply_ref(gy, xh, gamma * inv, s / n, sx / n), c.grad, rtol=0, atol=1e-10)


def test_bn_finalize_ref_equals_batch_norm_training_statistics():
    N, H, W, C = 3, 8, 8, 6
    x = operands(N, C, H, W, 85, density=0.9, zero_tiles=0)
    f = x.reshape(-1, C)
    n = float(f.shape[0])
    gamma, beta = _site(C, 86)[2:4]
    rm, rv = torch.zeros(C, dtype=D), torch.ones(C, dtype=D)
    F.batch_norm(nchw(x), rm, rv, gamma, beta, True, 0.125, 0.25)
    scale, shift, mean, inv, rmean, rvar = kref.bn_finalize_ref(f.sum(0), (f * f).sum(0), n, gamma, beta, 0.25, torch.zeros(C), torch.ones(C), 0.125)
    assert torch.allclose(mean.double(), f.mean(0), atol=1e-6) and torch.allclose(rmean.double(), rm, atol=1e-6)
    assert torch.allclose(rvar.double(), rv, atol=1e-6) and torch.equal(shift.double(), beta)
    assert torch.allclose(scale.double(), gamma / torch.sqrt(f.var(0, unbiased=False) + 0.25), atol=1e-6)
    assert torch.allclose(inv.double() * gamma, scale.double(), atol=1e-6)


@pytest.mark.parametrize("stride,H,W", [(1, 12, 17), (2, 16, 24), (2, 33, 47)])
def test_maxpool_ref_equals_aten_on_ties(stride, H, W):
    """ATen's CPU max_pool2d keeps the first maximum in scan order: the tie rule, pinned independently of this project"""
    N, C = 2, 8
    x = operands(N, C, H, W, 91, density=0.3, zero_tiles=0.3, tile=4)       # small integers, mostly zero: ties everywhere
    xf = kref.exact_affine(C, 92, relu=True)
    v = nchw(kref._xform(x, xf)).contiguous().requires_grad_(True)
    p, idx = F.max_pool2d(v, 3, stride, 1, return_indices=True)
    pooled, am, vt = kref.maxpool_ref(x, xf, stride)
    assert torch.equal(pooled, nhwc(p.detach())) and torch.equal(vt, nhwc(v.detach()))
    OH, OW = p.shape[2], p.shape[3]
    oy = torch.arange(OH).view(1, -1, 1, 1)
    ox = torch.arange(OW).view(1, 1, -1, 1)
    flat = (oy * stride - 1 + am // 3) * W + (ox * stride - 1 + am % 3)       # the arg-max tap as ATen's flat input index
    assert torch.equal(flat, nhwc(idx))
    ties = 0
    for t in range(9):          # the case has teeth: many windows hold their maximum more than once
        ky, kx = t // 3, t % 3
        vp = F.pad(vt, (0, 0, 1, 1, 1, 1), value=float("-inf"))
        ties = ties + (vp[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride, :] == pooled).long()
    assert float((ties > 1).float().mean()) > 0.3
    gp, ge = operands(N, C, OH, OW, 93, density=0.7, zero_tiles=0, exp=-1), operands(N, C, H, W, 94, density=0.5, zero_tiles=0, exp=-1)
    p.backward(nchw(gp))
    assert torch.equal(kref.maxpool_bwd_ref(gp, am, (H, W), stride, ge), nhwc(v.grad) + ge)
    assert torch.equal(kref.maxpool_bwd_ref(gp, am, (H, W), stride), nhwc(v.grad))


def test_head_refs_equal_pytorch_and_the_oracle():
    from oracle import uresnet_oracle as O
    N, C, H, W = 2, 3, 9, 14
    z = torch.randn((N, C, H, W), dtype=D, generator=torch.Generator().manual_seed(95)).requires_grad_(True)
    lp = F.log_softmax(z, 1)
    g = kref.exact_operands((N, C, H, W), D, seed=96, density=0.5, zero_tiles=0, exp=-2)
    lp.backward(g)
    ref, lim = kref.logsoftmax_bwd_ref(g, lp.detach().exp(), torch.bfloat16)
    assert torch.allclose(ref, nhwc(z.grad), rtol=0, atol=1e-14) and bool((lim >= 0).all())
    # the loss pair against the oracle's PixelWiseNLLLoss and its autograd, with class weights and ignored pixels
    pred = lp.detach().clone().requires_grad_(True)
    gen = torch.Generator().manual_seed(97)
    tgt = torch.randint(0, C, (N, H, W), generator=gen)
    tgt[torch.rand((N, H, W), generator=gen) < 0.2] = -100
    pw = torch.tensor([0., 0.5, 1., 2.], dtype=D)[torch.randint(0, 4, (N, H, W), generator=gen)]
    cw = torch.tensor([0.5, 1., 2.], dtype=D)
    loss = O.pixelwise_nll(pred, tgt, pw, cw)
    loss.backward()
    s, ab, bad, ok, w = kref.nll_ref(pred.detach(), tgt, pw, cw, -100)
    assert bad == 0 and abs(float(s) / tgt.numel() - float(loss.detach())) <= 1e-14 and float(ab) >= abs(float(s))
    gref = kref.nll_bwd_ref(1.0, tgt, pw, cw, -100, C)
    assert torch.allclose(gref, pred.grad, rtol=1e-6, atol=0)           # gl is rounded to fp32 once, as the kernel forms it
    tb = tgt.clone()
    tb[0, 0, :3] = C + 1
    assert kref.nll_ref(pred.detach(), tb, pw, cw, -100)[2] == 3
    # confusion: first arg-max over channels, as Tensor.max(1)
    lq = kref.exact_operands((N, C, H, W), D, seed=98, density=0.5, zero_tiles=0)
    t2 = tgt.clamp_min(-1)
    cm = kref.confusion_ref(lq, t2)
    pred_c = lq.max(1)[1]
    want = torch.zeros(C * C, dtype=torch.int64)
    for t, q in zip(t2.reshape(-1).tolist(), pred_c.reshape(-1).tolist()):
        if 0 <= t < C:
            want[t * C + q] += 1
    assert torch.equal(cm, want)
    # stem expansion
    x = kref.exact_operands((2, 2, 5, 9), D, seed=99, density=0.8, zero_tiles=0)
    e = kref.stem_expand_ref(x)
    assert e.shape == (2, 5, 9, 32) and float(e[..., 7:16].abs().max()) == 0.0 and torch.equal(e[..., 16 + 3], x[:, 1])
    assert torch.equal(e[:, :, 2:, 16 + 1], x[:, 1, :, :-2]) and float(e[:, :, :2, 16 + 1].abs().max()) == 0.0


def _tail_case(npix_shape=(2, 40, 37, 16), dt=torch.bfloat16):
    N, H, W, C = npix_shape
    c2 = kref.exact_operands(npix_shape, dt, seed=101, density=0.6, zero_tiles=0.2)
    sc = kref.exact_operands(npix_shape, dt, seed=102, density=0.4, zero_tiles=0.2, exp=-1)
    m2, s2, t2, _ = _vectors(_site(C, 103))
    ref = kref.tail_fwd_ref(c2, m2, s2, t2, sc)
    return ref, kref.round_to(ref, dt)


def test_fault_last_trip_pixel_left_unwritten_is_caught():
    ref, got = _tail_case()
    kref.assert_exact(got, ref, torch.bfloat16, ref.abs(), 0.125, "reference itself")
    flat = got.reshape(-1, 16).clone()
    p = (ref.reshape(-1, 16)[-64:] != 0).any(1).nonzero()[-1] + flat.shape[0] - 64     # a pixel of the last trip with a nonzero output
    flat[p] = float("nan")                                                              # what the sentinel-filled buffer still holds
    with pytest.raises(AssertionError, match="differ"):
        kref.assert_exact(flat.view(ref.shape), ref, torch.bfloat16, ref.abs(), 0.125, "unwritten pixel")
    flat[p] = 0.0                                                                       # ... or a zero-initialised one
    with pytest.raises(AssertionError, match="differ"):
        kref.assert_exact(flat.view(ref.shape), ref, torch.bfloat16, ref.abs(), 0.125, "unwritten pixel")


def test_fault_one_mask_bit_flipped_is_caught():
    ref, got = _tail_case()
    want = kref.mask_pack(got > 0, 8)
    assert torch.equal(kref.mask_pack(kref.round_to(ref, torch.bfloat16) > 0, 8), want)
    bad = want.clone()
    bad[bad.numel() // 2] ^= 1 << 5
    assert not torch.equal(bad, want)
    # and a flipped bit moves the backward's sums: the gate it feeds is part of the reduce reference
    go = kref.exact_operands(ref.shape, D, seed=104, density=1.0, zero_tiles=0, exp=-1)
    z = torch.zeros(16, dtype=D)
    one = torch.ones(16, dtype=D)
    sums = lambda m: kref.reduce_ref(kref.tail_bwd_ref(go, None, kref.mask_unpack(m, ref.shape, 8), ref + 1, one, one, z, one)[0])
    (s, _, a, _), (sb, _, _, _) = sums(want), sums(bad)
    kref.assert_sums_exact(s, s, a, 0.5, "reference itself")
    with pytest.raises(AssertionError, match="channel"):
        kref.assert_sums_exact(sb, s, a, 0.5, "flipped bit")


def test_fault_tie_resolved_to_the_second_maximum_is_caught():
    x = operands(2, 8, 16, 16, 111, density=0.3, zero_tiles=0.3, tile=4)
    pooled, am, v = kref.maxpool_ref(x, None, 2)
    # a window whose maximum occurs twice: move its arg-max to the second occurrence
    vp = F.pad(v, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    for t in range(8, 0, -1):
        ky, kx = t // 3, t % 3
        hit = (vp[:, ky:ky + 15:2, kx:kx + 15:2, :] == pooled) & (am < t)
        if bool(hit.any()):
            break
    i = tuple(hit.nonzero()[0].tolist())
    bad = am.clone()
    bad[i] = t
    assert not torch.equal(bad, am)                                        # the arg-max check itself
    gp = kref.exact_operands(tuple(pooled.shape), D, seed=112, density=1.0, zero_tiles=0, exp=-1)
    ref = kref.maxpool_bwd_ref(gp, am, (16, 16), 2)
    got = kref.round_to(kref.maxpool_bwd_ref(gp, bad, (16, 16), 2), torch.bfloat16)
    kref.assert_exact(kref.round_to(ref, torch.bfloat16), ref, torch.bfloat16, ref.abs(), 0.5, "reference itself")
    with pytest.raises(AssertionError, match="differ"):
        kref.assert_exact(got, ref, torch.bfloat16, ref.abs(), 0.5, "second maximum")


def test_fault_stripe_left_out_of_a_sum_is_caught():
    N, H, W, C = 2, 32, 32, 16
    g = operands(N, C, H, W, 121, density=0.5, zero_tiles=0.2, exp=-1)
    s, _, a, _ = kref.reduce_ref(g)
    f = g.reshape(-1, C)
    stripes = torch.stack([f[i::kref.RED_SLOTS].sum(0) for i in range(kref.RED_SLOTS)])       # workgroup i adds into stripe i % 8
    kref.assert_sums_exact(stripes.sum(0), s, a, 0.5, "reference itself")
    assert bool((stripes[3] != 0).any())
    with pytest.raises(AssertionError, match="channel"):
        kref.assert_sums_exact(stripes.sum(0) - stripes[3], s, a, 0.5, "stripe 3 missing")
    with pytest.raises(AssertionError, match="budget"):
        kref.assert_sums_exact(s, s, a * 2.0 ** 24, 0.5, "over budget")


def test_fault_element_written_past_C_in_a_sliced_view_is_caught():
    N, H, W, C, PS = 1, 6, 7, 16, 80
    v = kref.TV.make((N, H, W, C), (H * W * PS, W * PS, PS, 1), torch.bfloat16, 1 << 40, (1 << 40) + 64 * 2)      # channels 64..79 of 80
    B = kref.Buffers([v], device="cpu")
    snap = B.snapshot()
    B.mark_written(v)
    B.view(v).fill_(1.0)
    B.check_sentinel(snap, "the view itself")
    g = B.groups[v.gid]
    first = g["m"]                                        # element 0 of pixel 0 of the slice
    g["buf"][first + C] = 1.0                             # channel 16 of pixel 0 = channel 0 of the NEXT 80-channel pixel: outside
    with pytest.raises(AssertionError, match="outside its output view"):
        B.check_sentinel(snap, "one element past C")
    g["buf"][first + C] = float("nan")
    B.check_sentinel(snap, "restored")
    g["buf"][first - 1] = 0.0                             # channel 63 of pixel 0: just in front of the slice
    with pytest.raises(AssertionError, match="outside its output view"):
        B.check_sentinel(snap, "one element in front")
