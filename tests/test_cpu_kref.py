"""CPU: the float64 kernel references of tests/kref.py restate the PyTorch ops they stand for, and their checks have
teeth -- each injected fault of the kind a tiled kernel makes (a tap dropped at a border pixel, a channel slice of one
tile scaled, a tile missing from a statistics sum, a tile counted twice in a weight gradient) fails the check."""
import math

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


def _frozen_site(C, seed):
    """a frozen site as the module holds it: running statistics (not the batch's), gamma / beta as autograd leaves"""
    mean, var, gamma, beta, eps = _site(C, seed)
    return mean, var, gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True), eps


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_bn_bwd_frozen_ref_equals_autograd_through_eval_mode_batch_norm(relu, two):
    """g_c = scale*g_y, dbeta = sum g_y, dgamma = sum g_y*xhat against autograd through F.batch_norm(training=False) (+ relu)"""
    N, H, W, C = 2, 7, 13, 8
    c = operands(N, C, H, W, 86, density=0.8, zero_tiles=0).requires_grad_(True)
    ga = operands(N, C, H, W, 87, density=0.6, zero_tiles=0, exp=-1)
    ga2 = operands(N, C, H, W, 88, density=0.6, zero_tiles=0, exp=-1) if two else None
    mean, var, gamma, beta, eps = _frozen_site(C, 89)
    f = c.detach().reshape(-1, C)
    assert not torch.allclose(f.mean(0), mean) and not torch.allclose(f.var(0, unbiased=False), var)      # not the batch's statistics
    y = F.batch_norm(nchw(c), mean, var, gamma, beta, False, 0.0, eps)
    (F.relu(y) if relu else y).backward(nchw(ga + ga2 if two else ga))
    inv = 1.0 / torch.sqrt(var + eps)
    gc, (db, a1), (dg, a2) = kref.bn_bwd_frozen_ref(ga, ga2, c.detach(), gamma.detach() * inv, beta.detach(), mean, inv, relu)
    assert torch.allclose(gc, c.grad, rtol=0, atol=1e-12)
    assert torch.allclose(db, beta.grad, rtol=0, atol=1e-10) and torch.allclose(dg, gamma.grad, rtol=0, atol=1e-10)
    assert bool((a1 >= db.abs()).all()) and bool((a2 >= dg.abs()).all())
    assert bool((dg != db).any()) and bool((gc != 0).any())


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("byp", [False, True])
def test_tail_bwd_frozen_ref_equals_autograd_through_eval_mode_batch_norm(byp, two):
    """relu(relu(bn2(c2)) + shortcut), shortcut = bnpass(cb) or x, both sites frozen; the gate is the forward output's sign,
    handed over as the mask bits the forward kernel would have stored"""
    N, H, W, C = 2, 9, 11, 8
    c2 = operands(N, C, H, W, 91, density=0.7, zero_tiles=0).requires_grad_(True)
    sc = operands(N, C, H, W, 92, density=0.7, zero_tiles=0, exp=-1).requires_grad_(True)
    go = operands(N, C, H, W, 93, density=0.6, zero_tiles=0, exp=-1)
    go2 = operands(N, C, H, W, 94, density=0.6, zero_tiles=0, exp=-1) if two else None
    mean2, var2, g2, b2, eps = _frozen_site(C, 95)
    meanb, varb, gb, bb, _ = _frozen_site(C, 96)
    bn2 = F.batch_norm(nchw(c2), mean2, var2, g2, b2, False, 0.0, eps)
    sh = F.batch_norm(nchw(sc), meanb, varb, gb, bb, False, 0.0, eps) if byp else nchw(sc)
    out = F.relu(F.relu(bn2) + sh)
    out.backward(nchw(go + go2 if two else go))
    i2, ib = 1.0 / torch.sqrt(var2 + eps), 1.0 / torch.sqrt(varb + eps)
    s2, sb = g2.detach() * i2, gb.detach() * ib
    positive = nhwc(out.detach()) > 0
    bits = kref.mask_pack(positive, 8)
    g_c2, g_sc, sums2, sumsb = kref.tail_bwd_frozen_ref(go, go2, kref.mask_unpack(bits, positive.shape, 8), c2.detach(), s2, b2.detach(),
                                                        mean2, i2, sc.detach() if byp else None, sb if byp else None,
                                                        meanb if byp else None, ib if byp else None)
    assert torch.allclose(g_c2, c2.grad, rtol=0, atol=1e-12) and torch.allclose(g_sc, sc.grad, rtol=0, atol=1e-12)
    (db2, a1), (dg2, a2) = sums2
    assert torch.allclose(db2, b2.grad, rtol=0, atol=1e-10) and torch.allclose(dg2, g2.grad, rtol=0, atol=1e-10)
    assert bool((a1 >= db2.abs()).all()) and bool((a2 >= dg2.abs()).all())
    if byp:
        (dbb, _), (dgb, _) = sumsb
        assert torch.allclose(dbb, bb.grad, rtol=0, atol=1e-10) and torch.allclose(dgb, gb.grad, rtol=0, atol=1e-10)
        assert bool((g_sc != go + go2 if two else g_sc != go).any())          # scale_b is in it
    else:
        assert sumsb is None and gb.grad is None


def test_fault_frozen_dgamma_from_the_centred_input_or_an_unscaled_shortcut_is_caught():
    """two slips a one-pass kernel can make without touching its sibling: sum g_y*(c - mean) in place of sum g_y*xhat, and a
    bypass block's g_sc stored without scale_b"""
    N, H, W, C = 2, 32, 32, 16
    dt = torch.bfloat16
    go = kref.exact_operands((N, H, W, C), dt, seed=131, density=0.5, zero_tiles=0.2, exp=-1)
    c2 = kref.exact_operands((N, H, W, C), dt, seed=132, density=0.6, zero_tiles=0.2)
    cb = kref.exact_operands((N, H, W, C), dt, seed=133, density=0.6, zero_tiles=0.2)
    positive = kref.exact_operands((N, H, W, C), dt, seed=134, density=0.5, zero_tiles=0) > 0
    m2, s2, t2, i2 = _vectors(_site(C, 135))
    mb, sb, _, ib = _vectors(_site(C, 136))
    assert bool((i2 != 1).any()) and bool((sb != 1).any())
    g_c2, g_sc, [(db, a1), (dg, a2)], _ = kref.tail_bwd_frozen_ref(go, None, positive, c2, s2, t2, m2, i2, cb, sb, mb, ib)
    kref.assert_sums_exact(dg, dg, a2, 0.25, "reference itself")
    gz, gy2, _, _ = kref.tail_bwd_ref(go, None, positive, c2, s2, t2, m2, i2, cb, mb, ib)
    wrong = (gy2 * (c2.double() - m2)).reshape(-1, C).sum(0)
    with pytest.raises(AssertionError, match="channel"):
        kref.assert_sums_exact(wrong, dg, a2, 0.25, "centred input")
    kref.assert_exact(kref.round_to(g_sc, dt), g_sc, dt, g_sc.abs(), 2.0 ** -5, "reference itself")
    with pytest.raises(AssertionError, match="differ"):
        kref.assert_exact(kref.round_to(gz, dt), g_sc, dt, g_sc.abs(), 2.0 ** -5, "unscaled shortcut")


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


# ------------------------------------------------------------------------------------------------------------------
# parameter-side references (tests/test_gpu_param_exact.py)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fwd", [True, False])
def test_pack_ref_equals_pack_dense(dt, fwd):
    Cout, Cin, k = 24, 16, 3
    w = kref.exact_operands((Cout, Cin, k, k), torch.float32, seed=21, density=0.7)
    kk = k * k
    M, K, sm, sk = (Cout, Cin, Cin * kk, kk) if fwd else (Cin, Cout, kk, Cin * kk)
    img = kref.pack_ref(w, M, 32, K, K, sm, sk, range(kk), dt)
    assert img.dtype == dt and tuple(img.shape) == (kk, K // kref.CPU[dt], 32, kref.CPU[dt])
    assert torch.equal(kref.unpack_weights(img, K, M), kref.pack_dense(w, range(kk), fwd=fwd))
    assert not bool(img[:, :, M:, :].any())


def test_pack_ref_rounds_once_pads_and_scales():
    bf, h = torch.bfloat16, torch.float16
    src = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.0, 1023 * 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1 + 2.0 ** -11, 0.3],
                       dtype=torch.float32)
    got = kref.pack_ref(src, 1, 16, 8, 8, 0, 1, [0], bf)[0, 0, 0]
    assert got[0] == 1.0 and got[1] == 1 + 2.0 ** -6 and kref.bits(got[2:3]).item() == -32768       # ties to even; -0.0 kept
    goth = kref.pack_ref(src, 1, 16, 8, 8, 0, 1, [0], h)[0, 0, 0]
    assert goth[3] == 1023 * 2.0 ** -24 and goth[4] == 0 and goth[5] == 2 * 2.0 ** -24 and goth[6] == 1.0
    # K and M padding are +0; an offset and a scattered tap list address the source as the header says
    img = kref.pack_ref(torch.arange(100, dtype=torch.float32), 3, 16, 5, 8, 10, 2, [1, 0], torch.float32, src_offset=7)
    assert img[0, 1, 2, 0] == 7 + 2 * 10 + 4 * 2 + 1 and img[1, 0, 1, 3] == 7 + 10 + 3 * 2
    assert not bool(kref.bits(img[:, 1, :, 1:]).any()) and not bool(kref.bits(img[:, :, 3:, :]).any())
    # the scale is one fp32 multiply, then one rounding to the stored type: not the rounding of the exact product
    s = torch.tensor([1 + 2.0 ** -12])
    v = torch.tensor([1 + 2.0 ** -11 + 2.0 ** -13])               # v*s = 1 + 2^-11 + 2^-12 + ... -> fp32 -> f16 tie region
    one = kref.pack_ref(v, 1, 16, 1, 8, 0, 0, [0], h, oscale=s)[0, 0, 0, 0]
    assert one == (v.double() * s.double()).float().to(h)[0]


def test_bn_fold_ref_is_fp64_and_an_fp32_evaluation_misses_its_bound():
    g = torch.Generator().manual_seed(5)
    C = 256
    gamma, beta, mean = (torch.randn(C, generator=g) for _ in range(3))
    var = torch.rand(C, generator=g) + 0.01
    cb = torch.randn(C, generator=g)
    sc, bias, lim = kref.bn_fold_ref(gamma, beta, mean, var, 1e-5, cb)
    exact = (cb.double() - mean.double()) * (gamma.double() / (var.double() + kref.f32(1e-5)).sqrt()) + beta.double()
    assert torch.equal(bias, exact) and torch.equal(sc, (gamma.double() / (var.double() + kref.f32(1e-5)).sqrt()).float())
    assert bool(((bias.float().double() - bias).abs() <= lim).all())            # the correctly rounded value passes
    s32 = gamma / torch.sqrt(var + 1e-5)
    b32 = (cb - mean) * s32 + beta
    assert bool(((b32.double() - bias).abs() > lim).any())                      # fp32 arithmetic does not
    assert kref.ulp32(torch.tensor([1.0, 1.5, 0.75, 0.0], dtype=D)).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -24, 2.0 ** -149]


def test_finalize_refs_sum_in_stripe_order_and_model_the_accumulate_rounding():
    C = 5
    red = torch.zeros((32, 2 * C), dtype=D)
    red[0], red[1], red[2] = 1.0, 2.0 ** -60, -1.0                       # stripe order: (1 + 2^-60) - 1 = 0; any other order: 2^-60
    dg, db, k1, k2 = kref.bn_bwd_finalize_ref(red, C, 4.0)
    assert not bool(dg.any()) and not bool(k1.any())
    red[3] = 3.0
    dg0 = torch.full((C,), 2.0 ** 24)
    dg, db, k1, k2 = kref.bn_bwd_finalize_ref(red, C, 4.0, dg0, dg0.clone(), accumulate=True)
    assert torch.equal(dg, torch.full((C,), 2.0 ** 24 + 4)) and torch.equal(k2, torch.full((C,), 0.75))     # 2^24 + 3 rounds to even
    assert torch.equal(kref.bn_bwd_finalize_ref(red, C, None)[2], torch.zeros(C))
    src = torch.arange(64, dtype=D)
    assert torch.equal(kref.cast_ref(src, 16, 3, 3, 0.5), torch.tensor([24., 25.5, 27.]))
    inv, sc = kref.bn_eval_affine_ref(torch.tensor([2.0]), torch.tensor([0.75]), 0.25)
    assert inv.item() == 1.0 and sc.item() == 2.0
    # the clamp and count == 1 of bn_finalize_ref
    out = kref.bn_finalize_ref(torch.tensor([3.0], dtype=D), torch.tensor([8.9], dtype=D), 1.0, torch.ones(1), torch.zeros(1), 0.25,
                               torch.zeros(1), torch.ones(1), 0.5)
    assert out[3].item() == 2.0 and out[4].item() == 1.5 and out[5].item() == 0.5


def test_fma64_rounds_once():
    from fractions import Fraction
    g = torch.Generator().manual_seed(3)
    a = torch.randn(200, generator=g, dtype=D) * 1000
    b = a.clone()
    b[100:] = torch.randn(100, generator=g, dtype=D)
    c = -(a * b) * (1 + torch.randint(-4, 5, (200,), generator=g).double() * 2.0 ** -52)      # a*b + c cancels to the last bits
    c[150:] = torch.randn(50, generator=g, dtype=D)
    got = kref.fma64(a, b, c)
    exp = torch.tensor([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], dtype=D)
    assert torch.equal(got, exp) and not torch.equal(got, a * b + c)
    # bn_finalize_ref: both evaluations clamp a constant channel whose s2/count lies below m*m
    cnt, mc = 4096.0, 1000.1
    for fused in (False, True):
        out = kref.bn_finalize_ref(torch.tensor([cnt * mc], dtype=D), torch.tensor([cnt * (mc * mc * (1 - 2.0 ** -49))], dtype=D), cnt,
                                   torch.ones(1), torch.zeros(1), 0.25, torch.zeros(1), torch.ones(1), 0.5, fused=fused)
        assert out[3].item() == 2.0 and out[5].item() == 0.5


ADAM_FLAGS = [(s, wd, lr) for s in (1, 2, 100000) for wd in (0.0, 1e-4) for lr in (1e-5, 1e-3)]
# torch.optim.SGD refuses Nesterov momentum with zero momentum or non-zero dampening: those combinations have no torch.optim run
SGD_FLAGS = [(mom, damp, nest) for mom in (0.0, 0.9) for damp in (0.0, 0.5) for nest in (False, True)
             if not (nest and (mom == 0.0 or damp != 0.0))]


def _opt_operands(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 10.0 ** torch.empty(n).uniform_(-8, 3, generator=g) for _ in range(3)]
    return p, grads


@pytest.mark.parametrize("step0,wd,lr", ADAM_FLAGS)
def test_adam_ref_equals_torch_optim_in_float64(step0, wd, lr):
    p0, grads = _opt_operands(64, 7)
    f = kref.f32
    q = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([q], lr=f(lr), betas=(f(0.9), f(0.999)), eps=f(1e-8), weight_decay=f(wd))
    m, v = torch.zeros(64, dtype=D), torch.zeros(64, dtype=D)
    if step0 > 1:           # start from a state as of step0 - 1
        q.grad = grads[0].double()
        opt.step()
        st = opt.state[q]
        st["step"] = torch.tensor(float(step0 - 1)) if torch.is_tensor(st["step"]) else step0 - 1
        m, v = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    p = q.detach().clone()
    for i in range(3):
        (p, m, v), lims = kref.adam_ref(p, grads[i], m, v, lr, 0.9, 0.999, 1e-8, wd, step0 + i, round_bc=False)
        q.grad = grads[i].double()
        opt.step()
        for a, b in ((p, q.detach()), (m, opt.state[q]["exp_avg"]), (v, opt.state[q]["exp_avg_sq"])):
            assert float(((a - b).abs() / b.abs().clamp_min(1e-300)).max()) <= 1e-12
        assert all(bool(torch.isfinite(e).all()) and bool((e >= 0).all()) for e in lims)
    # the fp32-rounded bias corrections of the entry point move the step by at most two fp32 roundings
    (pa, _, _), _ = kref.adam_ref(p0, grads[0], m, v, lr, 0.9, 0.999, 1e-8, wd, step0, round_bc=True)
    (pb, _, _), _ = kref.adam_ref(p0, grads[0], m, v, lr, 0.9, 0.999, 1e-8, wd, step0, round_bc=False)
    assert bool(((pa - pb).abs() <= kref.gamma(3) * (pb - p0.double()).abs()).all())


@pytest.mark.parametrize("mom,damp,nest", SGD_FLAGS)
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_sgd_ref_equals_torch_optim_in_float64(mom, damp, nest, wd):
    p0, grads = _opt_operands(64, 9)
    f = kref.f32
    q = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.SGD([q], lr=f(1e-2), momentum=f(mom), dampening=f(damp), weight_decay=f(wd), nesterov=nest)
    p, buf = p0.double(), None
    for i in range(3):
        (p, buf), lims = kref.sgd_ref(p, grads[i], buf, 1e-2, mom, damp, wd, nest, i == 0)
        q.grad = grads[i].double()
        opt.step()
        assert float(((p - q.detach()).abs() / q.detach().abs().clamp_min(1e-300)).max()) <= 1e-12
        if mom:
            b = opt.state[q]["momentum_buffer"]
            assert float(((buf - b).abs() / b.abs().clamp_min(1e-300)).max()) <= 1e-12
        else:
            assert buf is None and lims[1] is None


def _f(x):
    return torch.tensor(x, dtype=torch.float32)


def _adam_f32(p, g, m, v, lr, b1, b2, eps, wd, step, gs):
    """adam_kernel's statements, one fp32 torch op per rounding (nothing fused)"""
    lr, b1, b2, eps, wd, gs = (_f(x) for x in (lr, b1, b2, eps, wd, gs))
    bc1, sbc2 = _f(1.0 - float(b1) ** step), _f((1.0 - float(b2) ** step) ** 0.5)
    gr = wd * p + g * gs
    m = m + (1 - b1) * (gr - m)
    v = b2 * v + (1 - b2) * gr * gr
    return p - (lr / bc1) * (m / (v.sqrt() / sbc2 + eps)), m, v


def _sgd_f32(p, g, buf, lr, mom, damp, wd, nest, first, gs):
    lr, mom, damp, wd, gs = (_f(x) for x in (lr, mom, damp, wd, gs))
    gr = wd * p + g * gs
    if float(mom) != 0:
        buf = gr if first else mom * buf + (1 - damp) * gr
        gr = mom * buf + gr if nest else buf
    return p - lr * gr, buf


@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_optimizer_bounds_cover_a_float32_run_and_catch_a_skipped_element(gs):
    """the running-error bounds hold for the kernels' statements evaluated in fp32 with nothing fused, and an element that was
    left untouched is outside them"""
    p, grads = _opt_operands(4096, 11)
    for step0, wd, lr in ADAM_FLAGS:
        m, v = torch.zeros(4096), torch.zeros(4096)
        for i in range(3):
            (p64, m64, v64), lims = kref.adam_ref(p, grads[i], m, v, lr, 0.9, 0.999, 1e-8, wd, step0 + i, gs)
            got = _adam_f32(p, grads[i], m, v, lr, 0.9, 0.999, 1e-8, wd, step0 + i, gs)
            for a, ref, lim in zip(got, (p64, m64, v64), lims):
                assert bool(((a.double() - ref).abs() <= lim).all())
            assert bool(((m.double() - m64).abs() > lims[1]).any()) and bool(((v.double() - v64).abs() > lims[2]).any())
            if lr == 1e-3:
                assert bool(((p.double() - p64).abs() > lims[0]).any())
            _, m, v = got
    for mom in (0.0, 0.9):
        for damp in (0.0, 0.5):
            for nest in (False, True):
                buf = None
                for i in range(3):
                    (p64, b64), (Ep, Eb) = kref.sgd_ref(p, grads[i], buf, 1e-2, mom, damp, 1e-4, nest, i == 0, gs)
                    gp, buf = _sgd_f32(p, grads[i], buf, 1e-2, mom, damp, 1e-4, nest, i == 0, gs)
                    assert bool(((gp.double() - p64).abs() <= Ep).all()) and bool(((p.double() - p64).abs() > Ep).any())
                    if mom:
                        assert bool(((buf.double() - b64).abs() <= Eb).all())


def test_tile_refs_crop_with_zero_fill_and_stitch_only_inside_keep_windows():
    import numpy as np
    view = np.arange(2 * 5 * 7, dtype=np.float32).reshape(2, 5, 7) + 1
    crop = kref.crop_tiles_ref(view, [(1, 3, 4, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0)], 4, 6)
    assert np.array_equal(crop[0, :2, :3], view[1, 3:5, 4:7]) and not crop[0, 2:].any() and not crop[0, :, 3:].any()
    assert np.array_equal(crop[1], view[0, :4, :6])
    out = np.full((2, 1, 5, 7), np.nan, dtype=np.float32)
    scores = np.stack([crop[0][None], crop[1][None]])
    kref.stitch_tiles_ref(scores, [(1, 3, 4, 0, 4, 0, 6), (0, 0, 0, 1, 3, 2, 2)], out)
    assert np.array_equal(out[1, 0, 3:5, 4:7], view[1, 3:5, 4:7]) and int(np.isnan(out).sum()) == out.size - 6


# ------------------------------------------------------------------------------------------------------------------
# edge-value table (kref.edge_table / edge_values / assert_bits)
# ------------------------------------------------------------------------------------------------------------------
def _t_from_bits(b, dt):
    """fp64 value of bit pattern b of the 16-bit type (no rounding involved: widening is exact)"""
    return float(torch.tensor([b], dtype=torch.int32).to(torch.int16).view(dt).double())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_edge_table_holds_what_its_class_names_say(dt):
    names = kref.edge_names(dt)
    v = kref.edge_values(dt)
    assert len(names) == v.numel() and v.dtype == torch.float32
    r = v.to(dt)                                   # torch's conversion: RNE, the reference
    fi = torch.finfo(dt)
    seen = set()
    for i, nm in enumerate(names):
        neg = nm.startswith("-")
        base = nm.lstrip("-")
        seen.add(base)
        x, rx = v[i:i + 1], r[i:i + 1]
        assert bool(torch.signbit(x)) == neg, nm
        if base in kref.NAN_CLASSES:
            assert bool(torch.isnan(x)) and bool(torch.isnan(rx)), nm
            if base == "nan_low_payload":
                b = int(x.view(torch.int32)) & 0x7fffffff
                assert b >> 16 == 0x7f80 and b & 0xffff, nm            # truncation gives infinity
                assert ((b + 0x7fff) >> 16) == 0x7f80, nm
            continue
        mag, rmag = abs(float(x)), abs(float(rx))
        if base.startswith("tie_"):
            # neighbours from the T bit patterns b and b + 1, independent of the conversion under reference
            kind = "tie_even" if base.startswith("tie_even") else "tie_odd"
            seq = [j for j, n in enumerate(names) if n == ("-" if neg else "") + base]
            b = kref.tie_bases(dt)[kind][seq.index(i)]
            lo, hi = _t_from_bits(b, dt), _t_from_bits(b + 1, dt)
            assert (b & 1) == (0 if kind == "tie_even" else 1) and 0 < lo < hi, nm
            if base == kind:
                assert hi - mag == mag - lo > 0, nm                        # both neighbours equidistant, in fp64
                assert rmag == (lo if kind == "tie_even" else hi), nm       # RNE: the neighbour with the even last bit
            else:
                tie = float((x.abs().view(torch.int32) + (-1 if base.endswith("above") else 1)).view(torch.float32))
                assert hi - tie == tie - lo and (mag > tie) == base.endswith("above"), nm
                assert rmag == (hi if base.endswith("above") else lo), nm
        elif base == "t_max":
            assert mag == fi.max and rmag == fi.max, nm
        elif base == "overflow_tie":
            assert mag == fi.max + (fi.max - float(torch.nextafter(torch.tensor(fi.max, dtype=dt), torch.tensor(0., dtype=dt)))) / 2 and rmag == float("inf"), nm
        elif base == "overflow_below":
            assert rmag == fi.max and mag > fi.max, nm
        elif base == "flt_max":
            assert mag == torch.finfo(torch.float32).max and rmag == float("inf"), nm
        elif base == "t_subnormal_min":
            assert mag == fi.smallest_normal * fi.eps and rmag == mag, nm
        elif base == "t_subnormal_half":
            assert mag == fi.smallest_normal * fi.eps / 2 and rmag == 0.0 and bool(torch.signbit(rx)) == neg, nm
        elif base == "t_subnormal_half_above":
            assert rmag == fi.smallest_normal * fi.eps and mag < rmag, nm
        elif base == "t_subnormal_max":
            assert mag == fi.smallest_normal * (1 - fi.eps) and rmag == mag, nm
        elif base == "t_normal_min":
            assert mag == fi.smallest_normal and rmag == mag, nm
        elif base.startswith("f32_subnormal"):
            assert 0 < mag < torch.finfo(torch.float32).smallest_normal, nm
        elif base == "zero":
            assert mag == 0 and rmag == 0 and bool(torch.signbit(rx)) == neg, nm
        elif base == "inf":
            assert mag == float("inf") and rmag == float("inf"), nm
        else:
            raise AssertionError("unknown class " + nm)
    assert {"tie_even", "tie_odd", "tie_even_above", "tie_odd_below", "t_max", "overflow_tie", "overflow_below", "flt_max", "t_subnormal_min",
            "t_subnormal_half", "t_subnormal_half_above", "t_subnormal_max", "t_normal_min", "f32_subnormal", "zero", "inf", "nan",
            "nan_low_payload"} <= seen
    # ties at several exponents, a value that rounds to 0 although it is > 0, one that rounds to the largest finite
    assert len({torch.frexp(v[i])[1].item() for i, n in enumerate(names) if n == "tie_even"}) >= 4
    assert any(float(v[i]) > 0 and float(r[i]) == 0 for i in range(len(names)))


def test_edge_table_float32_and_filters():
    names = kref.edge_names(torch.float32)
    v = kref.edge_values(torch.float32)
    tiny, big = 2.0 ** -149, float(torch.finfo(torch.float32).max)
    want = {"f32_subnormal_min": tiny, "f32_subnormal": 0x12345 * tiny, "f32_subnormal_max": 2.0 ** -126 - tiny, "zero": 0.0,
            "inf": float("inf"), "flt_max": big, "nan": None}
    assert {n.lstrip("-") for n in names} == set(want) and len(names) == 2 * len(want)
    for i, n in enumerate(names):
        w = want[n.lstrip("-")]
        assert bool(torch.signbit(v[i])) == n.startswith("-"), n
        assert bool(torch.isnan(v[i])) if w is None else abs(float(v[i].double())) == w, n
    assert big == (2.0 - 2.0 ** -23) * 2.0 ** 127
    v = kref.edge_values(torch.float32, exclude=kref.NAN_CLASSES)
    assert not bool(torch.isnan(v).any()) and v.numel() == len(names) - 2
    fin = kref.edge_values(torch.float16, exclude=kref.NAN_CLASSES + ("inf", "flt_max", "overflow_tie"))
    assert bool(torch.isfinite(fin.to(torch.float16)).all())
    # the ties reach from the subnormal range to the top binade of either type
    for dt in (torch.bfloat16, torch.float16):
        t = kref.edge_values(dt, classes=("tie_even",)).abs()
        fi = torch.finfo(dt)
        assert float(t.min()) < fi.smallest_normal and float(t.max()) > fi.max / 2


def test_assert_bits_tells_signed_zeros_and_nans():
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        a = torch.tensor([0.0, -0.0, float("nan"), float("inf"), 1.0]).to(dt)
        kref.assert_bits(a, a.clone())
        nan2 = a.clone()
        nan2[2] = -a[2]                                   # another NaN bit pattern
        kref.assert_bits(a, nan2)
        z = a.clone()
        z[1] = 0.0
        with pytest.raises(AssertionError, match="differ in bits"):
            kref.assert_bits(a, z)
        kref.assert_bits(a, z, zero_sign=False)
        for j, val in ((2, float("inf")), (3, float("nan")), (4, 1.0 + 2.0 ** -7)):
            b = a.clone()
            b[j] = val
            with pytest.raises(AssertionError, match="differ in bits"):
                kref.assert_bits(a, b, zero_sign=False)
    kref.assert_bits(torch.tensor([1, 2], dtype=torch.uint8), torch.tensor([1, 2], dtype=torch.uint8))
    with pytest.raises(AssertionError):
        kref.assert_bits(torch.tensor([1, 2], dtype=torch.uint8), torch.tensor([1, 3], dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------------
# bounds for launches replayed on inexact operands (tests/stage_shadow.py)
# ------------------------------------------------------------------------------------------------------------------
def _inexact(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_inexact_bounds_cover_a_float32_evaluation_and_miss_a_wrong_site(dt):
    """the kernels' statements evaluated in fp32 (torch, no contraction) and stored in `dt` lie inside tail_fwd_bound /
    apply_bound / xf_operand_err; the same evaluation with another site's mean lies outside"""
    C, shape = 16, (2, 9, 7, 16)
    c2, sc = _inexact(shape, 1).to(dt), _inexact(shape, 2).to(dt)
    m2, s2, t2 = _inexact((C,), 3, 0.1), _inexact((C,), 4).abs() + 0.5, _inexact((C,), 5, 0.3)
    mb, sb, tb = _inexact((C,), 6, 0.1), _inexact((C,), 7).abs() + 0.5, _inexact((C,), 8, 0.3)

    def tail(mean2):
        r2 = ((c2.float() - mean2) * s2 + t2).clamp_min(0)
        return (r2 + ((sc.float() - mb) * sb + tb)).clamp_min(0).to(dt)
    ref, lim = kref.tail_fwd_bound(c2, m2, s2, t2, sc, dt, mb, sb, tb)
    kref.assert_within(tail(m2), ref, lim, "tail")
    with pytest.raises(AssertionError):
        kref.assert_within(tail(mb), ref, lim, "tail with bnpass's mean")
    # apply pass
    gy, k1, k2, inv = _inexact(shape, 9).to(dt), _inexact((C,), 10, 0.05), _inexact((C,), 11, 0.05), _inexact((C,), 12).abs() + 0.5
    d = c2.float() - m2
    got = (s2 * (gy.float() - k1 - (d * inv) * k2)).to(dt)
    xh = (c2.double() - m2.double()) * inv.double()
    ref, lim = kref.apply_bound(gy.double(), xh, s2, k1, k2, dt)
    kref.assert_within(got, ref, lim, "apply")
    with pytest.raises(AssertionError):
        kref.assert_within((sb * (gy.float() - k1 - (d * inv) * k2)).to(dt), ref, lim, "apply with bnpass's scale")
    # an operand transformed on load, then packed to the compute type
    lo = torch.zeros(C)
    got = torch.maximum((c2.float() - m2) * s2 + t2, lo).to(dt)
    want = torch.maximum((c2.double() - m2.double()) * s2.double() + t2.double(), lo.double())
    kref.assert_within(got, want, kref.xf_operand_err(c2, (m2, s2, t2, lo), dt), "operand")
    assert float(kref.xf_operand_err(c2, None, dt).abs().max()) == 0.0


def test_reduce_bound_covers_float32_partials_and_an_open_gate():
    C, shape = 16, (2, 24, 40, 16)
    g32, c32, m32, i32 = _inexact(shape, 1), _inexact(shape, 2), _inexact((C,), 3, 0.1), _inexact((C,), 4).abs() + 0.5
    gy, xh = g32.double(), (c32.double() - m32.double()) * i32.double()
    L = kref.reduce_chain(2 * 24 * 40, C, torch.bfloat16)
    assert L == (1920 * 2 + 256 * kref.pick_blocks(1920, 2, 512, 8) - 1) // (256 * kref.pick_blocks(1920, 2, 512, 8)) + 6
    s, sx, l1, l2 = kref.reduce_bound(gy, xh, L)
    # the kernel's statements in fp32: xhat = fl(fl(c - mean) * invstd), the term fl(g_y * xhat): the three roundings reduce_bound
    # counts on top of the chain.  Then fp32 partials of L terms each, added in fp64.  The limits stand on their own.
    g32, t32 = g32.reshape(-1, C), (g32 * ((c32 - m32) * i32)).reshape(-1, C)
    parts = lambda v: sum(v[i:i + L].sum(0, dtype=torch.float32).double() for i in range(0, v.shape[0], L))
    assert bool(((parts(g32) - s).abs() <= l1).all()) and bool(((parts(t32) - sx).abs() <= l2).all())
    # one term dropped is outside, unless its gate is open
    drop = g32.clone()
    drop[5] = 0
    assert not bool(((parts(drop) - s).abs() <= l1).all())
    opn = torch.zeros(shape, dtype=torch.bool).reshape(-1, C)
    opn[5] = True
    _, _, o1, _ = kref.reduce_bound(gy, xh, L, opn.reshape(shape))
    assert bool(((parts(drop) - s).abs() <= o1).all())
    assert kref.gate_open(torch.tensor([1e-9, 0.5]), torch.tensor([1.0, 1.0])).tolist() == [True, False]


def test_stored_stats_and_eval_affine_bounds():
    dt = torch.float16
    ref = _inexact((2, 5, 7, 16), 1).double()
    pre = ref.abs() * 1e-4
    lim = kref.stored_bound(ref, pre, dt)
    kref.assert_within((ref * (1 + 1e-4)).float().to(dt), ref, lim, "a value inside pre, then stored")
    assert not bool((((ref * (1 + 2e-3)).float().to(dt).double() - ref).abs() <= lim).all())
    z = torch.zeros(3, dtype=torch.float64)
    assert float(kref.stored_bound(z, z, dt).max()) == 0.0                   # nothing in, nothing allowed out
    assert float(kref.stored_bound(z + 1e-9, z, dt).min()) >= kref.TINY[dt]    # a subnormal result may miss by half a spacing
    # statistics of values that are themselves off by up to pre
    s, l = kref.conv_stats_bound(ref, pre, 2, 5, 7)
    v = (ref * (1 + 1e-4)).float()
    got = torch.cat([v.reshape(-1, 16).sum(0, dtype=torch.float32).double(), (v * v).reshape(-1, 16).sum(0, dtype=torch.float32).double()])
    assert bool(((got - s).abs() <= l).all())
    s0, l0 = kref.conv_stats_bound(ref, torch.zeros_like(ref), 2, 5, 7)
    assert not bool(((got - s0).abs() <= l0).all())
    # ubr_bn_eval_affine's statements in fp32
    g, rv, eps = _inexact((64,), 2), _inexact((64,), 3).abs() + 0.1, 1e-5
    inv32 = 1.0 / torch.sqrt(rv + torch.tensor(eps))
    (inv, li), (sc, ls) = kref.bn_eval_affine_bound(g, rv, eps)
    assert bool(((inv32.double() - inv).abs() <= li).all()) and bool((((g * inv32).double() - sc).abs() <= ls).all())
    assert not bool(((1.0 / torch.sqrt(rv)).double() - inv).abs().le(li).all())


def test_logsoftmax_bound_covers_perturbed_logits_and_misses_a_shifted_class():
    """kref.logsoftmax_bound: the epilogue in fp32 on logits that are off by up to `pre` stays inside; a bias of 3 pre on one class does not"""
    g = torch.Generator().manual_seed(5)
    v = torch.randn((2, 9, 7, 3), generator=g, dtype=torch.float64) * 4
    pre = (torch.rand(v.shape, generator=g, dtype=torch.float64) + 0.1) * 1e-4
    ref, lim = kref.logsoftmax_bound(v, pre)
    for seed in range(8):
        d = (torch.rand(v.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1) * pre
        v32 = (v + d).float()                                    # the kernel's fp32 logits, then its statements in fp32
        m = v32.amax(-1, keepdim=True)
        got = v32 - (m + torch.log(torch.exp(v32 - m).sum(-1, keepdim=True)))
        kref.assert_within(got, ref, lim, "log-softmax of perturbed logits")
    # worst case of the derivation: one class up by pre, the others down by pre
    d = -pre.clone()
    d[..., 0] = pre[..., 0]
    kref.assert_within(torch.log_softmax(v + d, -1), ref, lim, "extreme perturbation")
    # the propagated term is 2 max pre per pixel on top of the epilogue's own bound, no more
    assert torch.equal(lim, kref.logsoftmax_ref(v)[1] + 2 * pre.amax(-1, keepdim=True))
    d = torch.zeros_like(v)
    d[..., 1] = 3 * pre.amax(-1) + 1e-5
    with pytest.raises(AssertionError):
        kref.assert_within(torch.log_softmax(v + d, -1), ref, lim, "a class shifted beyond the bound")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_pool_xf_bound_covers_a_float32_evaluation_stored_once(dt):
    """the stem pool's statements in fp32 (affine + ReLU per tap, maximum, ONE store of pooled and of the copy): inside
    kref.pool_xf_bound; pooled is the stored copy at the arg-max tap, which lies within twice its bound of the fp64 maximum;
    the same with another channel's shift is outside"""
    C, shape = 16, (2, 10, 14, 16)
    x = _inexact(shape, 1).to(dt)
    sub, sc, sh, lo = _inexact((C,), 2, 0.1), _inexact((C,), 3).abs() + 0.5, _inexact((C,), 4, 0.3), torch.zeros(C)
    t32 = torch.maximum((x.float() - sub) * sc + sh, lo)
    xcopy = t32.to(dt)
    p32, am, _ = kref.maxpool_ref(t32, None, 2)            # (exact on fp32 inputs: the kernel's maximum and first arg-max)
    pooled = p32.float().to(dt)
    ref_p, lim_p, am64, t, lim_t = kref.pool_xf_bound(x, (sub, sc, sh, lo), 2, dt)
    kref.assert_within(xcopy, t, lim_t, "xcopy")
    kref.assert_within(pooled, ref_p, lim_p, "pooled")
    got, inside = kref.window_take(xcopy, am, 2)
    assert bool(inside.all()) and torch.equal(got, pooled)
    tv, _ = kref.window_take(t, am, 2)
    lv, _ = kref.window_take(lim_t, am, 2)
    assert bool(((ref_p - tv) <= 2 * lv).all()) and bool((ref_p >= tv).all())
    # a tap outside the image is reported; a window's wrong tap is (nearly always) further than twice its bound from the maximum
    bad = am.clone()
    bad[:, 0, :, :] = 0                                        # row -1
    assert not bool(kref.window_take(xcopy, bad, 2)[1].all())
    other = (am + 4) % 9
    ov, oin = kref.window_take(t, other, 2)
    olv, _ = kref.window_take(lim_t, other, 2)
    assert int((((ref_p - ov) > 2 * olv) & oin).sum()) > 0.5 * int(oin.sum())
    with pytest.raises(AssertionError):
        kref.assert_within(torch.maximum((x.float() - sub) * sc + sh.roll(1), lo).to(dt), t, lim_t, "xcopy with a neighbour's shift")
    # near-ties: two taps closer than the fp32 error resolve either way inside the window the check allows
    z = torch.zeros((1, 2, 2, 8))
    z[0, 0, 0], z[0, 1, 1] = 1.0, 1.0
    rp, lp, amz, tz, lz = kref.pool_xf_bound(z.to(dt), (torch.zeros(8), torch.ones(8), torch.zeros(8), torch.zeros(8)), 2, dt)
    for tap in (4, 8):
        tv, inside = kref.window_take(tz, torch.full((1, 1, 1, 8), tap), 2)
        assert bool(inside.all()) and bool(((rp - tv) <= 2 * kref.window_take(lz, torch.full((1, 1, 1, 8), tap), 2)[0]).all())
    assert not bool(((rp - kref.window_take(tz, torch.full((1, 1, 1, 8), 5), 2)[0]) <= 2 * kref.window_take(lz, torch.full((1, 1, 1, 8), 5), 2)[0]).all())


def test_nominal_abs_covers_products_aligned_at_the_subnormal_exponent():
    """kref.nominal_abs: a dot product whose f16 subnormal operand is multiplied as 0.m * 2^-14 and whose sum keeps 24 bits below
    the largest NOMINAL product exponent (bits below are dropped) stays inside gamma(K) of the nominal sum of |terms| and falls
    outside gamma(K) of the plain one; the values are those measured on the device (tests/kref.py, the note above nominal_abs)"""
    g = torch.tensor([37 * 2.0 ** -24, 9 * 2.0 ** -24], dtype=torch.float16)
    x = torch.tensor([1177 * 2.0 ** -15, 1514 * 2.0 ** -10], dtype=torch.float16)
    assert g.double().tolist() == [37 * 2.0 ** -24, 9 * 2.0 ** -24] and x.double().tolist() == [1177 * 2.0 ** -15, 1514 * 2.0 ** -10]
    ref = float((g.double() * x.double()).sum())
    assert ref == 479581 * 2.0 ** -39
    # the model: nominal exponent of a product = 2^-14 (g has no hidden bit) times 2^floor(log2 x); 24 bits are kept below the largest
    top = max(-14 + math.floor(math.log2(float(v))) for v in x)
    q = 2.0 ** (top - 24)
    got = sum(math.floor(float(a) * float(b) / q) * q for a, b in zip(g.double(), x.double()))
    assert got == 479580 * 2.0 ** -39                                   # what the MI355X returned
    K = 2
    plain = kref.C_ACC * K * kref.U32 * float((g.double().abs() * x.double().abs()).sum()) + kref.U32 * abs(ref)
    nominal = kref.C_ACC * K * kref.U32 * float((kref.nominal_abs(g, torch.float16) * kref.nominal_abs(x, torch.float16)).sum()) + kref.U32 * abs(ref)
    assert plain < abs(got - ref) <= nominal
    # zero stays zero, normal values and the other types are untouched
    v = torch.tensor([0.0, 2.0 ** -24, -2.0 ** -15, 2.0 ** -14, -0.5], dtype=torch.float16)
    assert kref.nominal_abs(v, torch.float16).tolist() == [0.0, 2.0 ** -14, 2.0 ** -14, 2.0 ** -14, 0.5]
    assert torch.equal(kref.nominal_abs(v.to(torch.bfloat16), torch.bfloat16), v.double().abs())
