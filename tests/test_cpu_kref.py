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
