"""ubr_aspp_front (the five branches of an ASPP level in one launch), bit for bit against a float64 restatement written from
its descriptor in include/ubresnet_hip.h, on the exact dyadic operands of tests/kref.py:

    y[..., 16b:16b+16] = relu(conv_b(x) + bias[16b:16b+16])   b = 0..3: 1x1, 3x3, 3x3 dilation 3, 3x3 dilation 5; taps of the
                                                              packed image: 0 = B1, 1..9 = B2, 10..18 = B3, 19..27 = B4
    y[..., 64:64+C]    = MaxPool2d(3, 1, 1)(x), padding = minus infinity

at the three ASPP levels of a 512 x 832 tile (N = 1 and the whole-view batch N = 10) and at a shape whose height and width
are no multiples of the kernel's pixel tile, for f16, bf16 and fp32.  Input and output are channel slices of wider buffers
whose every other element (guard bands included) holds a NaN sentinel: a read outside the input shows up in the output, a
write outside the 64 + C channels is caught by the sentinel check.  assert_exact() asserts its own budget."""
import pytest
import torch
import torch.nn.functional as F

import kref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import _lib as L
    from ubresnet_amd import ops, plan

DEV = "cuda"
BRANCHES = [(1, 1), (3, 1), (3, 3), (3, 5)]          # (kernel, dilation) in concat order
LEVELS = [(64, 104, 128), (32, 52, 256), (16, 26, 512)]
SHAPES = [(n, h, w, c) for (h, w, c) in LEVELS for n in (1, 10)] + [(2, 13, 21, 128), (1, 5, 3, 64)]
DTYPES = [torch.float16, torch.bfloat16, torch.float32]


def front_taps():
    """[(branch, [(dy, dx, tap of the packed image)])] as the header states them"""
    out, t = [], 0
    for k, dil in BRANCHES:
        taps = []
        for ky in range(k):
            for kx in range(k):
                taps.append(((ky - k // 2) * dil, (kx - k // 2) * dil, t))
                t += 1
        out.append(taps)
    assert t == 28
    return out


def front_ref(x, wp, bias):
    """fp64 (ref, absref) [N,h,w,64+C] of one ubr_aspp_front launch; the pool slice's budget is |x| (a selection, no sum)"""
    N, h, w, Cn = x.shape
    W = kref.unpack_weights(wp, Cn, 16)
    refs, abss = [], []
    for b, taps in enumerate(front_taps()):
        r, a = kref.conv_ref(x, W, taps, 16, h, w, bias=bias[16 * b:16 * b + 16], act=1)
        refs.append(r)
        abss.append(a)
    pooled = kref.maxpool_ref(x, None, 1)[0]
    refs.append(pooled)
    abss.append(pooled.abs())
    return torch.cat(refs, 3), torch.cat(abss, 3)


def guarded(shape, dt, lead, trail, seed):
    """NaN-filled flat buffer holding an NHWC view of `shape` as the channel slice [lead, lead + C) of pixels lead + C + trail
    wide, with 256 guard elements on either side -> (buffer, view)"""
    N, h, w, Cn = shape
    ps = lead + Cn + trail
    buf = torch.full((512 + N * h * w * ps,), float("nan"), dtype=dt, device=DEV)
    view = buf.as_strided((N, h, w, Cn), (h * w * ps, w * ps, ps, 1), 256 + lead)
    return buf, view


def operands(shape, dt, seed):
    N, h, w, Cn = shape
    cpu = kref.CPU[dt]
    xbuf, x = guarded(shape, dt, 32, 32, seed)
    x.copy_(kref.exact_operands(shape, dt, density=0.25, seed=seed, exp=0, device=DEV))
    wp = kref.exact_operands((28, Cn // cpu, 16, cpu), dt, density=0.5, seed=seed + 1, exp=-1, zero_tiles=0, device=DEV)
    bias = kref.exact_operands((64,), torch.float32, density=0.8, seed=seed + 2, exp=-2, device=DEV)
    ybuf, y = guarded((N, h, w, 64 + Cn), dt, 32, 32, seed)
    return x, wp, bias, ybuf, y


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_aspp_front_exact(shape, dt):
    x, wp, bias, ybuf, y = operands(shape, dt, 4000 + 7 * sum(shape))
    before = ybuf.clone()
    written = torch.zeros(ybuf.numel(), dtype=torch.bool, device=DEV)
    written.as_strided(y.shape, y.stride(), y.storage_offset()).fill_(True)
    ops.aspp_front(x, wp, bias, y)
    torch.cuda.synchronize()
    ref, absref = front_ref(x, wp, bias)
    # products are multiples of 2^-1, the bias of 2^-2
    kref.assert_exact(y, ref, dt, absref=absref, unit=0.25, what="aspp_front %s %s" % (shape, dt))
    kref.assert_untouched(ybuf, before, written, "aspp_front %s %s" % (shape, dt))
    assert float(y[..., :64].float().abs().max()) > 0, "the exact operands must reach the outputs"
    for b in range(4):
        assert float(y[..., 16 * b:16 * b + 16].float().max()) > 0, "branch %d is all zero" % b


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16", "f32"])
def test_pool_slice_equals_max_pool2d_on_dense_input(dt):
    N, h, w, Cn = 2, 19, 37, 128
    cpu = kref.CPU[dt]
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((N, h, w, Cn), generator=g, device=DEV).to(dt)
    wp = torch.zeros((28, Cn // cpu, 16, cpu), dtype=dt, device=DEV)
    bias = torch.zeros(64, dtype=torch.float32, device=DEV)
    y = torch.full((N, h, w, 64 + Cn), float("nan"), dtype=dt, device=DEV)
    ops.aspp_front(x, wp, bias, y)
    want = F.max_pool2d(x.permute(0, 3, 1, 2).float(), 3, 1, 1).permute(0, 2, 3, 1).to(dt)
    assert torch.equal(y[..., 64:], want)
    assert torch.equal(y[..., :64], torch.zeros_like(y[..., :64]))


def test_wider_destination_keeps_its_other_channels():
    dt = torch.float16
    shape = (1, 16, 26, 512)
    x, wp, bias, _, _ = operands(shape, dt, 77)
    N, h, w, Cn = shape
    full = torch.full((N, h, w, 64 + Cn + 64), 7.0, dtype=dt, device=DEV)      # a concat buffer with 64 channels behind the slice
    ops.aspp_front(x, wp, bias, full)
    assert torch.equal(full[..., 64 + Cn:], torch.full_like(full[..., 64 + Cn:], 7.0))
    ref, absref = front_ref(x, wp, bias)
    kref.assert_exact(full[..., :64 + Cn], ref, dt, absref=absref, unit=0.25, what="wider destination")


@pytest.mark.parametrize("dt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_replays_identically_from_a_tape(dt):
    shape = (3, 32, 52, 256)
    x, wp, bias, ybuf, y = operands(shape, dt, 91)
    tape = plan.Tape()
    st = [L.stream_ptr()]
    tape.begin(st)
    try:
        ops.aspp_front(x, wp, bias, y)
    finally:
        tape.end()
    assert tape.size() == 1, "one launch per ASPP level front"
    torch.cuda.synchronize()
    first = ybuf.clone()
    y.fill_(float("nan"))
    tape.replay(st)
    torch.cuda.synchronize()
    assert torch.equal(ybuf.view(torch.int16 if dt == torch.float16 else torch.int32), first.view(torch.int16 if dt == torch.float16 else torch.int32))
    ref, absref = front_ref(x, wp, bias)
    kref.assert_exact(y, ref, dt, absref=absref, unit=0.25, what="replayed aspp_front")


def test_rejects_what_it_cannot_run():
    dt = torch.float16
    x = torch.zeros((1, 8, 8, 128), dtype=dt, device=DEV)
    wp = torch.zeros((28, 16, 16, 8), dtype=dt, device=DEV)
    bias = torch.zeros(64, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.aspp_front(x, wp, bias, torch.zeros((1, 8, 8, 64 + 127), dtype=dt, device=DEV))        # too narrow
    with pytest.raises(RuntimeError):
        ops.aspp_front(x, wp[:27], bias, torch.zeros((1, 8, 8, 192), dtype=dt, device=DEV))         # a tap short
    # an image beyond 2 GiB of 32-bit offsets: the descriptor is refused on the host, nothing is launched
    d = L.AsppFrontDesc()
    d.dtype, d.N, d.H, d.W, d.C = L.F16, 1, 1 << 16, 1 << 8, 128
    d.x = L.Tensor(x.data_ptr(), 1 << 31, 1 << 15, 128)
    d.y = L.Tensor(x.data_ptr(), 1 << 31, 1 << 15, 192)
    d.w, d.bias = wp.data_ptr(), bias.data_ptr()
    import ctypes as C
    assert L.lib().ubr_aspp_front(C.byref(d), L.stream_ptr()) == -1
    assert b"32-bit" in L.lib().ubr_last_error()
