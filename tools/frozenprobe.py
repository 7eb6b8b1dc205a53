#!/usr/bin/env python3
"""Frozen-BatchNorm backward: the one-pass kernels against the two launches they replace, and the whole frozen step against
the train-mode step.  usage: python tools/frozenprobe.py [batch] [out.txt]

Part 1, per block-tail shape of the ip16 network on 512x512 images (bf16): ubr_block_tail_bwd's UBR_PASS_FROZEN against
its UBR_PASS_REDUCE + UBR_PASS_APPLY_FIN (masked), and the same passes of ubr_bn_bwd; old and new alternate, REPS rounds of ITERS launches each, median and spread (max - min over rounds) per
launch, achieved bytes/s of the one-pass kernel from its algorithmic bytes.
Part 2: train step (forward, loss, backward, FlatAdam) in train mode and with every BatchNorm frozen, alternated.
Event timing, profiler off."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ubresnet_amd import ops, synthetic
from ubresnet_amd.models.ub_uresnet import UResNet
from ubresnet_amd.optim import FlatAdam
from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
OUT = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
DT, DEV, REPS, ITERS = torch.bfloat16, "cuda", 7, 20


def say(s):
    print(s, flush=True)
    if OUT:
        OUT.write(s + "\n")
        OUT.flush()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS      # us per call


def ab(old, new):
    for f in (old, new):
        f()
    torch.cuda.synchronize()
    to, tn = [], []
    for _ in range(REPS):
        to.append(timed(old))
        tn.append(timed(new))
    return statistics.median(to), max(to) - min(to), statistics.median(tn), max(tn) - min(tn)


say("# one-pass frozen backward vs reduce + apply_fin, bf16, batch %d; us per call: median (spread over %d rounds of %d)" % (B, REPS, ITERS))
for side, C in [(512, 16), (256, 32), (128, 64), (64, 128), (32, 256), (16, 512)]:
    shape = (B, side, side, C)
    npix = B * side * side
    T = lambda: torch.randn(shape, device=DEV).to(DT)
    V = lambda: torch.rand(C, device=DEV) + 0.5
    go, c2, cb = T(), T(), T()
    g_c2, g_sc = torch.empty_like(c2), torch.empty_like(c2)
    mask = torch.randint(0, 256, (npix * (C // 8),), device=DEV, dtype=torch.uint8)
    s2, t2, m2, i2, sb, mb, ib = [V() for _ in range(7)]
    r2, rb = ops.stat_buffer(2 * C, DEV), ops.stat_buffer(2 * C, DEV)
    dg = [torch.empty(C, device=DEV) for _ in range(4)]
    tensor_bytes = npix * C * 2
    for byp in (False, True):
        a = (cb, mb, ib) if byp else (None, None, None)
        gs = g_sc if byp else None

        def old():
            ops.block_tail_bwd_reduce(go, None, None, c2, s2, t2, m2, i2, a[0], a[1], a[2], r2, rb if byp else None, relu_mask=mask)
            ops.block_tail_bwd_apply_fin(go, None, mask, c2, s2, t2, m2, i2, r2, dg[0], dg[1], a[0], sb if byp else None, a[1], a[2],
                                         rb if byp else None, dg[2] if byp else None, dg[3] if byp else None, npix, g_c2, gs)

        def new():
            ops.block_tail_bwd_frozen(go, None, mask, c2, s2, t2, m2, i2, r2, a[0], sb if byp else None, a[1], a[2], rb if byp else None, g_c2, gs)
        o, so, n, sn = ab(old, new)
        nbytes = tensor_bytes * (5 if byp else 3) + npix * (C // 8)
        say("tail %4dx%-4d C=%-3d %-8s two-pass %7.1f (%.1f)  one-pass %7.1f (%.1f)  x%.2f  %5.2f TB/s (%.0f%% of 6.29)  %s"
            % (side, side, C, "bypass" if byp else "identity", o, so, n, sn, o / n, nbytes / n * 1e-6, 100 * nbytes / n * 1e-6 / 6.29,
               "FASTER" if o - n > max(so, sn) else "NOT faster beyond the spread"))

    def old_bn():
        ops.bn_bwd_reduce(go, None, c2, s2, t2, m2, i2, True, r2)
        ops.bn_bwd_apply_fin(go, None, c2, s2, t2, m2, i2, True, r2, npix, dg[0], dg[1], g_c2)

    def new_bn():
        ops.bn_bwd_frozen(go, None, c2, s2, t2, m2, i2, True, r2, g_c2)
    o, so, n, sn = ab(old_bn, new_bn)
    nbytes = tensor_bytes * 3
    say("bn   %4dx%-4d C=%-3d %-8s two-pass %7.1f (%.1f)  one-pass %7.1f (%.1f)  x%.2f  %5.2f TB/s (%.0f%% of 6.29)  %s"
        % (side, side, C, "", o, so, n, sn, o / n, nbytes / n * 1e-6, 100 * nbytes / n * 1e-6 / 6.29,
           "FASTER" if o - n > max(so, sn) else "NOT faster beyond the spread"))
    del go, c2, cb, g_c2, g_sc, mask

say("# whole step (forward, loss, backward, FlatAdam), ip16 512x512 batch %d bf16; ms per step: median (spread)" % B)
torch.manual_seed(1)
x, lab, wgt = [torch.from_numpy(t).cuda() for t in synthetic.make_batch(B, 512, 512, 1000)]
crit = PixelWiseNLLLoss()
steps = {}
for mode in ("train", "frozen"):
    m = UResNet(num_classes=3, input_channels=1, inplanes=16).cuda()
    m.compute_dtype = DT
    m.train()
    with torch.no_grad():
        for _ in range(2):
            m(x)                      # running statistics that normalise, before they are frozen
    if mode == "frozen":
        m.eval()
    opt = FlatAdam(m, lr=1e-5)

    def step(m=m, opt=opt):
        loss = crit(m(x), lab, wgt)
        opt.zero_grad()
        loss.backward()
        opt.step()
    steps[mode] = step
ITERS = 10
o, so, n, sn = ab(steps["train"], steps["frozen"])
say("train-mode step %.3f (%.3f) ms   frozen step %.3f (%.3f) ms   x%.3f" % (o * 1e-3, so * 1e-3, n * 1e-3, sn * 1e-3, o / n))
