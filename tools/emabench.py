#!/usr/bin/env python3
"""The device-side parameter average (libubresnet_ema.so) against what a user would write with torch, alone on the device and
inside a train step, alternated in one process.

    python tools/emabench.py [--launches N] [--reps R] [--steps S] [--no-train] [--inplanes 16,32] [--out FILE]

Kernel legs, on the flat parameter buffer of UResNet inplanes 16 and 32 and on its 104 BatchNorm statistics tensors:
ube_advance + ube_update (the flat pair of ParamEMA.update()); the same plus ube_update_segs (buffers="average"); ube_swap (what
entering or leaving applied() costs); torch._foreach_lerp_ over the 165 parameter views plus the 104 statistics tensors against
separately allocated shadows -- what a user writes without the library.  A repetition is `--launches` back-to-back calls of one
leg between two device events; the legs alternate; median and spread (max - min) of the per-call time over `--reps`
repetitions.  An update reads the parameter and the average and writes the average, 12 bytes per float; a swap reads and writes
both, 16; the byte bound is those bytes at 6 TB/s.  (At inplanes 16 the two buffers together are 145 MB and stay in the 256 MiB
last-level cache from call to call, so a leg can run under its HBM bound.)

Train-step legs: bf16 16 x 1 x 512 x 512, inplanes 16, FlatAdam(lr 1e-5, weight_decay 1e-4, max_grad_norm=1.0,
skip_nonfinite=True) without and with ParamEMA(decay 0.999, warmup 10, buffers="average").update() after the step, two models
from the same seed; a repetition is `--steps` steps between two synchronisations, ms per step."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM = 6.0e12
B, H, W = 16, 512, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--inplanes", default="16,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ubresnet_amd import _ema as E
    from ubresnet_amd import synthetic
    from ubresnet_amd.ema import ParamEMA
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = ["# us per call, %d back-to-back calls between two device events; median (spread = max - min) over %d alternating "
             "repetitions; byte bound at 6 TB/s; 12 B per float for an update, 16 for a swap" % (a.launches, a.reps)]
    verdicts = []
    for inplanes in [int(x) for x in a.inplanes.split(",")]:
        torch.manual_seed(inplanes)
        model = UResNet(num_classes=3, input_channels=1, inplanes=inplanes).to(dev)
        opt = FlatAdam(model, lr=1e-5)
        ema = ParamEMA(opt, decay=0.999, warmup=10, buffers="average")
        n, nstat, nseg = opt.flat.numel(), ema.stats.numel(), len(ema._stats)
        opt.flat.add_(torch.randn_like(opt.flat) * 1e-3)                       # the average and the weights differ
        ctl, shadow, flat, table = ema.ctl.data_ptr(), ema.shadow.data_ptr(), opt.flat.data_ptr(), ema._table.data_ptr()
        # the torch way: one shadow tensor per parameter and per statistics tensor, one multi-tensor call
        live = [p.detach() for _, p, _ in opt._layout] + [b for _, b, _ in ema._stats]
        mine = [t.clone() for t in live]

        def pair():
            E.advance(ctl, None, 0.999, 10, stream)
            E.update(shadow, flat, n, ctl, stream)

        def triple():
            pair()
            E.update_segs(table, nseg, ctl, stream)

        legs = {
            "ube_advance+update": (pair, 12 * n),
            "  + ube_update_segs": (triple, 12 * (n + nstat)),
            "ube_swap": (lambda: E.swap(shadow, flat, n, stream), 16 * n),
            "_foreach_lerp_ %d" % len(live): (lambda: torch._foreach_lerp_(mine, live, 0.001), 12 * (n + nstat)),
        }
        times = {k: [] for k in legs}
        for fn, _ in legs.values():
            for _ in range(6):                                                # (an even count: the swap leg ends where it began)
                fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, (fn, _) in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        lines.append("# inplanes %d: n = %d floats (%.1f MB) in %d parameters; %d statistics tensors of %d floats in all" % (
            inplanes, n, 4 * n / 1e6, len(opt._layout), nseg, nstat))
        for name, (_, nbytes) in legs.items():
            t = times[name]
            med = statistics.median(t)
            lines.append("ip%-3d %-22s %8.2f us (spread %.2f)   %6.1f MB   bound %6.2f us   x%.2f of the bound   %5.2f TB/s   runs: %s" % (
                inplanes, name, med, max(t) - min(t), nbytes / 1e6, nbytes / HBM * 1e6, med / (nbytes / HBM * 1e6), nbytes / med / 1e6,
                " ".join("%.2f" % x for x in t)))
        md = {k: statistics.median(t) for k, t in times.items()}
        sp = {k: max(t) - min(t) for k, t in times.items()}
        kp, kt, kf = "ube_advance+update", "  + ube_update_segs", "_foreach_lerp_ %d" % len(live)
        gap = md[kf] - md[kp]
        beats = gap > sp[kf] + sp[kp]
        verdicts.append(beats)
        lines.append("ip%-3d _foreach_lerp_ - flat pair = %.2f us against spreads %.2f + %.2f us: the flat pair %s; _foreach_lerp_ is x%.2f of "
                     "the flat pair and x%.2f of the pair with the statistics; the statistics launch adds %.2f us" % (
                         inplanes, gap, sp[kf], sp[kp], "beats it by more than the two spreads" if beats else "does NOT beat it by more than the two spreads",
                         md[kf] / md[kp], md[kf] / md[kt], md[kt] - md[kp]))
        del model, opt, ema, live, mine
    if not a.no_train:
        x, lab, wgt = synthetic.make_batch(B, H, W, seed0=1000)
        x, lab, wgt = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(wgt).to(dev)
        runs = {}
        for name in ("guarded", "guarded + ema"):
            torch.manual_seed(1234)
            model = UResNet(num_classes=3, input_channels=1, inplanes=16).to(dev)
            model.compute_dtype = torch.bfloat16
            model.train()
            opt = FlatAdam(model, lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
            runs[name] = (model, opt, PixelWiseNLLLoss(), ParamEMA(opt, decay=0.999, warmup=10, buffers="average") if name.endswith("ema") else None)

        def step(name):
            model, opt, crit, ema = runs[name]
            loss = crit.forward(model.forward(x), lab, wgt)
            opt.zero_grad()
            loss.backward()
            opt.step()
            if ema is not None:
                ema.update()
        for name in runs:
            for _ in range(5):
                step(name)
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.reps):
            for name in runs:
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(name)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
        lines.append("# train step, bf16 %d x 1 x %d x %d, inplanes 16, guarded FlatAdam; ms per step, %d steps between two synchronisations; "
                     "median (spread) over %d alternating repetitions" % (B, H, W, a.steps, a.reps))
        for name in runs:
            t = times[name]
            lines.append("train %-16s %8.3f ms (spread %.3f)   runs: %s" % (name, statistics.median(t), max(t) - min(t), " ".join("%.3f" % v for v in t)))
        ema = runs["guarded + ema"][3]
        lines.append("# with ema: updates %d, held %d; difference of the medians %.1f us per step against spreads %.1f / %.1f us" % (
            ema.updates, ema.held, (statistics.median(times["guarded + ema"]) - statistics.median(times["guarded"])) * 1e3,
            (max(times["guarded"]) - min(times["guarded"])) * 1e3, (max(times["guarded + ema"]) - min(times["guarded + ema"])) * 1e3))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
