#!/usr/bin/env python3
"""The guarded optimizer step against the plain one, alone on the device and inside a train step, alternated in one process.

    python tools/guardbench.py [--launches N] [--reps R] [--steps S] [--out FILE]

Kernel legs, at the flat gradient sizes of UResNet inplanes 16 and 32 (Engine.grad_numel): ubr_adam_step, ubo_adam_step alone,
ubo_grad_norm alone (its two launches), and the pair.  A repetition is `--launches` back-to-back calls of one leg between two
device events; the legs alternate; median and spread (max - min) of the per-call time over `--reps` repetitions.  An Adam step
reads 16 and writes 12 bytes per element; the norm pass reads 4.  The byte bound is those bytes at 6 TB/s.

Train-step legs: bf16 16 x 1 x 512 x 512, inplanes 16, FlatAdam(lr 1e-5, weight_decay 1e-4) unguarded and guarded
(max_grad_norm=1.0, skip_nonfinite=True), two models from the same seed; a repetition is `--steps` steps between two
synchronisations, ms per step."""
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _opt as O
    from ubresnet_amd import synthetic
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = ["# us per call, %d back-to-back calls between two device events; median (spread = max - min) over %d alternating "
             "repetitions; byte bound at 6 TB/s" % (a.launches, a.reps)]
    table = torch.from_numpy(O.bias_table(0.9, 0.999)).to(dev)
    hyp = (1e-5, 0.9, 0.999, 1e-8, 1e-4)
    for inplanes in (16, 32):
        model = UResNet(num_classes=3, input_channels=1, inplanes=inplanes).to(dev)
        n = FlatAdam(model, lr=1e-5)._numel
        del model
        g = torch.Generator(device=dev).manual_seed(inplanes)
        p, grad = torch.randn(n, generator=g, device=dev), torch.randn(n, generator=g, device=dev) * 1e-3
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        ctl = torch.zeros(O.CTL_BYTES, dtype=torch.uint8, device=dev)
        O.ctl_init(ctl.data_ptr(), 0, stream)
        ptrs = (p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr())

        def plain():
            L.check(L.lib().ubr_adam_step(*ptrs, n, *hyp, 100, 1.0, stream), "adam_step")

        def guarded():
            O.adam_step(*ptrs, n, *hyp, ctl.data_ptr(), stream)

        def norm():
            O.grad_norm(grad.data_ptr(), n, 1.0, 1.0, True, table.data_ptr(), table.shape[0], ctl.data_ptr(), stream)

        def pair():
            norm()
            guarded()
        legs = {"ubr_adam_step": (plain, 28), "ubo_adam_step": (guarded, 28), "ubo_grad_norm": (norm, 4), "norm + step": (pair, 32)}
        norm()                                        # the block says apply = 1 before ubo_adam_step runs alone
        times = {k: [] for k in legs}
        for fn, _ in legs.values():
            for _ in range(5):
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
        h = O.read_ctl(ctl[:O.CTL_HEAD_BYTES].cpu().numpy().tobytes())
        lines.append("# inplanes %d: n = %d floats (%.1f MB); block after the run: applied %d skipped %d" % (inplanes, n, 4 * n / 1e6, h.applied, h.skipped))
        for name, (_, bytes_per) in legs.items():
            t = times[name]
            bound = bytes_per * n / HBM * 1e6
            lines.append("ip%-3d %-14s %8.2f us (spread %.2f)   %6.1f MB   bound %6.2f us   x%.2f of the bound   runs: %s" % (
                inplanes, name, statistics.median(t), max(t) - min(t), bytes_per * n / 1e6, bound, statistics.median(t) / bound,
                " ".join("%.2f" % x for x in t)))
        del p, grad, m, v
    if not a.no_train:
        x, lab, wgt = synthetic.make_batch(B, H, W, seed0=1000)
        x, lab, wgt = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(wgt).to(dev)
        runs = {}
        for name, kw in (("unguarded", {}), ("guarded", dict(max_grad_norm=1.0, skip_nonfinite=True))):
            torch.manual_seed(1234)
            model = UResNet(num_classes=3, input_channels=1, inplanes=16).to(dev)
            model.compute_dtype = torch.bfloat16
            model.train()
            runs[name] = (model, FlatAdam(model, lr=1e-5, weight_decay=1e-4, **kw), PixelWiseNLLLoss())

        def step(name):
            model, opt, crit = runs[name]
            loss = crit.forward(model.forward(x), lab, wgt)
            opt.zero_grad()
            loss.backward()
            opt.step()
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
        lines.append("# train step, bf16 %d x 1 x %d x %d, inplanes 16, FlatAdam; ms per step, %d steps between two synchronisations; "
                     "median (spread) over %d alternating repetitions" % (B, H, W, a.steps, a.reps))
        for name in runs:
            t = times[name]
            lines.append("train %-10s %8.3f ms (spread %.3f)   runs: %s" % (name, statistics.median(t), max(t) - min(t), " ".join("%.3f" % v for v in t)))
        r = runs["guarded"][1].guard.read()
        lines.append("# guarded: last norm %.3e, scale %.3e, applied %d, skipped %d, clipped %d; difference of the medians %.1f us per step" % (
            r["norm"], r["scale"], r["applied"], r["skipped"], r["clipped_total"],
            (statistics.median(times["guarded"]) - statistics.median(times["unguarded"])) * 1e3))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
