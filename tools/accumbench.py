#!/usr/bin/env python3
"""Gradient accumulation on the device (libubresnet_accum.so, ubresnet_amd.accum.GradAccumulator) against what a user would write
with torch and against the package's legacy accumulating backward, alternated in one process.

    python tools/accumbench.py [--launches N] [--reps R] [--steps S] [--no-train] [--inplanes 16,32] [--out FILE]

(a) Kernel legs, on flat buffers of the gradient size of UResNet inplanes 16 and 32: ubc_set, ubc_add, ubc_finish; the torch
one-liners `acc.copy_(g)`, `acc.add_(g)`, `torch.add(acc, g, out=g).mul_(s)`; and ube_update of libubresnet_ema.so, which moves the
same 12 B per float as ubc_add with the other lane-to-unit mapping.  A repetition is `--launches` back-to-back calls of one leg
between two device events; the legs alternate; median and spread (max - min) of the per-call time over `--reps` repetitions.
Byte bound: 8 B per float (set) or 12 (add, finish) at 6 TB/s.  (At inplanes 16 the two buffers together are 145 MB and stay in
the 256 MiB last-level cache from call to call, so a leg can run under its HBM bound.)

(b) One optimizer step of K = 4 micro-batches of 4 x 1 x 512 x 512, bf16, inplanes 16, guarded FlatAdam, three ways: through
GradAccumulator (zero_grad between the passes: four replayed passes and three kernels); the legacy path (no zero_grad between
the passes: passes 2 to 4 are scheduled from Python into a fresh buffer and added with one add_ per parameter); and, for scale,
four plain replayed passes with zero_grad between them and no accumulation at all.  ms per optimizer step.

(c) The bf16 16 x 1 x 512 x 512 guarded train step without any accumulator: the default path."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM = 6.0e12
H, W, K, MICRO, FULL = 512, 512, 4, 4, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--inplanes", default="16,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from ubresnet_amd import _accum as A
    from ubresnet_amd import _ema as E
    from ubresnet_amd import synthetic
    from ubresnet_amd.accum import GradAccumulator
    from ubresnet_amd.autograd_fn import _engine
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = ["# (a) us per call, %d back-to-back calls between two device events; median (spread = max - min) over %d alternating "
             "repetitions; byte bound at 6 TB/s; 8 B per float for a set, 12 for an add or a finish" % (a.launches, a.reps)]
    scale = float(np.float32(0.25))
    for inplanes in [int(x) for x in a.inplanes.split(",")]:
        model = UResNet(num_classes=3, input_channels=1, inplanes=inplanes).to(dev)
        n = _engine(model, "uresnet").grad_numel
        del model
        acc = torch.randn(n, device=dev) * 1e-3
        g = torch.randn(n, device=dev) * 1e-3
        ctl = torch.zeros(E.CTL_BYTES, dtype=torch.uint8, device=dev)
        E.ctl_init(ctl.data_ptr(), 0, stream)
        E.advance(ctl.data_ptr(), None, 0.999, 0, stream)                      # apply = 1, w = 0.001: ube_update acts on every call
        pa, pg, pc = acc.data_ptr(), g.data_ptr(), ctl.data_ptr()
        legs = {
            "ubc_set": (lambda: A.set_(pa, pg, n, stream), 8 * n),
            "torch acc.copy_(g)": (lambda: acc.copy_(g), 8 * n),
            "ubc_add": (lambda: A.add(pa, pg, n, stream), 12 * n),
            "torch acc.add_(g)": (lambda: acc.add_(g), 12 * n),
            "ube_update (ema lib)": (lambda: E.update(pa, pg, n, pc, stream), 12 * n),
            "ubc_finish": (lambda: A.finish(pg, pa, n, scale, stream), 12 * n),
            "torch add(out=g).mul_": (lambda: torch.add(acc, g, out=g).mul_(scale), 20 * n),
        }
        times = {k: [] for k in legs}
        for fn, _ in legs.values():
            for _ in range(5):
                fn()
            g.normal_().mul_(1e-3)                                             # (finish scales g down call after call: keep it ordinary)
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
                acc.normal_().mul_(1e-3)
                g.normal_().mul_(1e-3)
        lines.append("# inplanes %d: n = %d floats (%.1f MB per buffer)" % (inplanes, n, 4 * n / 1e6))
        for name, (_, nbytes) in legs.items():
            t = times[name]
            med = statistics.median(t)
            note = "   (two launches, 20 B per float as written)" if name.startswith("torch add(") else ""
            lines.append("ip%-3d %-24s %8.2f us (spread %.2f)   %6.1f MB   bound %6.2f us   x%.2f of the bound   %5.2f TB/s   runs: %s%s" % (
                inplanes, name, med, max(t) - min(t), nbytes / 1e6, nbytes / HBM * 1e6, med / (nbytes / HBM * 1e6), nbytes / med / 1e6,
                " ".join("%.2f" % x for x in t), note))
        del acc, g
    if not a.no_train:
        hyp = dict(lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)

        def make(batch):
            torch.manual_seed(1234)
            model = UResNet(num_classes=3, input_channels=1, inplanes=16).to(dev)
            model.compute_dtype = torch.bfloat16
            model.train()
            data = []
            for k in range(K):
                x, lab, wgt = synthetic.make_batch(batch, H, W, seed0=1000 + 100 * k)
                data.append((torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(wgt).to(dev)))
            return model, FlatAdam(model, **hyp), PixelWiseNLLLoss(), data

        runs = {name: make(MICRO) for name in ("GradAccumulator", "legacy path", "no accumulation")}
        accs = {"GradAccumulator": GradAccumulator(runs["GradAccumulator"][0], every=K)}

        def step(name):
            model, opt, crit, data = runs[name]
            if name == "legacy path":
                opt.zero_grad()
                for x, lab, wgt in data:
                    crit.forward(model.forward(x), lab, wgt).backward()       # passes 2..K add into the existing .grad tensors
                opt.step()
                return
            acc = accs.get(name)
            for x, lab, wgt in data:
                loss = crit.forward(model.forward(x), lab, wgt)
                opt.zero_grad()
                loss.backward()
                if acc is not None:
                    acc.add()
            opt.step()

        def measure(runs_, step_, steps):
            for name in runs_:
                for _ in range(3):
                    step_(name)
            torch.cuda.synchronize()
            times = {k: [] for k in runs_}
            for _ in range(a.reps):
                for name in runs_:
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        step_(name)
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1e3 / steps)
            return times
        times = measure(runs, step, a.steps)
        lines.append("# (b) one optimizer step of K = %d micro-batches of %d x 1 x %d x %d, bf16, inplanes 16, guarded FlatAdam; ms per optimizer "
                     "step, %d steps between two synchronisations; median (spread) over %d alternating repetitions" % (K, MICRO, H, W, a.steps, a.reps))
        for name in runs:
            t = times[name]
            lines.append("accum %-16s %8.3f ms (spread %.3f)   runs: %s" % (name, statistics.median(t), max(t) - min(t), " ".join("%.3f" % v for v in t)))
        md = {k: statistics.median(t) for k, t in times.items()}
        sp = {k: max(t) - min(t) for k, t in times.items()}
        lines.append("# GradAccumulator - no accumulation = %.1f us per optimizer step (spreads %.1f / %.1f us): the expectation is the three "
                     "kernels of (a) at ip16; legacy path - GradAccumulator = %.3f ms (spreads %.3f / %.3f ms): x%.2f" % (
                         (md["GradAccumulator"] - md["no accumulation"]) * 1e3, sp["GradAccumulator"] * 1e3, sp["no accumulation"] * 1e3,
                         md["legacy path"] - md["GradAccumulator"], sp["legacy path"], sp["GradAccumulator"], md["legacy path"] / md["GradAccumulator"]))
        del runs, accs
        full = {"guarded": make(FULL)}

        def fstep(name):
            model, opt, crit, data = full[name]
            x, lab, wgt = data[0]
            loss = crit.forward(model.forward(x), lab, wgt)
            opt.zero_grad()
            loss.backward()
            opt.step()
        t = measure(full, fstep, 2 * a.steps)["guarded"]
        lines.append("# (c) train step, bf16 %d x 1 x %d x %d, inplanes 16, guarded FlatAdam, no accumulator; ms per step" % (FULL, H, W))
        lines.append("train %-16s %8.3f ms (spread %.3f)   runs: %s" % ("guarded", statistics.median(t), max(t) - min(t), " ".join("%.3f" % v for v in t)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
