#!/usr/bin/env python3
"""The grouped optimizer step against the ungrouped guarded one, alone on the device and inside a train step, alternated in one
process.

    python tools/groupbench.py [--launches N] [--reps R] [--steps S] [--no-train] [--inplanes 16,32] [--legs TEXT,..] [--out FILE]

Kernel legs, at the flat gradient sizes of UResNet inplanes 16 and 32 (Engine.grad_numel): ubo_adam_step (the yardstick);
ubg_adam_step with ONE segment over the whole buffer; with the network's own segments (one per parameter) in three groups, all
active; the same with the encoder half inactive; ubo_grad_norm (the yardstick) and ubg_grad_norm over the network's segments, all
active and half inactive.  A repetition is `--launches` back-to-back calls of one leg between two device events; the legs
alternate; median and spread (max - min) of the per-call time over `--reps` repetitions.  An Adam step reads 16 and writes 12
bytes per ACTIVE element, the norm pass reads 4; the byte bound is those bytes at 6 TB/s, and the achieved rate is those bytes
over the median.

Train-step legs: bf16 16 x 1 x 512 x 512, inplanes 16, FlatAdam(lr 1e-5, weight_decay 1e-4, max_grad_norm=1.0,
skip_nonfinite=True) plain and with two groups (encoder at a tenth of the learning rate), two models from the same seed; a
repetition is `--steps` steps between two synchronisations, ms per step.

For a kernel trace in which every kernel name stands for ONE configuration, restrict the run (profiles/README.md has the command):
`--inplanes 16 --legs "ubo_adam_step,ubg_adam 165" --no-train` times those two legs only (a leg is kept if its name contains one of
the texts)."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM = 6.0e12
B, H, W = 16, 512, 512
ENC = ("conv1.", "bn1.", "enc_")          # with the dots: conv10, conv11 and bn10 are the head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--inplanes", default="16,32")
    ap.add_argument("--legs", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from ubresnet_amd import _group as G
    from ubresnet_amd import _opt as O
    from ubresnet_amd import synthetic
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = ["# us per call, %d back-to-back calls between two device events; median (spread = max - min) over %d alternating "
             "repetitions; byte bound at 6 TB/s; 28 B per active float for Adam, 4 for the norm" % (a.launches, a.reps)]
    table = torch.from_numpy(O.bias_table(0.9, 0.999)).to(dev)
    hyp = (1e-5, 0.9, 0.999, 1e-8, 1e-4)

    def upload(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(dev)

    class Plan(object):
        """tile table, hyper, state and control block of a segment list; every segment has 100 steps behind it"""

        def __init__(self, unit0, units, group, active):
            tiles = G.plan_tiles(unit0, units)
            self.nseg, self.ntiles = len(units), len(tiles)
            self.tiles = upload(tiles)
            h = np.zeros(self.nseg, dtype=G.HYPER)
            h["lr"] = [(1e-5, 1e-6, 3e-6)[k] for k in group]
            h["weight_decay"] = [(1e-4, 0.0, 1e-5)[k] for k in group]
            h["active"] = [1 if x else 0 for x in active]
            self.hyper = upload(h)
            self.state = torch.zeros(16 * self.nseg, dtype=torch.uint8, device=dev)
            self.ctl = torch.zeros(G.CTL_BYTES, dtype=torch.uint8, device=dev)
            counts = torch.full((self.nseg,), 100, dtype=torch.int64, device=dev)
            G.state_set(self.state.data_ptr(), self.nseg, 0, self.nseg, counts.data_ptr(), table.data_ptr(), table.shape[0], stream)
            torch.cuda.synchronize()
            self.active_floats = 4 * sum(u for u, x in zip(units, active) if x)

        def norm(self, grad, n):
            G.grad_norm(grad.data_ptr(), n, self.tiles.data_ptr(), self.ntiles, self.hyper.data_ptr(), self.state.data_ptr(), self.nseg, 1.0, 1.0,
                        True, table.data_ptr(), table.shape[0], self.ctl.data_ptr(), stream)

        def adam(self, ptrs, n):
            G.adam_step(*ptrs, n, self.tiles.data_ptr(), self.ntiles, self.hyper.data_ptr(), self.state.data_ptr(), self.nseg, 0.9, 0.999, 1e-8,
                        self.ctl.data_ptr(), stream)

    for inplanes in [int(x) for x in a.inplanes.split(",")]:
        model = UResNet(num_classes=3, input_channels=1, inplanes=inplanes).to(dev)
        opt = FlatAdam(model, lr=1e-5)
        n = opt._numel
        layout = [(name, o // 4, (p.numel() + 3) // 4) for name, p, o in opt._layout]
        del model, opt
        g = torch.Generator(device=dev).manual_seed(inplanes)
        p, grad = torch.randn(n, generator=g, device=dev), torch.randn(n, generator=g, device=dev) * 1e-3
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        ctl = torch.zeros(O.CTL_BYTES, dtype=torch.uint8, device=dev)
        O.ctl_init(ctl.data_ptr(), 0, stream)
        ptrs = (p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr())
        unit0, units = [u for _, u, _ in layout], [c for _, _, c in layout]
        is_enc = [name.startswith(ENC) for name, _, _ in layout]
        one = Plan([0], [n // 4], [0], [True])
        net = Plan(unit0, units, [k % 3 for k in range(len(units))], [True] * len(units))
        half = Plan(unit0, units, [k % 3 for k in range(len(units))], [not e for e in is_enc])
        for pl in (one, net, half):
            pl.norm(grad, n)                          # the blocks say apply = 1 before a step runs alone
        O.grad_norm(grad.data_ptr(), n, 1.0, 1.0, True, table.data_ptr(), table.shape[0], ctl.data_ptr(), stream)
        legs = {
            "ubo_adam_step": (lambda: O.adam_step(*ptrs, n, *hyp, ctl.data_ptr(), stream), 28 * n),
            "ubg_adam 1 segment": (lambda: one.adam(ptrs, n), 28 * one.active_floats),
            "ubg_adam %d seg" % net.nseg: (lambda: net.adam(ptrs, n), 28 * net.active_floats),
            "ubg_adam enc off": (lambda: half.adam(ptrs, n), 28 * half.active_floats),
            "ubo_grad_norm": (lambda: O.grad_norm(grad.data_ptr(), n, 1.0, 1.0, True, table.data_ptr(), table.shape[0], ctl.data_ptr(), stream), 4 * n),
            "ubg_norm %d seg" % net.nseg: (lambda: net.norm(grad, n), 4 * net.active_floats),
            "ubg_norm enc off": (lambda: half.norm(grad, n), 4 * half.active_floats),
        }
        if a.legs:
            legs = {k: v for k, v in legs.items() if any(t.strip() in k for t in a.legs.split(","))}
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
        lines.append("# inplanes %d: n = %d floats (%.1f MB) in %d segments, %d tiles; encoder segments hold %.1f%% of the floats" % (
            inplanes, n, 4 * n / 1e6, net.nseg, net.ntiles, 100.0 * (1 - half.active_floats / net.active_floats)))
        for name, (_, nbytes) in legs.items():
            t = times[name]
            med = statistics.median(t)
            lines.append("ip%-3d %-20s %8.2f us (spread %.2f)   %6.1f MB   bound %6.2f us   x%.2f of the bound   %5.2f TB/s   runs: %s" % (
                inplanes, name, med, max(t) - min(t), nbytes / 1e6, nbytes / HBM * 1e6, med / (nbytes / HBM * 1e6), nbytes / med / 1e6,
                " ".join("%.2f" % x for x in t)))
        if a.legs:
            del p, grad, m, v
            continue
        md = {k: statistics.median(t) for k, t in times.items()}
        sp = {k: max(t) - min(t) for k, t in times.items()}
        k1, kn, kh = "ubg_adam 1 segment", "ubg_adam %d seg" % net.nseg, "ubg_adam enc off"
        lines.append("ip%-3d ratios to ubo_adam_step: 1 segment x%.3f, %d segments x%.3f, encoder off x%.3f (active floats x%.3f); "
                     "difference %d segments - ubo %.2f us against spreads %.2f / %.2f us" % (
                         inplanes, md[k1] / md["ubo_adam_step"], net.nseg, md[kn] / md["ubo_adam_step"], md[kh] / md["ubo_adam_step"],
                         half.active_floats / net.active_floats, net.nseg, md[kn] - md["ubo_adam_step"], sp[kn], sp["ubo_adam_step"]))
        lines.append("ip%-3d ratios to ubo_grad_norm: %d segments x%.3f, encoder off x%.3f" % (
            inplanes, net.nseg, md["ubg_norm %d seg" % net.nseg] / md["ubo_grad_norm"], md["ubg_norm enc off"] / md["ubo_grad_norm"]))
        del p, grad, m, v
    if not a.no_train:
        x, lab, wgt = synthetic.make_batch(B, H, W, seed0=1000)
        x, lab, wgt = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(wgt).to(dev)
        runs = {}
        for name in ("plain guarded", "grouped guarded"):
            torch.manual_seed(1234)
            model = UResNet(num_classes=3, input_channels=1, inplanes=16).to(dev)
            model.compute_dtype = torch.bfloat16
            model.train()
            kw = {}
            if name.startswith("grouped"):
                kw["groups"] = [{"params": [q for k, q in model.named_parameters() if k.startswith(ENC)], "lr": 1e-6},
                                {"params": [q for k, q in model.named_parameters() if not k.startswith(ENC)]}]
            runs[name] = (model, FlatAdam(model, lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True, **kw), PixelWiseNLLLoss())

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
        lines.append("# train step, bf16 %d x 1 x %d x %d, inplanes 16, guarded FlatAdam; ms per step, %d steps between two synchronisations; "
                     "median (spread) over %d alternating repetitions" % (B, H, W, a.steps, a.reps))
        for name in runs:
            t = times[name]
            lines.append("train %-16s %8.3f ms (spread %.3f)   runs: %s" % (name, statistics.median(t), max(t) - min(t), " ".join("%.3f" % v for v in t)))
        r = runs["grouped guarded"][1].guard.read()
        lines.append("# grouped: last norm %.3e, scale %.3e, applied %d, skipped %d, clipped %d; difference of the medians %.1f us per step" % (
            r["norm"], r["scale"], r["applied"], r["skipped"], r["clipped_total"],
            (statistics.median(times["grouped guarded"]) - statistics.median(times["plain guarded"])) * 1e3))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
