#!/usr/bin/env python3
"""The guard of the BatchNorm running statistics (libubresnet_stats.so) against what a user could write with torch, alone on the
device and inside a train step, alternated in one process.

    python tools/statsbench.py [--launches N] [--reps R] [--steps S] [--no-train] [--inplanes 16,32] [--out FILE]

Kernel legs, on the table of UResNet inplanes 16 and 32 (every running_mean / running_var / num_batches_tracked): the launches
of StatsGuard.resolve() -- ubs_scan + ubs_note + ubs_decide + ubs_resolve -- on the keep branch (flag 1, clean statistics) and
on the restore branch (flag 0); the two launches of check_nonfinite=False (ubs_decide + ubs_resolve); and torch._foreach_copy_ of
the same tensors in a direction fixed in advance, live -> shadow and shadow -> live.  The torch legs are NOT the same operation:
the direction is chosen on the host before the call, so they cannot decide on the device and would need a host sync to do what
resolve() does; they are the nearest thing without the library that also avoids one.  A repetition is `--launches` back-to-back
calls of one leg between two device events; the legs alternate; median and spread (max - min) of the per-call time over `--reps`
repetitions.

Train-step legs: bf16 16 x 1 x 512 x 512, inplanes 16, FlatAdam(lr 1e-5, weight_decay 1e-4, max_grad_norm=1.0,
skip_nonfinite=True) without and with StatsGuard(model, optimizer=opt).resolve() after the step, two models from the same seed;
a repetition is `--steps` steps between two synchronisations, ms per step.  The leg without resolve() is the step as it was
before the library existed."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

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
    from ubresnet_amd import _stats as S
    from ubresnet_amd import synthetic
    from ubresnet_amd.bnguard import StatsGuard
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = ["# us per call, %d back-to-back calls between two device events; median (spread = max - min) over %d alternating "
             "repetitions.  The _foreach_copy_ legs move the same tensors in a direction fixed on the host: not the same operation, "
             "they cannot decide on the device" % (a.launches, a.reps)]
    for inplanes in [int(x) for x in a.inplanes.split(",")]:
        torch.manual_seed(inplanes)
        model = UResNet(num_classes=3, input_channels=1, inplanes=inplanes).to(dev)
        sg = StatsGuard(model)
        nseg, units = len(sg._rows), sg.shadow.numel()
        nf32 = sum(1 for _, _, k, _ in sg._rows if k == S.KIND_F32)
        table, bad, seen, ctl = sg._table.data_ptr(), sg.bad.data_ptr(), sg.seen.data_ptr(), sg.ctl.data_ptr()
        blk = torch.zeros(8, dtype=torch.int32, device=dev)                    # an optimizer's control block as far as ubs_decide looks
        flag = blk.data_ptr() + E.APPLY_OFFSET
        live = [b for _, b, _, _ in sg._rows]
        mine = [b.clone() for b in live]

        def four():
            S.scan(table, nseg, bad, stream)
            S.note(seen, bad, nseg, stream)
            S.decide(ctl, bad, nseg, flag, True, stream)
            S.resolve(table, nseg, ctl, stream)

        def two():
            S.decide(ctl, bad, nseg, flag, False, stream)
            S.resolve(table, nseg, ctl, stream)

        def set_flag(v):
            def f():
                blk[E.APPLY_OFFSET // 4] = v
                torch.cuda.synchronize()
            return f

        legs = {
            "scan+note+decide+resolve, keep": (set_flag(1), four),
            "scan+note+decide+resolve, restore": (set_flag(0), four),
            "decide+resolve, keep": (set_flag(1), two),
            "decide+resolve, restore": (set_flag(0), two),
            "_foreach_copy_ %d live->shadow" % nseg: (None, lambda: torch._foreach_copy_(mine, live)),
            "_foreach_copy_ %d shadow->live" % nseg: (None, lambda: torch._foreach_copy_(live, mine)),
        }
        times = {k: [] for k in legs}
        for pre, fn in legs.values():
            if pre is not None:
                pre()
            for _ in range(6):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, (pre, fn) in legs.items():
                if pre is not None:
                    pre()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        h = sg.read()
        lines.append("# inplanes %d: %d rows (%d fp32 rows scanned, %d raw rows of 2 units), %d units of 4 bytes = %d bytes of statistics; "
                     "table %d bytes; counters after the legs: kept %d restored %d" % (
                         inplanes, nseg, nf32, nseg - nf32, units, 4 * units, 32 * nseg, h["kept"], h["restored"]))
        md = {k: statistics.median(t) for k, t in times.items()}
        sp = {k: max(t) - min(t) for k, t in times.items()}
        for name in legs:
            t = times[name]
            lines.append("ip%-3d %-36s %8.2f us (spread %.2f)   runs: %s" % (inplanes, name, md[name], sp[name], " ".join("%.2f" % x for x in t)))
        names = list(legs)
        for mine_leg, torch_leg in ((names[0], names[4]), (names[1], names[5])):
            gap = md[mine_leg] - md[torch_leg]
            lines.append("ip%-3d %s - %s = %+.2f us against spreads %.2f + %.2f us: %s the two spreads (x%.2f)" % (
                inplanes, mine_leg, torch_leg, gap, sp[mine_leg], sp[torch_leg], "outside" if abs(gap) > sp[mine_leg] + sp[torch_leg] else "inside",
                md[mine_leg] / md[torch_leg]))
        gap = md[names[1]] - md[names[0]]
        lines.append("ip%-3d restore - keep = %+.2f us against spreads %.2f + %.2f us: %s the two spreads" % (
            inplanes, gap, sp[names[1]], sp[names[0]], "outside" if abs(gap) > sp[names[1]] + sp[names[0]] else "inside"))
        del model, sg, live, mine
    if not a.no_train:
        x, lab, wgt = synthetic.make_batch(B, H, W, seed0=1000)
        x, lab, wgt = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(wgt).to(dev)
        runs = {}
        for name in ("guarded", "guarded + resolve"):
            torch.manual_seed(1234)
            model = UResNet(num_classes=3, input_channels=1, inplanes=16).to(dev)
            model.compute_dtype = torch.bfloat16
            model.train()
            opt = FlatAdam(model, lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
            runs[name] = (model, opt, PixelWiseNLLLoss(), StatsGuard(model, optimizer=opt) if name.endswith("resolve") else None)

        def step(name):
            model, opt, crit, sg = runs[name]
            loss = crit.forward(model.forward(x), lab, wgt)
            opt.zero_grad()
            loss.backward()
            opt.step()
            if sg is not None:
                sg.resolve()
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
                     "median (spread) over %d alternating repetitions; the leg without resolve() is the step as it was" % (B, H, W, a.steps, a.reps))
        for name in runs:
            t = times[name]
            lines.append("train %-20s %8.3f ms (spread %.3f)   runs: %s" % (name, statistics.median(t), max(t) - min(t), " ".join("%.3f" % v for v in t)))
        h = runs["guarded + resolve"][3].read()
        g, r = times["guarded"], times["guarded + resolve"]
        gap = (statistics.median(r) - statistics.median(g)) * 1e3
        s0, s1 = (max(g) - min(g)) * 1e3, (max(r) - min(r)) * 1e3
        lines.append("# with resolve(): kept %d, restored %d; difference of the medians %+.1f us per step against spreads %.1f / %.1f us: %s the two spreads" % (
            h["kept"], h["restored"], gap, s0, s1, "outside" if abs(gap) > s0 + s1 else "inside"))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
