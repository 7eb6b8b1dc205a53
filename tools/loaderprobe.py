#!/usr/bin/env python3
"""The bf16 16 x 1 x 512 x 512 UResNet train step fed six ways, alternated in one process: ms per step, wall clock.

    python tools/loaderprobe.py [--steps N] [--reps R] [--out FILE]

  (a) resident    one batch resident in HBM, as bench.py times the step
  (b) device      synthetic.DeviceStager: loader call, float -> int64 on the host and three copies, on the training thread
  (c) batch-1     staging.BatchStager, threads=1
  (d) batch-2     staging.BatchStager, threads=2
  (e) epoch       leg (d) driven by training.epoch.train (adds the per-batch confusion matrix and the read-backs)
  (f) augment     leg (d) with augment=Augment(): uba_augment_batch in place of ubd_prep_batch behind the same copy

The loader is SyntheticLArCVDataset with cache >= nentries, filled before anything is timed: the crop generator is a stand-in
for the real input, its cost is kept out.  A leg runs `--steps` steps between two device synchronisations; median and spread
(max - min) over `--reps` alternating repetitions.  The legs run in a child process under a time limit; a failure ends the run.
For the BatchStager legs the producers' mean host time per batch is printed per stage: loader call (under the lock), slot
fill (wait for the slot's last copy + memcpy into the pinned slot), wait for a free slot (idle: the consumer is the bottleneck).
Leg (f) passes if its median is within the combined spread of legs (d) and (f) of leg (d)'s, measured in the same run.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, H, W, NENTRIES = 16, 512, 512, 64
LIMIT = 420                # seconds for the child
TARGET = 1.15              # legs (d) and (e) against leg (a)


def legs(a, say):
    import torch
    torch.set_num_threads(8)
    from ubresnet_amd import synthetic
    from ubresnet_amd.augment import Augment
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.staging import BatchStager
    from ubresnet_amd.training import epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = UResNet(num_classes=3, input_channels=1, inplanes=16).to(dev)
    model.compute_dtype = torch.bfloat16
    model.train()
    crit = PixelWiseNLLLoss()
    opt = FlatAdam(model, lr=1e-4, weight_decay=1e-4)

    def loader():
        ld = synthetic.SyntheticLArCVDataset(height=H, width=W, tag="train", nentries=NENTRIES, cache=NENTRIES)
        ld.start(B)
        for i in range(NENTRIES):
            ld._entry(i)                   # fill the cache: the generator never runs inside a timed step
        return ld

    def step(x, lab, wgt):
        out = model.forward(x)
        loss = crit.forward(out, lab, wgt)
        opt.zero_grad()
        loss.backward()
        opt.step()

    resident = tuple(torch.from_numpy(t).to(dev) for t in synthetic.make_batch(B, H, W, 1000))
    old = synthetic.DeviceStager(loader(), B, H, W, tag="train")
    st = {1: BatchStager(loader(), B, H, W, tag="train", threads=1), 2: BatchStager(loader(), B, H, W, tag="train", threads=2),
          "e": BatchStager(loader(), B, H, W, tag="train", threads=2),
          "f": BatchStager(loader(), B, H, W, tag="train", threads=2, augment=Augment())}

    def run(leg, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if leg == "a":
            for _ in range(n):
                step(*resident)
        elif leg == "b":
            for _ in range(n):
                step(*old.next())
        elif leg in ("c", "d", "f"):
            s = st[{"c": 1, "d": 2, "f": "f"}[leg]]
            for _ in range(n):
                step(*s.next())
        else:
            epoch.train(st["e"], model, crit, opt, n, print_freq=10, log=lambda s: None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    names = {"a": "resident batch", "b": "DeviceStager", "c": "BatchStager threads=1", "d": "BatchStager threads=2",
             "e": "epoch.train over (d)", "f": "(d) with Augment()"}
    for leg in names:
        run(leg, 4)                        # warm-up: kernel selection, pinned slots, allocator
    runs = {leg: [] for leg in names}
    for _ in range(a.reps):
        for leg in names:                  # alternating
            runs[leg].append(run(leg, a.steps))
    crit.flush()
    say("# UResNet ip16 nc3 bf16 train step, batch %d x 1 x %d x %d, FlatAdam; loader: SyntheticLArCVDataset, %d entries, all cached"
        % (B, H, W, NENTRIES))
    say("# ms per step, wall clock over %d steps between two synchronisations: median (spread = max - min) over %d alternating repetitions"
        % (a.steps, a.reps))
    med = {}
    for leg, name in names.items():
        r = runs[leg]
        med[leg] = statistics.median(r)
        say("(%s) %-24s %7.2f ms (spread %.2f)  x%.3f of (a)   runs: %s"
            % (leg, name, med[leg], max(r) - min(r), med[leg] / med["a"], " ".join("%.2f" % x for x in r)))
    say("# producers' host time per batch, mean ms (batches): loader call | slot fill | wait for a free slot")
    stage = {}
    for leg, key in (("c", 1), ("d", 2), ("e", "e"), ("f", "f")):
        t = stage[leg] = st[key].stage_times()
        say("(%s) loader %.2f (%d) | fill %.2f (%d) | wait_slot %.2f (%d)" % (
            leg, t["loader"][0], t["loader"][1], t["fill"][0], t["fill"][1], t["wait_slot"][0], t["wait_slot"][1]))
    for s in st.values():
        s.close()
    for leg in ("d", "e"):
        ratio = med[leg] / med["a"]
        if ratio <= TARGET:
            say("target (%s) <= %.2f x (a): MET at x%.3f" % (leg, TARGET, ratio))
        else:
            t = stage[leg]
            serial = t["loader"][0] + t["fill"][0]          # one producer's busy time per batch; the loader call is serial across producers
            bound = max(t["loader"][0], serial / 2.0)
            say("target (%s) <= %.2f x (a): MISSED at x%.3f (%.2f ms over the %.2f ms step); producers need max(loader, (loader + fill) / 2) = "
                "%.2f ms per batch: %s bounds the loop" % (leg, TARGET, ratio, med[leg] - med["a"], med["a"], bound,
                                                          "the loader call" if t["loader"][0] >= serial / 2.0 else "the slot fill"))


    spread = {leg: max(runs[leg]) - min(runs[leg]) for leg in ("d", "f")}
    delta, allowed = med["f"] - med["d"], spread["d"] + spread["f"]
    if abs(delta) <= allowed:
        say("augment (f) against (d): %+.2f ms, within the two legs' combined spread of %.2f ms: PASSED" % (delta, allowed))
    else:
        t = stage["f"]
        say("augment (f) against (d): %+.2f ms, outside the two legs' combined spread of %.2f ms: %s; producers of (f): loader %.2f | "
            "fill %.2f | wait_slot %.2f ms per batch" % (delta, allowed, "FASTER" if delta < 0 else "MISSED", t["loader"][0], t["fill"][0],
                                                         t["wait_slot"][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="run the legs in this process (what the driver starts)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least five repetitions per leg")
    if a.child:
        legs(a, lambda s: print(s, flush=True))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--reps", str(a.reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
        text, rc = r.stdout, r.returncode
        if rc != 0:
            text += "# the legs FAILED (exit %d)\n%s" % (rc, r.stderr[-2000:])
    except subprocess.TimeoutExpired as e:
        so = e.stdout.decode("utf-8", "replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        text, rc = so + "# the legs ran out of their %d s\n" % LIMIT, 124
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
