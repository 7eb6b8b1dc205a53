#!/usr/bin/env python3
"""ubw_pixel_weights on the device, the same weights made with numpy on host threads, and the train step with and without
generated weights, in one process with the legs alternated.

    python tools/weightbench.py [--launches N] [--reps R] [--steps S] [--no-train] [--out FILE]

(a) A repetition is `--launches` back-to-back ubw_pixel_weights calls (memset, count pass, apply pass) between two device
    events, at 16 x 512 x 512 and 16 x 512 x 832 for r = 0, 1, 4; the legs alternate; median and spread (max - min) of the
    per-call time over `--reps` repetitions.  The byte bound is 8 B/pixel read by the count pass plus 8 B/pixel read and
    4 B/pixel written by the apply pass, at 6 TB/s.
(b) The numpy reference of tests/weights_ref.py on the same labels, one image per thread on 16 host threads, wall clock.
(c) The bf16 16 x 1 x 512 x 512 train step fed through BatchStager from a loader without a weight entry, `--steps` steps per
    repetition between two host clock readings that end in a device synchronise, weights=None (all ones) against
    PixelWeights(radius=1, gain=2), alternated."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

B = 16
SHAPES = [(512, 512), (512, 832)]
RADII = [0, 1, 4]
HBM = 6.0e12
BYTES_PER_PIXEL = 8 + 8 + 4
HOST_THREADS = 16


class _NoWeight(object):
    def __init__(self, inner):
        self.inner = inner

    def __getitem__(self, idx):
        return {k: v for k, v in self.inner[idx].items() if not k.startswith("weight_")}


def _fmt(t):
    return "%10.2f (spread %.2f)" % (statistics.median(t), max(t) - min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import weights_ref
    from ubresnet_amd import synthetic
    from ubresnet_amd.pixel_weights import PixelWeights
    if not torch.cuda.is_available():
        raise SystemExit("weightbench: needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = []

    # ---- (a) the launch pair alone --------------------------------------------------------------------------------------
    legs, labels = {}, {}
    for h, w in SHAPES:
        lab = np.concatenate([synthetic.make_batch(B, 64, 64, 1000 + i)[1] for i in range((h // 64) * (w // 64))], 0)
        lab = lab.reshape(h // 64, w // 64, B, 64, 64).transpose(2, 0, 3, 1, 4).reshape(B, h, w).copy()
        labels[(h, w)] = lab
        label = torch.from_numpy(lab).to(dev)
        weight = torch.empty((B, h, w), dtype=torch.float32, device=dev)
        counts = torch.empty((B, 16), dtype=torch.int64, device=dev)
        for r in RADII:
            pw = PixelWeights(num_classes=3, radius=r, gain=2.0)
            legs["%dx%dx%d r=%d" % (B, h, w, r)] = (lambda pw=pw, label=label, weight=weight, counts=counts, h=h, w=w: pw.launch(
                label.data_ptr(), weight.data_ptr(), counts.data_ptr(), (B, h, w), stream), B * h * w, (label, weight, counts))
    times = {k: [] for k in legs}
    for fn, _, _ in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for name, (fn, _, _) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    lines.append("# (a) ubw_pixel_weights, int64 labels of synthetic crops tiled to the shape; us per call (memset + count pass + apply pass), %d"
                 " back-to-back calls between two device events; median (spread = max - min) over %d alternating repetitions;"
                 " byte bound: %d B/pixel at 6 TB/s" % (a.launches, a.reps, BYTES_PER_PIXEL))
    for name, (_, n, _) in legs.items():
        t = times[name]
        bound = BYTES_PER_PIXEL * n / HBM * 1e6
        lines.append("%-18s %s us   %6.1f MB   bound %6.2f us   x%.2f of the bound   runs: %s" % (
            name, _fmt(t), BYTES_PER_PIXEL * n / 1e6, bound, statistics.median(t) / bound, " ".join("%.2f" % v for v in t)))

    # ---- (b) numpy on host threads --------------------------------------------------------------------------------------
    lines.append("# (b) the numpy reference (tests/weights_ref.py) on the same labels, one image per thread on %d host threads; ms per"
                 " batch, wall clock; median (spread) over %d repetitions" % (HOST_THREADS, a.reps))
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        for h, w in SHAPES:
            lab = labels[(h, w)]
            for r in RADII:
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    list(ex.map(lambda b: weights_ref.reference(lab[b:b + 1], 3, radius=r, gain=2.0), range(B)))
                    t.append((time.perf_counter() - t0) * 1e3)
                lines.append("%-18s %s ms   runs: %s" % ("%dx%dx%d r=%d" % (B, h, w, r), _fmt(t), " ".join("%.2f" % v for v in t)))

    # ---- (c) the train step ---------------------------------------------------------------------------------------------
    if not a.no_train:
        from ubresnet_amd.models.ub_uresnet import UResNet
        from ubresnet_amd.optim import FlatAdam
        from ubresnet_amd.staging import BatchStager
        from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
        torch.manual_seed(0)
        model = UResNet(num_classes=3, input_channels=1, inplanes=16).to(dev)
        model.compute_dtype = torch.bfloat16
        model.train()
        crit, opt = PixelWiseNLLLoss(), FlatAdam(model, lr=1e-3, weight_decay=1e-4)
        stagers = {}
        for name, pw in (("weights=None", None), ("PixelWeights(radius=1, gain=2)", PixelWeights(num_classes=3, radius=1, gain=2.0))):
            ld = synthetic.SyntheticLArCVDataset(height=512, width=512, tag="train", nentries=64, cache=64)
            ld.start(B)
            stagers[name] = BatchStager(_NoWeight(ld), B, 512, 512, tag="train", weights=pw)

        def steps(st, k):
            for _ in range(k):
                x, lab, wgt = st.next()
                loss = crit.forward(model.forward(x), lab, wgt)
                opt.zero_grad()
                loss.backward()
                opt.step()
            crit.flush()
            torch.cuda.synchronize()

        try:
            for st in stagers.values():
                steps(st, 3)
            t = {k: [] for k in stagers}
            for _ in range(a.reps):
                for name, st in stagers.items():
                    t0 = time.perf_counter()
                    steps(st, a.steps)
                    t[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
        finally:
            for st in stagers.values():
                st.close()
        lines.append("# (c) bf16 train step %d x 1 x 512 x 512 through BatchStager, loader without a weight entry; ms per step, %d steps"
                     " between two host clock readings ending in a device synchronise; median (spread) over %d alternating repetitions"
                     % (B, a.steps, a.reps))
        for name in stagers:
            lines.append("%-32s %s ms   runs: %s" % (name, _fmt(t[name]), " ".join("%.2f" % v for v in t[name])))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
