#!/usr/bin/env python3
"""uba_augment_batch against ubd_prep_batch at 16 x 1 x 512 x 512, alone on the device, alternated in one process.

    python tools/augbench.py [--launches N] [--reps R] [--out FILE]

A repetition is `--launches` back-to-back launches of one kernel between two device events; the two kernels alternate; median
and spread (max - min) of the per-launch time over `--reps` repetitions.  The augment kernel reads (P + 2) * 4 bytes per pixel
(image, wire label, weight) and writes (P + 1) * 4 + 8 (image, weight, int64 label); the prep kernel with the threshold off
reads 4 and writes 8.  The byte bound is those bytes at 6 TB/s."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, P, H, W = 16, 1, 512, 512
HBM = 6.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from ubresnet_amd import _aug, _data, synthetic
    from ubresnet_amd.augment import Augment
    dev = torch.device("cuda:0")
    n = B * H * W
    x, lab, wgt = synthetic.make_batch(B, H, W, 1000)
    packed = torch.from_numpy(np.concatenate([x.reshape(-1), lab.astype(np.float32).reshape(-1), wgt.reshape(-1)])).to(dev)
    adc = torch.empty((B, P, H, W), dtype=torch.float32, device=dev)
    label = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    weight = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    base = packed.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    legs = {}
    for name, aug in (("augment Augment()", Augment()), ("augment flips only", Augment(pad=0)), ("augment identity", Augment(pad=0, flip_rows=False, flip_cols=False))):
        par = aug.params(0, B)
        legs[name] = (lambda par=par, aug=aug: _aug.augment_batch(base, base + 4 * P * n, base + 4 * (P + 1) * n, adc.data_ptr(), label.data_ptr(),
                                                                  weight.data_ptr(), (B, P, H, W), aug.pad, par, stream=stream), (P + 2) * 4 + (P + 1) * 4 + 8)
    legs["prep_batch"] = (lambda: _data.prep_batch(base + 4 * P * n, label.data_ptr(), n, 0, stream=stream), 4 + 8)
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
    lines = ["# %d x %d x %d x %d, fp32; us per launch, %d back-to-back launches between two device events; median (spread = max - min) over %d"
             " alternating repetitions; byte bound at 6 TB/s" % (B, P, H, W, a.launches, a.reps)]
    for name, (_, bytes_per_pixel) in legs.items():
        t = times[name]
        bound = bytes_per_pixel * n / HBM * 1e6
        lines.append("%-22s %8.2f us (spread %.2f)   %6.1f MB   bound %6.2f us   x%.2f of the bound   runs: %s" % (
            name, statistics.median(t), max(t) - min(t), bytes_per_pixel * n / 1e6, bound, statistics.median(t) / bound,
            " ".join("%.2f" % v for v in t)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
