#!/usr/bin/env python3
"""ubx_apply (libubresnet_det.so) alone on the device, the same effects in numpy on 16 host threads, the table copy, and the bf16
train step through BatchStager with and without a detector; legs alternated in one process.

    python tools/detbench.py [--launches N] [--reps R] [--steps S] [--out FILE]

A repetition of a kernel leg is `--launches` back-to-back launches between two device events (the image is restored from a
pristine copy in front of the first event: the call works in place); the legs alternate; median and spread (max - min) of the
per-launch time over `--reps` repetitions.  Every leg uses a non-unit gain, so every image element is read and written once:
the byte bound is 8 bytes per element at 6 TB/s (the table and the few label and weight stores are not counted).  The host legs
do the same to a numpy batch, one image per thread on 16 threads.  A repetition of a step leg is `--steps` train steps between two
host clock readings that end in a device synchronise.  The worst ratio of an error to the bound of tests/det_ref.py is taken over
one 16 x 1 x 512 x 512 batch with noise on every pixel."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SHAPES = [(16, 1, 512, 512), (16, 3, 512, 832)]
HBM = 6.0e12
SETTINGS = [("dead wires + gain", dict(noise_sigma=0.0)), ("+ noise on lit pixels", dict(noise_sigma=1.5)),
            ("+ noise on all pixels", dict(noise_sigma=1.5, noise_on="all"))]
DET = dict(dead_runs=(0, 3), run_len=(1, 32), gain=(0.9, 1.1), dead_label=0, dead_weight=0.0, seed=1)


def crops(np, shape):
    """synthetic crops at any plane count: plane p of image b is the crop of seed 1000 + b * P + p"""
    from ubresnet_amd import synthetic
    b, p, h, w = shape
    x = synthetic.make_batch(b * p, h, w, 1000)[0].reshape(b, p, h, w)
    _, lab, wgt = synthetic.make_batch(b, h, w, 1000)
    return np.ascontiguousarray(x), lab.astype(np.int64), wgt


def host_effects(np, x, table, sigma, noise_all, seed):
    """the same effects in numpy, in place on image b (the noise from numpy's own generator: the cost is what is measured)"""
    def one(b):
        rs = np.random.RandomState(seed + b)
        for p in range(x.shape[1]):
            words = table[b, p, 1:]
            dead = np.unpackbits(words.view(np.uint8), bitorder="little")[:x.shape[3]].astype(bool)
            v = x[b, p]
            lit = np.ones(v.shape, bool) if noise_all else v != 0
            v *= table[b, p, :1].view(np.float32)[0]
            if sigma > 0:
                v[lit] += np.float32(sigma) * rs.standard_normal(int(lit.sum())).astype(np.float32)
            v[:, dead] = 0.0
    return one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import det_ref
    from ubresnet_amd import synthetic
    from ubresnet_amd.detector import DetectorEffects
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.staging import BatchStager
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = ["# ubx_apply, fp32, in place; us per launch, %d back-to-back launches between two device events; median (spread = max - min) over %d"
             " alternating repetitions; byte bound: 8 bytes per image element at 6 TB/s; host: numpy, one image per thread on 16 threads, ms per batch"
             % (a.launches, a.reps)]
    pool = ThreadPoolExecutor(max_workers=16)
    for shape in SHAPES:
        b, p, h, w = shape
        x, lab, wgt = crops(np, shape)
        pristine = torch.from_numpy(x).to(dev)
        image = torch.empty_like(pristine)
        label, weight = torch.from_numpy(lab).to(dev), torch.from_numpy(wgt).to(dev)
        legs, host = {}, {}
        for name, kw in SETTINGS:
            det = DetectorEffects(**dict(DET, **kw))
            table = det.table(0, b, p, w)
            dtab = torch.from_numpy(table.view(np.int32)).to(dev)
            legs[name] = lambda det=det, dtab=dtab: det.launch(image.data_ptr(), label.data_ptr(), weight.data_ptr(), shape, dtab.data_ptr(), 0, stream)
            host[name] = (table, det.noise_sigma, det.noise_on == "all")
        times = {k: [] for k in legs}
        for fn in legs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, fn in legs.items():
                image.copy_(pristine)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        htimes = {k: [] for k in legs}
        for _ in range(a.reps):
            for name, (table, sigma, noise_all) in host.items():
                y = x.copy()
                t0 = time.perf_counter()
                list(pool.map(host_effects(np, y, table, sigma, noise_all, 7), range(b)))
                htimes[name].append((time.perf_counter() - t0) * 1e3)
        nbytes = 8 * b * p * h * w
        bound = nbytes / HBM * 1e6
        lit = float((x != 0).mean())
        lines.append("%d x %d x %d x %d (%.1f %% of the pixels lit), %.1f MB, bound %.2f us" % (b, p, h, w, 100 * lit, nbytes / 1e6, bound))
        for name in legs:
            t, ht = times[name], htimes[name]
            lines.append("  %-24s %8.2f us (spread %.2f)  x%.2f of the bound   runs: %s   | host %7.2f ms (spread %.2f)" % (
                name, statistics.median(t), max(t) - min(t), statistics.median(t) / bound, " ".join("%.2f" % v for v in t),
                statistics.median(ht), max(ht) - min(ht)))
    # the table copy: a pinned array to the device, non-blocking, as the stager issues it
    for b, p, h, w in SHAPES:
        table = DetectorEffects(**DET).table(0, b, p, w)
        pinned = torch.from_numpy(table.view(np.int32).reshape(-1).copy()).pin_memory()
        dtab = torch.empty(pinned.numel(), dtype=torch.int32, device=dev)
        t = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                dtab.copy_(pinned, non_blocking=True)
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        t0 = time.perf_counter()
        for _ in range(20):
            DetectorEffects(**DET).table(3, b, p, w)
        lines.append("table copy %d x %d x %d words (%d bytes): %.2f us (spread %.2f); DetectorEffects.table on the host: %.3f ms" % (
            b, p, table.shape[2], table.nbytes, statistics.median(t), max(t) - min(t), (time.perf_counter() - t0) / 20 * 1e3))
    # the worst ratio to the derived bound
    b, p, h, w = SHAPES[0]
    x, lab, wgt = crops(np, SHAPES[0])
    det = DetectorEffects(**dict(DET, noise_sigma=1.5, noise_on="all"))
    table = det.table(5, b, p, w)
    image = torch.from_numpy(x).to(dev)
    dtab = torch.from_numpy(table.view(np.int32)).to(dev)
    label, weight = torch.from_numpy(lab).to(dev), torch.from_numpy(wgt).to(dev)
    det.launch(image.data_ptr(), label.data_ptr(), weight.data_ptr(), SHAPES[0], dtab.data_ptr(), 5, stream)
    torch.cuda.synchronize()
    ref = det_ref.reference(x, lab, wgt, table, det.noise_sigma, True, det.seed, 5, det.dead_label, det.dead_weight)
    worst = det_ref.compare(image.cpu().numpy(), ref)
    lines.append("worst error / derived bound over %d noisy elements of one 16 x 1 x 512 x 512 batch (sigma 1.5 on every pixel): %.3f" % (
        int(ref["noisy"].sum()), worst))
    # the train step through the stager
    torch.manual_seed(0)
    model = UResNet(num_classes=3, input_channels=1, inplanes=16).to(dev)
    model.compute_dtype = torch.bfloat16
    crit, opt = PixelWiseNLLLoss(), FlatAdam(model, lr=1e-3, weight_decay=1e-4)
    stagers = {}
    for name, det in (("without a detector", None), ("with a detector", DetectorEffects(**dict(DET, noise_sigma=1.5)))):
        ld = synthetic.SyntheticLArCVDataset(height=512, width=512, tag="train", nentries=64, cache=64)
        ld.start(16)
        stagers[name] = BatchStager(ld, 16, 512, 512, tag="train", detector=det)

    def run(st, n):
        for _ in range(n):
            adc, label, weight = st.next()
            loss = crit.forward(model.forward(adc), label, weight)
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
    stimes = {k: [] for k in stagers}
    for st in stagers.values():
        run(st, 10)
    for _ in range(a.reps):
        for name, st in stagers.items():
            t0 = time.perf_counter()
            run(st, a.steps)
            stimes[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    for st in stagers.values():
        st.close()
    lines.append("# bf16 train step, 16 x 1 x 512 x 512, through BatchStager; ms per step, %d steps per repetition; median (spread) over %d"
                 " alternating repetitions" % (a.steps, a.reps))
    for name, t in stimes.items():
        lines.append("  %-20s %7.3f ms (spread %.3f)   runs: %s" % (name, statistics.median(t), max(t) - min(t), " ".join("%.3f" % v for v in t)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
