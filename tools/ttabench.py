#!/usr/bin/env python3
"""Flip test-time augmentation (libubresnet_tta.so, deploy.WholeViewSegmenter(tta=...)): the two launches against their byte
bounds and against the torch composite a user would write instead, events/s of a full-size fp16 UResNet event (3 x 1008 x 3456 =
30 tiles of 512 x 832, batch 10, hipGraph replay) with tta off, ("cols",) and ("rows", "cols", "both"), and the worst
error-to-bound ratio of the merge over the cases of tests/tta_ref.py.

    python tools/ttabench.py [--events N] [--reps R] [--out FILE]

Three steps, each a fresh child process under its own time limit; the first step that fails or runs out of time ends the run
(nothing is tried again):

  exact    every merge case of tests/tta_ref.py (the shapes and view counts of tests/test_gpu_tta_exact.py) on the device against
           the fp64 reference: the worst |error| / bound.
  kernel   10 tiles x 3 classes x 512 x 832 (one chunk's log-probabilities, 51 MB): ubt_flip_planes and ubt_merge_view for every
           flip against their byte bounds at HBM_TBS, and torch.flip / torch.logaddexp / sub on the same buffers.  Six buffer
           sets are rotated (6 x 51 MB per operand) so that a launch does not find its operands in the 256 MB Infinity Cache.
  events   events/s of tta off, two views and four views, for output="scores" and "products", alternated in one process, the
           result left on the device.  Device events around `--events` events per repetition after warm-up; median and spread
           (max - min) over the repetitions; each leg against the tta=None leg of the same run.
"""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROWS, COLS, TH, TW, P, NCLASS, BATCH = 1008, 3456, 512, 832, 3, 4, 10
KCLASS = 3              # the kernel step's planes: 10 tiles x 3 classes
HBM_TBS = 6.0           # the HBM rate the project states its byte bounds against (TB/s)
LIMITS = {"exact": 240, "kernel": 240, "events": 420}      # seconds per step
TTAS = (("off", None), ("cols", ("cols",)), ("rows+cols+both", ("rows", "cols", "both")))


def step_exact(a, say):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import tta_ref as R
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _tta as T
    worst, at, cases = 0.0, None, 0
    for name, s in R.SHAPES.items():
        n, H, W = s["shape"]
        rs = np.random.RandomState(sum(s["shape"]) % 65521)
        views = [R.logsoftmax_rows(rs, s["shape"]) for _ in range(R.MAX_VIEWS)]
        dev = []
        for v in views + [views[0]]:                                # the last one is the accumulator
            full = torch.empty(n * H * W + 64 + s["offset"], dtype=torch.float32, device="cuda")
            t = full[64 + s["offset"]:].view(n, H, W)
            t.copy_(torch.from_numpy(v))
            dev.append(t)
        for K, first in R.merge_cases(name):
            if K == 1:
                continue
            flips = R.view_flips(K, first)
            for k, f in enumerate(flips):
                T.merge_view(dev[k].data_ptr(), dev[-1].data_ptr(), n, H, W, f, k, K, L.stream_ptr())
            torch.cuda.synchronize()
            ref, lim = R.merge(views[:K], flips)
            ratio = float((np.abs(dev[-1].cpu().numpy().astype(np.float64) - ref) / lim).max())
            cases += 1
            if ratio > worst:
                worst, at = ratio, "%d x %d x %d, K = %d, flips %s" % (n, H, W, K, flips)
    say("# ubt_merge_view against the fp64 reference and the derived bound of tests/tta_ref.py (2 ulp per expf / log1pf, half an ulp per add)")
    say("worst |error| / bound over %d merge cases: %.3f  (%s)" % (cases, worst, at))


def step_kernel(a, say):
    import torch
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _tta as T
    n, nset = BATCH * KCLASS, 6
    elems = n * TH * TW
    g = torch.Generator(device="cuda").manual_seed(3)
    src = [torch.log_softmax(torch.randn((BATCH, KCLASS, TH, TW), device="cuda", generator=g) * 4, 1) for _ in range(nset)]
    dst = [torch.log_softmax(torch.randn((BATCH, KCLASS, TH, TW), device="cuda", generator=g) * 4, 1) for _ in range(nset)]
    log2 = float(torch.tensor(2.0).log())

    def time_us(fn, reps_n=60, reps=5):
        for i in range(nset):
            fn(i)
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(reps_n):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / reps_n)
        return statistics.median(out), max(out) - min(out)

    def flip(f):
        return lambda i: T.flip_planes(src[i % nset].data_ptr(), dst[i % nset].data_ptr(), n, TH, TW, f, L.stream_ptr())

    def merge(f, k, K):
        return lambda i: T.merge_view(src[i % nset].data_ptr(), dst[i % nset].data_ptr(), n, TH, TW, f, k, K, L.stream_ptr())

    dims = {1: [2], 2: [3], 3: [2, 3]}

    def torch_flip(f):
        return lambda i: dst[i % nset].copy_(torch.flip(src[i % nset], dims[f]))

    def torch_merge(f, last):
        def fn(i):
            d = dst[i % nset]
            torch.logaddexp(d, torch.flip(src[i % nset], dims[f]), out=d)
            if last:
                d.sub_(log2)
        return fn

    say("# %d planes of %d x %d fp32 (%.1f MB per operand), six operand sets rotated; us per call: median (spread) over 5 repetitions of 60 "
        "back-to-back calls, device events, alone on the device; byte bounds at %.1f TB/s" % (n, TH, TW, elems * 4e-6, HBM_TBS))
    rows = [("ubt_flip_planes flip %d" % f, flip(f), 8) for f in range(4)]
    rows += [("ubt_merge_view k=0 flip %d" % f, merge(f, 0, 2), 8) for f in (0, 3)]
    rows += [("ubt_merge_view k=1 of 4 flip %d" % f, merge(f, 1, 4), 12) for f in range(4)]
    rows += [("ubt_merge_view last of 2 flip %d" % f, merge(f, 1, 2), 12) for f in (2, 3)]
    rows += [("torch flip + copy_, flip %d" % f, torch_flip(f), 8) for f in (2, 3)]
    rows += [("torch flip, logaddexp, flip %d" % f, torch_merge(f, False), 12) for f in (2, 3)]
    rows += [("torch flip, logaddexp, sub, flip 3", torch_merge(3, True), 12)]
    for name, fn, per in rows:
        t, s = time_us(fn)
        bound = elems * per / (HBM_TBS * 1e12) * 1e6
        say("%-36s %8.1f us (spread %.1f)  %d B/element  byte bound %6.1f us  -> %.2fx the bound, %.2f TB/s"
            % (name, t, s, per, bound, t / bound, elems * per / (t * 1e-6) * 1e-12))
    say("# (the torch rows are held to the same minimal bytes; their temporaries move more)")


def step_events(a, say):
    import numpy as np
    import torch
    from ubresnet_amd import deploy, synthetic
    torch.manual_seed(7)
    m = deploy.load_model(None, "cuda:0", num_classes=NCLASS)
    adc = np.zeros((P, 1, ROWS, COLS), np.float32)
    for p in range(P):
        adc[p, 0] = synthetic.make_crop(ROWS, COLS, 5000 + p)[0]
    view = torch.from_numpy(adc).cuda()
    kw = dict(rows=ROWS, cols=COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float16, use_graph=True)
    variants = [(o, name) for o in ("scores", "products") for name, _ in TTAS]
    segs = {(o, name): deploy.WholeViewSegmenter(m, output=o, tta=tta, **kw) for o in ("scores", "products") for name, tta in TTAS}

    def run(v, events):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(events):
            segs[v](view)
        e1.record()
        torch.cuda.synchronize()
        return events / (e0.elapsed_time(e1) * 1e-3)

    for v in variants:
        run(v, 2)
    runs = {v: [] for v in variants}
    for _ in range(a.reps):
        for v in variants:                # alternating
            runs[v].append(run(v, a.events))
    say("# UResNet ip16 nc4, 3 x %d x %d event = %d tiles of %d x %d, f16, batch %d, hipGraph replay, result left on the device"
        % (ROWS, COLS, segs[variants[0]].tiles_per_event, TH, TW, BATCH))
    say("# events/s: median (spread = max - min) over %d alternating repetitions of %d events = %d timed events per line"
        % (a.reps, a.events, a.reps * a.events))
    med = {v: (statistics.median(runs[v]), max(runs[v]) - min(runs[v])) for v in variants}
    for v in variants:
        K = 1 + len(dict(TTAS)[v[1]] or ())
        base = med[(v[0], "off")][0]
        say("%-9s tta %-15s K = %d  %7.2f events/s (spread %.2f)  %6.2f ms/event = x%.3f of tta off (K views: x%d)   runs: %s"
            % (v[0], v[1], K, med[v][0], med[v][1], 1e3 / med[v][0], base / med[v][0], K, " ".join("%.2f" % x for x in runs[v])))
    for o in ("scores", "products"):
        t1 = 1e3 / med[(o, "off")][0]
        for name, tta in TTAS[1:]:
            K = 1 + len(tta)
            tk = 1e3 / med[(o, name)][0]
            say("%s, K = %d: %.2f ms/event against %d x %.2f = %.2f ms of K plain events: %+.2f ms (%+.1f %%)"
                % (o, K, tk, K, t1, K * t1, tk - K * t1, 100 * (tk - K * t1) / (K * t1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(LIMITS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    if a.events * a.reps < 20:
        ap.error("at least 20 timed events per variant (--events x --reps)")
    steps = {"exact": step_exact, "kernel": step_kernel, "events": step_events}
    if a.step:
        steps[a.step](a, lambda s: print(s, flush=True))
        return 0
    out = open(a.out, "w") if a.out else None
    rc = 0
    for step in ("exact", "kernel", "events"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--events", str(a.events), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[step])
            text, rc = r.stdout, r.returncode
            if rc != 0:
                text += "# step %s FAILED (exit %d)\n%s" % (step, rc, r.stderr[-2000:])
        except subprocess.TimeoutExpired as e:
            so = e.stdout.decode("utf-8", "replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
            text, rc = so + "# step %s ran out of its %d s\n" % (step, LIMITS[step]), 124
        print(text, end="", flush=True)
        if out:
            out.write(text)
            out.flush()
        if rc != 0:
            break                          # nothing more goes to the GPU after a failure
    if out:
        out.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
