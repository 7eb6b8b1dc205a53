#!/usr/bin/env python3
"""Temperature calibration (libubresnet_calib.so): ubf_apply and ubf_accumulate alone against their byte bounds and against the
torch composites a user would write instead, and events/s of a full-size fp16 UResNet event (3 x 1008 x 3456 = 30 tiles of
512 x 832, batch 10, hipGraph replay, output="products") with and without `temperature`.

    python tools/calibbench.py [--events N] [--reps R] [--out FILE]

Two steps, each a fresh child process under its own time limit; the first step that fails or runs out of time ends the run
(nothing is tried again):

  kernel   ubf_apply in place on 10 x 4 x 512 x 832 (8 B per element: one read, one write) against torch.log_softmax(beta * x);
           ubf_accumulate on a 3 x 1008 x 3456, C = 4 event with K = 33, int64 and uint8 truth, at the lit share of a synthetic
           event and with every pixel lit, against the bytes it must read (truth + lit per pixel, 16 B of scores per counting
           pixel) and against the torch composite (mask, gather, log_softmax per temperature, sums).  Operand sets are rotated so
           that a call does not find its operands in the 256 MB Infinity Cache.  Legs alternate; 50 calls between device events;
           median and spread (max - min) of 5 repetitions.
  events   events/s with and without temperature=(0.8, 1.0, 1.3), alternated in one process, the result left on the device.
"""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROWS, COLS, TH, TW, P, NCLASS, BATCH, K = 1008, 3456, 512, 832, 3, 4, 10, 33
HBM_TBS = 6.0           # the HBM rate the project states its byte bounds against (TB/s)
LIMITS = {"kernel": 420, "events": 420}      # seconds per step


def alternate(legs, nset, calls=50, reps=5):
    """legs: {name: fn(i)} -> {name: (median us per call, spread)}; the legs take turns within every repetition"""
    import torch
    for fn in legs.values():
        for i in range(nset):
            fn(i)
    torch.cuda.synchronize()
    out = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(calls):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    return {name: (statistics.median(v), max(v) - min(v)) for name, v in out.items()}


def step_kernel(a, say):
    import numpy as np
    import torch
    from ubresnet_amd import _calib as F
    from ubresnet_amd import calibration as CB
    from ubresnet_amd import synthetic
    st = torch.cuda.current_stream().cuda_stream
    say("# us per call: median (spread = max - min) of 5 repetitions of 50 back-to-back calls between device events, the legs of a "
        "block alternating, alone on the device; byte bounds at %.1f TB/s" % HBM_TBS)
    # ---- apply
    nset = 6                                                           # 6 x 68 MB: more than the Infinity Cache
    shape = (BATCH, NCLASS, TH, TW)
    xs = [torch.log_softmax(torch.randn(shape, device="cuda") * 3.0, 1).contiguous() for _ in range(nset)]
    betas = torch.from_numpy(np.array([1.0 / (0.8, 1.0, 1.3)[i % 3] for i in range(BATCH)], np.float32)).cuda()
    bcast = betas.reshape(BATCH, 1, 1, 1)
    elems = int(np.prod(shape))
    legs = {"ubf_apply (in place)": lambda i: F.apply(xs[i % nset].data_ptr(), xs[i % nset].data_ptr(), betas.data_ptr(), BATCH, NCLASS, TH, TW, st),
            "torch.log_softmax(beta * x)": lambda i: torch.log_softmax(bcast * xs[i % nset], 1)}
    bound = elems * 8 / (HBM_TBS * 1e12) * 1e6
    for name, (t, sp) in alternate(legs, nset).items():
        say("%-30s %d x %d x %d x %d  %8.1f us (spread %.1f)  byte bound (8 B/element) %5.1f us -> %.2fx the bound, %.2f TB/s of its 8 B"
            % (name, BATCH, NCLASS, TH, TW, t, sp, bound, t / bound, elems * 8 / (t * 1e-6) * 1e-12))
    del xs
    # ---- accumulate
    nset = 4                                                           # 4 x (167 MB scores + truth + lit)
    adc = np.zeros((P, ROWS, COLS), np.float32)
    truth = np.zeros((P, ROWS, COLS), np.int64)
    for p in range(P):
        adc[p], truth[p], _ = synthetic.make_crop(ROWS, COLS, 5000 + p)
    px = P * ROWS * COLS
    share = float((adc > 10.0).mean())
    ops = []
    for i in range(nset):
        ops.append(dict(scores=torch.log_softmax(torch.randn((P, NCLASS, ROWS, COLS), device="cuda") * 3.0, 1).contiguous(),
                        i64=torch.from_numpy(np.roll(truth, 17 * i, 1)).cuda(), lit=torch.from_numpy(np.roll(adc, 17 * i, 1)).cuda()))
        ops[-1]["u8"] = ops[-1]["i64"].to(torch.uint8)
    fit = CB.TemperatureFit(NCLASS, groups=P)
    bet = torch.from_numpy(fit.betas).cuda()
    groups = torch.arange(P, dtype=torch.uint8, device="cuda")
    table = torch.zeros((P, K, 3), dtype=torch.float64, device="cuda")
    counters = torch.zeros((P, 3), dtype=torch.int64, device="cuda")
    nbytes = F.scratch_bytes(P, ROWS, COLS, K)
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")

    def acc(tk, lit):
        def fn(i):
            o = ops[i % nset]
            F.accumulate(o["scores"].data_ptr(), o[tk].data_ptr(), F.TRUTH_U8 if tk == "u8" else F.TRUTH_I64,
                         o["lit"].data_ptr() if lit else None, 10.0, groups.data_ptr(), bet.data_ptr(), K, P, NCLASS, ROWS, COLS, P,
                         table.data_ptr(), counters.data_ptr(), scratch.data_ptr(), nbytes, st)
        return fn

    def composite(lit):
        bs = bet.double()

        def fn(i):
            o = ops[i % nset]
            t = o["i64"]
            m = (t >= 0) & (t < NCLASS)
            if lit:
                m = m & (o["lit"] > 10.0)
            s = o["scores"].permute(0, 2, 3, 1)[m]                       # [M, C]
            tt = t[m]
            out = []
            for k in range(K):
                lp = torch.log_softmax(bs[k] * s.double(), 1)
                out.append(-lp.gather(1, tt[:, None]).sum())
            return torch.stack(out)                                      # the NLL alone: no g, no h, no groups
        return fn

    say("# ubf_accumulate: one %d x %d x %d event per call (%.1f Mpixel), C = %d, K = %d, %d operand sets rotated; lit share of the "
        "synthetic event %.2f %%" % (P, ROWS, COLS, px * 1e-6, NCLASS, K, nset, 100 * share))
    for lit, what, counting in ((True, "%.2f %% lit" % (100 * share), share), (False, "all lit", 1.0)):
        legs = {"ubf_accumulate truth uint8": acc("u8", lit), "ubf_accumulate truth int64": acc("i64", lit)}
        res = alternate(legs, nset, calls=50 if lit else 10)
        for name, (t, sp) in res.items():
            per = (1 if "uint8" in name else 8) + (4 if lit else 0)
            nb = px * (per + 4 * NCLASS * counting)
            bound = nb / (HBM_TBS * 1e12) * 1e6
            say("%-28s %-12s %9.1f us (spread %.1f)  %2d B/pixel + 16 B per counting pixel = %6.1f MB  byte bound %6.1f us -> %.2fx the bound"
                % (name, what, t, sp, per, nb * 1e-6, bound, t / bound))
        t, sp = alternate({"c": composite(lit)}, nset, calls=3, reps=3)["c"]
        say("torch composite (NLL only)   %-12s %9.1f us (spread %.1f; 3 repetitions of 3 calls)" % (what, t, sp))
    say("# (all lit: every pixel costs one wave step of 33 busy lanes and about 4 expf each; the kernel is then bound by arithmetic, not "
        "by bytes, and the ratio above says by how much)")


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
    kw = dict(rows=ROWS, cols=COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float16, use_graph=True, output="products")
    segs = {"products": deploy.WholeViewSegmenter(m, **kw),
            "products, temperature": deploy.WholeViewSegmenter(m, temperature=(0.8, 1.0, 1.3), **kw)}

    def run(v, events):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(events):
            segs[v](view)
        e1.record()
        torch.cuda.synchronize()
        return events / (e0.elapsed_time(e1) * 1e-3)

    for v in segs:
        run(v, 2)
    runs = {v: [] for v in segs}
    for _ in range(a.reps):
        for v in segs:                    # alternating
            runs[v].append(run(v, a.events))
    say("# UResNet ip16 nc4, 3 x %d x %d event = %d tiles of %d x %d, f16, batch %d, hipGraph replay, output=\"products\", result left on "
        "the device; temperature = (0.8, 1.0, 1.3): one ubf_apply over the chunk's tile scores per forward, 3 per event"
        % (ROWS, COLS, segs["products"].tiles_per_event, TH, TW, BATCH))
    say("# events/s: median (spread = max - min) over %d alternating repetitions of %d events = %d timed events per line"
        % (a.reps, a.events, a.reps * a.events))
    med = {v: (statistics.median(runs[v]), max(runs[v]) - min(runs[v])) for v in segs}
    for v in segs:
        say("%-22s %7.2f events/s (spread %.2f)  %6.2f ms/event   runs: %s"
            % (v, med[v][0], med[v][1], 1e3 / med[v][0], " ".join("%.2f" % x for x in runs[v])))
    names = list(segs)
    d = med[names[0]][0] - med[names[1]][0]
    say("difference %.2f events/s against spreads of %.2f and %.2f: %s" % (d, med[names[0]][1], med[names[1]][1],
        "inside the spread, nothing is claimed" if abs(d) <= max(med[names[0]][1], med[names[1]][1]) else "outside the spread"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(LIMITS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    if a.events * a.reps < 20:
        ap.error("at least 20 timed events per variant (--events x --reps)")
    steps = {"kernel": step_kernel, "events": step_events}
    if a.step:
        steps[a.step](a, lambda s: print(s, flush=True))
        return 0
    out = open(a.out, "w") if a.out else None
    rc = 0
    for step in ("kernel", "events"):
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
