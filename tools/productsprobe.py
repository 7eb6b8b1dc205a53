#!/usr/bin/env python3
"""Whole-view inference with output="scores" against output="products": events/s of a full-size fp16 UResNet event
(3 x 1008 x 3456 = 30 tiles of 512 x 832, batch 10, hipGraph replay), and the stitch launch against ubp_stitch_products alone.

    python tools/productsprobe.py [--events N] [--reps R] [--out FILE]

Two steps, each a fresh child process under its own time limit; the first step that fails or runs out of time ends the run
(nothing is tried again):

  events   events/s of both outputs, alternated in one process, with the result left on the device and with the result copied
           to reused pinned host buffers (the .cpu() of the reference's deploy loops).  Device events around `--events` events
           per repetition after warm-up; median and spread (max - min) over the repetitions.
  kernel   one chunk of 10 tiles: ubr_stitch_tiles and ubp_stitch_products on synthetic log-probabilities at 2 % and at 100 %
           lit occupancy, against their byte bounds at HBM_TBS.  Six input sets are rotated (6 x 68 MB) so that a launch
           does not find its scores in the 256 MB Infinity Cache from the launch before.
"""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROWS, COLS, TH, TW, P, NCLASS, BATCH = 1008, 3456, 512, 832, 3, 4, 10
HBM_TBS = 6.0           # the HBM rate the project states its byte bounds against (TB/s)
LIMITS = {"events": 300, "kernel": 180}      # seconds per step


def _view():
    import numpy as np
    import torch
    from ubresnet_amd import synthetic
    adc = np.zeros((P, 1, ROWS, COLS), np.float32)
    for p in range(P):
        adc[p, 0] = synthetic.make_crop(ROWS, COLS, 5000 + p)[0]
    return torch.from_numpy(adc).cuda()


def step_events(a, say):
    import torch
    from ubresnet_amd import deploy
    torch.manual_seed(7)
    m = deploy.load_model(None, "cuda:0", num_classes=NCLASS)
    view = _view()
    lit = float((view > 10.0).float().mean())
    kw = dict(rows=ROWS, cols=COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float16, use_graph=True)
    segs = {"scores": deploy.WholeViewSegmenter(m, output="scores", **kw), "products": deploy.WholeViewSegmenter(m, output="products", **kw)}
    host = {"scores": [torch.empty((P, NCLASS, ROWS, COLS), dtype=torch.float32).pin_memory()],
            "products": [torch.empty((P, ROWS, COLS), dtype=torch.uint8).pin_memory(),
                         torch.empty((P, ROWS, COLS), dtype=torch.float16).pin_memory(),
                         torch.empty((P, NCLASS), dtype=torch.int64).pin_memory()]}

    def run(name, to_host, events):
        seg = segs[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(events):
            out = seg(view)
            if to_host:
                for h, d in zip(host[name], out if name == "products" else [out]):
                    h.copy_(d, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        return events / (e0.elapsed_time(e1) * 1e-3)

    variants = [(n, h) for h in (False, True) for n in ("scores", "products")]
    for v in variants:                    # warm-up of every graph and every copy
        run(v[0], v[1], 2)
    runs = {v: [] for v in variants}
    for _ in range(a.reps):
        for v in variants:                # alternating
            runs[v].append(run(v[0], v[1], a.events))
    nbytes = {"scores": P * NCLASS * ROWS * COLS * 4, "products": P * ROWS * COLS * 3 + P * NCLASS * 8}
    say("# UResNet ip16 nc4, 3 x %d x %d event = %d tiles of %d x %d, f16, batch %d, hipGraph replay; %.2f %% of the pixels above ADC 10"
        % (ROWS, COLS, segs["scores"].tiles_per_event, TH, TW, BATCH, 100 * lit))
    say("# events/s: median (spread = max - min) over %d alternating repetitions of %d events = %d timed events per line"
        % (a.reps, a.events, a.reps * a.events))
    med = {}
    for v in variants:
        r = runs[v]
        med[v] = (statistics.median(r), max(r) - min(r))
        say("%-9s %-28s %7.2f events/s (spread %.2f)  D2H %6.1f MB/event   runs: %s"
            % (v[0], "copied to pinned host" if v[1] else "left on the device", med[v][0], med[v][1],
               nbytes[v[0]] * 1e-6 if v[1] else 0.0, " ".join("%.2f" % x for x in r)))
    for h in (False, True):
        (ts, ss), (tp, sp) = med[("scores", h)], med[("products", h)]
        verdict = "products FASTER" if tp - ts > ss + sp else ("products SLOWER" if ts - tp > ss + sp else "level within the spreads")
        say("products vs scores, %s: x%.3f, %+.2f events/s against a combined spread of %.2f -> %s"
            % ("host" if h else "device", tp / ts, tp - ts, ss + sp, verdict))


def step_kernel(a, say):
    import ctypes as C
    import torch
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _post as PL
    from ubresnet_amd import deploy
    tiles = deploy.view_tiles(ROWS, COLS, P, TH, TW, False)[:BATCH]         # the ten tiles of plane 0
    kept = sum((min(t[4], ROWS - t[1]) - t[3]) * (min(t[6], COLS - t[2]) - t[5]) for t in tiles)
    flat = [v for t in tiles for v in t]
    desc = (C.c_int32 * len(flat))(*flat)
    g = torch.Generator(device="cuda").manual_seed(3)
    nset = 6
    logp = [torch.log_softmax(torch.randn((BATCH, NCLASS, TH, TW), device="cuda", generator=g) * 3, 1) for _ in range(nset)]
    dense = torch.empty((P, NCLASS, ROWS, COLS), dtype=torch.float32, device="cuda")
    label = torch.empty((P, ROWS, COLS), dtype=torch.uint8, device="cuda")
    conf = torch.empty((P, ROWS, COLS), dtype=torch.float16, device="cuda")
    counts = torch.zeros((P, NCLASS), dtype=torch.int64, device="cuda")
    u = torch.rand((P, 1, ROWS, COLS), device="cuda", generator=g)
    adcs = {"2 % lit": torch.where(u < 0.02, 50.0, 0.0).contiguous(), "100 % lit": torch.full_like(u, 50.0)}
    lib, post = L.lib(), PL.lib()

    def stitch(i):
        L.check(lib.ubr_stitch_tiles(logp[i % nset].data_ptr(), NCLASS, TH, TW, desc, BATCH, dense.data_ptr(), P, ROWS, COLS, L.stream_ptr()))

    def products(adc):
        def f(i):
            PL.check(post.ubp_stitch_products(logp[i % nset].data_ptr(), NCLASS, TH, TW, desc, BATCH, adc.data_ptr(), 1, 10.0,
                                              label.data_ptr(), conf.data_ptr(), counts.data_ptr(), 255, P, ROWS, COLS, L.stream_ptr()))
        return f

    def time_us(fn, n=60, reps=5):
        for i in range(nset):
            fn(i)
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / n)
        return statistics.median(out), max(out) - min(out)

    say("# one chunk of %d tiles (plane 0, %d kept pixels), C = %d; us per launch: median (spread) over 5 repetitions of 60 back-to-back "
        "launches, device events; byte bounds at %.1f TB/s" % (BATCH, kept, NCLASS, HBM_TBS))
    rows = [("ubr_stitch_tiles", stitch, kept * 8 * NCLASS)]
    for name, adc in adcs.items():
        share = float((adc[0] > 10.0).float().mean())
        rows.append(("ubp_stitch_products, %s" % name, products(adc), int(kept * (4 + 3 + share * 4 * NCLASS))))
    for name, fn, nbytes in rows:
        t, s = time_us(fn)
        bound = nbytes / (HBM_TBS * 1e12) * 1e6
        say("%-32s %8.1f us (spread %.1f)  %7.1f MB  byte bound %6.1f us  -> %.2fx the bound, %.2f TB/s"
            % (name, t, s, nbytes * 1e-6, bound, t / bound, nbytes / (t * 1e-6) * 1e-12))
    say("# (the 2 % bound counts 4 C bytes for lit pixels only; the scores arrive in whole cache lines, so the traffic is higher)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(LIMITS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    if a.events * a.reps < 20:
        ap.error("at least 20 timed events per variant (--events x --reps)")
    if a.step:
        {"events": step_events, "kernel": step_kernel}[a.step](a, lambda s: print(s, flush=True))
        return 0
    out = open(a.out, "w") if a.out else None
    rc = 0
    for step in ("events", "kernel"):
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
