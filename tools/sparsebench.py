#!/usr/bin/env python3
"""Sparse event I/O (libubresnet_sparse.so) on a synthetic full-size event, 3 x 1008 x 3456, at about 1.3 % and at 100 % lit: the
three calls alone against their byte bounds, the torch composite a user would write without them, and whole-view inference
INCLUDING the host copies, dense in / products out against sparse in / pixels out.

    python tools/sparsebench.py [--events N] [--reps R] [--out FILE]

Three steps, each a fresh child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the run
(nothing is tried again).  Within a step the legs are alternated; a figure is the median (spread = max - min) over `--reps`
repetitions of 50 back-to-back calls (`--events` events in the last step) between device events.

  calls      ubz_scatter_view, ubz_compact and ubz_expand alone, against their byte bounds at HBM_TBS
  composite  what a user would write in torch: zeros + index_put_ for the scatter; nonzero + three gathers for the compaction
             (nonzero synchronises: the host has to learn the length); full + index_put_ twice for the expand
  events     events/s of a fp16 UResNet event (30 tiles of 512 x 832, batch 10, hipGraph replay) at 1.3 % lit, every event from
             pinned host memory back to pinned host memory: the dense view uploaded and the products downloaded, against the list
             uploaded and PixelList.read() (the count, then that many entries)
"""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROWS, COLS, TH, TW, P, NCLASS, BATCH = 1008, 3456, 512, 832, 3, 4, 10
N = P * ROWS * COLS
HBM_TBS = 6.0           # the HBM rate the project states its byte bounds against (TB/s)
CALLS = 50              # back-to-back calls between two device events
LIMITS = {"calls": 240, "composite": 240, "events": 420}      # seconds per step
SHARES = (("1.3 % lit", 0.013), ("100 % lit", 1.0))


def _timed(legs, reps, calls=CALLS):
    """legs: {name: fn}; alternated; -> {name: (median us per call, spread)}"""
    import torch
    for fn in legs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            runs[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    return {k: (statistics.median(r), max(r) - min(r)) for k, r in runs.items()}


def _event(share, seed):
    """(view [P,1,ROWS,COLS] with `share` of the pixels at ADC 50, label, confidence) on the device"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand((P, 1, ROWS, COLS), device="cuda", generator=g)
    view = torch.where(u < share, 50.0, 0.0).contiguous()
    lit = view[:, 0] > 10.0
    label = torch.where(lit, torch.randint(0, NCLASS, (P, ROWS, COLS), device="cuda", generator=g), 255).to(torch.uint8)
    conf = torch.where(lit, torch.rand((P, ROWS, COLS), device="cuda", generator=g), 0.0).to(torch.float16)
    return view, label, conf


def step_calls(a, say):
    import torch
    from ubresnet_amd import deploy, sparse
    say("# the three calls alone, 3 x %d x %d = %d pixels; us per call: median (spread) over %d alternating repetitions of %d back-to-back "
        "calls, device events; byte bounds at %.1f TB/s" % (ROWS, COLS, N, a.reps, CALLS, HBM_TBS))
    for name, share in SHARES:
        view, label, conf = _event(share, 11)
        ev = sparse.SparseEvent.from_dense(view)
        dev = sparse.SparseEvent(ev.index.cuda(), ev.value.cuda(), P, ROWS, COLS)
        n = dev.n
        out, status = torch.empty_like(view), torch.zeros(1, dtype=torch.int64, device="cuda")
        comp = sparse.Compactor(P, ROWS, COLS, None, "cuda")
        prod = deploy.Products(label, conf, None)
        pl = comp(label, conf, None, view, 1, 10.0, 255)
        legs = {"ubz_scatter_view": lambda: dev.to_view("cuda", out=out, status=status),
                "ubz_compact": lambda: comp(prod.label, prod.confidence, None, view, 1, 10.0, 255),
                "ubz_expand": lambda: pl.to_products(status=status)}
        # scatter: the view written once, the list read; compact: adc read twice, label and confidence of the lit pixels, the list
        # written; expand: both planes written once, the list read
        nbytes = {"ubz_scatter_view": 4 * N + 12 * n, "ubz_compact": 8 * N + 3 * n + 7 * n, "ubz_expand": 3 * N + 7 * n}
        res = _timed(legs, a.reps)
        assert int(status) == 0 and int(pl.count) == n
        for k, (t, s) in res.items():
            bound = nbytes[k] / (HBM_TBS * 1e12) * 1e6
            say("%-18s %-10s n = %8d  %8.1f us (spread %.1f)  %6.1f MB  byte bound %6.1f us -> %.2fx the bound, %.2f TB/s"
                % (k, name, n, t, s, nbytes[k] * 1e-6, bound, t / bound, nbytes[k] / (t * 1e-6) * 1e-12))
    say("# (to_products allocates its two output planes per call; the other two legs reuse their buffers)")


def step_composite(a, say):
    import torch
    say("# the torch composite of the same three operations, same events, same timing")
    for name, share in SHARES:
        view, label, conf = _event(share, 11)
        flat, lab, cf = view.reshape(-1), label.reshape(-1), conf.reshape(-1)
        index = torch.nonzero(flat.view(torch.int32) != 0).reshape(-1)
        value, li, ci = flat[index], lab[index], cf[index]

        def scatter():
            v = torch.zeros(N, dtype=torch.float32, device="cuda")
            v.index_put_((index,), value)

        def compact():
            idx = torch.nonzero(flat > 10.0).reshape(-1)          # synchronises
            return idx.to(torch.int32), lab[idx], cf[idx]

        def expand():
            ol = torch.full((N,), 255, dtype=torch.uint8, device="cuda")
            oc = torch.zeros(N, dtype=torch.float16, device="cuda")
            ol.index_put_((index,), li)
            oc.index_put_((index,), ci)

        res = _timed({"zeros + index_put_": scatter, "nonzero + gathers": compact, "full + index_put_ x 2": expand}, a.reps)
        for k, (t, s) in res.items():
            say("%-22s %-10s n = %8d  %8.1f us (spread %.1f)" % (k, name, index.numel(), t, s))


def step_events(a, say):
    import torch
    from ubresnet_amd import deploy, sparse
    torch.manual_seed(7)
    m = deploy.load_model(None, "cuda:0", num_classes=NCLASS)
    view = _event(0.013, 13)[0]
    event = sparse.SparseEvent.from_dense(view)
    kw = dict(rows=ROWS, cols=COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float16, use_graph=True)
    dense_seg = deploy.WholeViewSegmenter(m, output="products", **kw)
    sparse_seg = deploy.WholeViewSegmenter(m, output="pixels", capacity=N // 8, **kw)
    h_view = view.cpu().pin_memory()
    d_view = torch.empty_like(view)
    h_prod = [torch.empty((P, ROWS, COLS), dtype=torch.uint8).pin_memory(), torch.empty((P, ROWS, COLS), dtype=torch.float16).pin_memory(),
              torch.empty((P, NCLASS), dtype=torch.int64).pin_memory()]
    h_event = sparse.SparseEvent(event.index.pin_memory(), event.value.pin_memory(), P, ROWS, COLS)
    h_list = [torch.empty(N // 8, dtype=torch.int32).pin_memory(), torch.empty(N // 8, dtype=torch.uint8).pin_memory(),
              torch.empty(N // 8, dtype=torch.float16).pin_memory()]
    got = {}

    def dense_leg():
        d_view.copy_(h_view, non_blocking=True)
        out = dense_seg(d_view)
        for h, d in zip(h_prod, out):
            h.copy_(d, non_blocking=True)

    def sparse_leg():
        pl = sparse_seg(h_event)
        total = int(pl.count.item())                             # read(): the count first -- the one synchronisation
        if total > pl.capacity:
            raise OverflowError(total)
        for h, d in zip(h_list, (pl.index, pl.label, pl.confidence)):
            h[:total].copy_(d[:total], non_blocking=True)
        got["n"] = total

    def device_leg():
        dense_seg(view)

    res = _timed({"dense in, products out": dense_leg, "sparse in, pixels out": sparse_leg, "on the device (no copies)": device_leg}, a.reps, a.events)
    nb = {"dense in, products out": (4 * N, 3 * N + 8 * P * NCLASS), "sparse in, pixels out": (8 * event.n, 8 + 7 * got["n"]),
          "on the device (no copies)": (0, 0)}
    say("# UResNet ip16 nc4, 3 x %d x %d event = %d tiles of %d x %d, f16, batch %d, hipGraph replay; %d list entries in, %d lit pixels out"
        % (ROWS, COLS, dense_seg.tiles_per_event, TH, TW, BATCH, event.n, got["n"]))
    say("# events/s including the host copies (pinned): median (spread) over %d alternating repetitions of %d events" % (a.reps, a.events))
    eps = {}
    for k, (t, s) in res.items():
        eps[k] = (1e6 / t, 1e6 / (t - s / 2) - 1e6 / (t + s / 2))
        say("%-28s %7.2f events/s (spread %.2f)  %8.1f us/event  H2D %6.2f MB  D2H %6.2f MB"
            % (k, eps[k][0], eps[k][1], t, nb[k][0] * 1e-6, nb[k][1] * 1e-6))
    (d, ds), (z, zs) = eps["dense in, products out"], eps["sparse in, pixels out"]
    verdict = "sparse I/O FASTER" if z - d > ds + zs else ("sparse I/O SLOWER" if d - z > ds + zs else "level within the spreads")
    say("sparse in / pixels out vs dense in / products out: x%.3f, %+.2f events/s against a combined spread of %.2f -> %s"
        % (z / d, z - d, ds + zs, verdict))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(LIMITS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    steps = {"calls": step_calls, "composite": step_composite, "events": step_events}
    if a.step:
        steps[a.step](a, lambda s: print(s, flush=True))
        return 0
    out = open(a.out, "w") if a.out else None
    head = "# python tools/sparsebench.py --events %d --reps %d\n" % (a.events, a.reps)
    print(head, end="", flush=True)
    if out:
        out.write(head)
    rc = 0
    for step in ("calls", "composite", "events"):
        cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--events", str(a.events),
               "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        text, rc = r.stdout, r.returncode
        if rc in (124, 137):
            text += "# step %s ran out of its %d s\n" % (step, LIMITS[step])
        elif rc != 0:
            text += "# step %s FAILED (exit %d)\n%s" % (step, rc, r.stderr[-2000:])
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
