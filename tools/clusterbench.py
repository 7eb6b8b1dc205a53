#!/usr/bin/env python3
"""EventClusters (libubresnet_cluster.so) on a synthetic full-size event, 3 x 1008 x 3456, C = 4, at about 1.3 % lit, at 41 % lit
(the 8-connected percolation threshold: the most tortuous clusters) and all lit (one cluster per plane: the contended tally).

    python tools/clusterbench.py [--events N] [--reps R] [--out FILE]

Four steps, each a fresh child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the run
(nothing is tried again).  Within a step the legs are alternated; a figure is the median (spread = max - min) over `--reps`
repetitions of 20 back-to-back calls (`--events` events in the events step) between device events.

  calls      ubi_label (three launches) and ubi_tabulate (four launches) alone, against the sum of their launches' byte bounds
  host       the same clustering on the host: the 31 MB download of label and confidence into pinned memory, then
             scipy.ndimage.label per plane (the numpy reference of tests/cluster_ref.py if scipy is absent) and the per-cluster
             pixel and class counts by bincount
  events     events/s of a fp16 UResNet event (30 tiles of 512 x 832, batch 10, hipGraph replay) with output="products", with
             and without cl(products) behind it, in the same run
  launches   each of the seven launches alone, from the kernel records of torch.profiler over 10 calls, against its byte bound

Byte bounds at HBM_TBS, from the bytes a pass must move (N pixels, L lit, T tiles of 32 x 64 with 96 border pixels each):
  local    N label bytes read, 4 N root bytes written                                   5 N
  border   the label of every border pixel and of its three neighbours, one root word  8 * 96 T
  flatten  4 N root bytes read, one word written per lit pixel                          4 N + 4 L
  count    4 N root bytes read                                                          4 N
  scan     one word per 1024 pixels, read and written                                   8 N / 1024
  number   4 N root bytes read, -1 written at every pixel that is not lit               4 N + 4 (N - L)
  tally    root and label of every pixel, confidence, the root's number and ids of the lit  5 N + 10 L
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
CALLS = 20              # back-to-back calls between two device events
LIMITS = {"calls": 240, "host": 300, "events": 420, "launches": 240}      # seconds per step
SHARES = (("1.3 % lit", 0.013), ("41 % lit", 0.41), ("all lit", 1.0))
KERNELS = ("local_kernel", "border_kernel", "flatten_kernel", "count_kernel", "scan_kernel", "number_kernel", "tally_kernel")


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
    """(label, confidence) of an event with `share` of the pixels lit, on the device"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    lit = torch.rand((P, ROWS, COLS), device="cuda", generator=g) < share
    label = torch.where(lit, torch.randint(0, NCLASS, (P, ROWS, COLS), device="cuda", generator=g), 255).to(torch.uint8)
    conf = torch.where(lit, torch.rand((P, ROWS, COLS), device="cuda", generator=g), 0.0).to(torch.float16)
    return label.contiguous(), conf.contiguous()


def _bounds(lit):
    from ubresnet_amd import _cluster as I
    tiles = P * -(-ROWS // I.TILE_H) * -(-COLS // I.TILE_W)
    return {"local_kernel": 5 * N, "border_kernel": 8 * (I.TILE_H + I.TILE_W) * tiles, "flatten_kernel": 4 * N + 4 * lit, "count_kernel": 4 * N,
            "scan_kernel": 8 * N // I.PIXEL_BLOCK, "number_kernel": 4 * N + 4 * (N - lit), "tally_kernel": 5 * N + 10 * lit}


def _clusterer():
    from ubresnet_amd import clusters
    return clusters.EventClusterer(P, ROWS, COLS, NCLASS, 8, False, 255, 1 << 20, "cuda:0")


def step_calls(a, say):
    import torch
    from ubresnet_amd import _cluster as I, _lib as L
    say("# ubi_label and ubi_tabulate alone, 3 x %d x %d = %d pixels, C = %d, 8-connected; us per call: median (spread) over %d alternating "
        "repetitions of %d back-to-back calls, device events; byte bounds at %.1f TB/s" % (ROWS, COLS, N, NCLASS, a.reps, CALLS, HBM_TBS))
    tally = {}
    for name, share in SHARES:
        label, conf = _event(share, 11)
        cl = _clusterer()
        found = cl(label, conf)
        count, lit = int(found.count.item()), int((found.ids >= 0).sum().item())
        assert count <= cl.capacity, "the table is short"
        b = _bounds(lit)

        def label_leg():
            I.label(label.data_ptr(), NCLASS, 255, 8, False, cl.root.data_ptr(), cl.status.data_ptr(), P, ROWS, COLS, L.stream_ptr())

        def tabulate_leg():
            I.tabulate(label.data_ptr(), conf.data_ptr(), cl.root.data_ptr(), NCLASS, 255, cl.ids.data_ptr(), cl.table.data_ptr(), cl.capacity,
                       cl.count.data_ptr(), cl.scratch.data_ptr(), P, ROWS, COLS, L.stream_ptr())

        res = _timed({"ubi_label": label_leg, "ubi_tabulate": tabulate_leg, "cl(label, confidence)": lambda: cl(label, conf)}, a.reps)
        nbytes = {"ubi_label": b["local_kernel"] + b["border_kernel"] + b["flatten_kernel"],
                  "ubi_tabulate": b["count_kernel"] + b["scan_kernel"] + b["number_kernel"] + b["tally_kernel"]}
        nbytes["cl(label, confidence)"] = nbytes["ubi_label"] + nbytes["ubi_tabulate"]
        for k, (t, s) in res.items():
            bound = nbytes[k] / (HBM_TBS * 1e12) * 1e6
            say("%-22s %-10s lit = %8d clusters = %7d  %8.1f us (spread %.1f)  %6.1f MB  byte bound %6.1f us -> %.2fx the bound"
                % (k, name, lit, count, t, s, nbytes[k] * 1e-6, bound, t / bound))
        tally[name] = res["ubi_tabulate"]
    (t0, s0), (t1, s1) = tally["1.3 % lit"], tally["all lit"]
    say("ubi_tabulate all lit (one cluster per plane, every wave on the same three table rows) vs 1.3 %% lit: %.1f us against %.1f us, "
        "combined spread %.1f -> the contended tally costs %s" % (t1, t0, s0 + s1, "MORE" if t1 - t0 > s0 + s1 else "no more"))


def step_host(a, say):
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor
    try:
        from scipy import ndimage
        how = "scipy.ndimage.label per plane"
    except ImportError:
        ndimage, how = None, "the numpy reference of tests/cluster_ref.py"
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import cluster_ref
    torch.set_num_threads(16)
    say("# the same clustering on the host (%s, three planes on a pool of threads, 16 threads allowed), including the %.1f MB download "
        "of label and confidence into pinned memory; ms per event, median (spread) over %d events" % (how, 3 * N * 1e-6, a.reps))
    h_label, h_conf = torch.empty((P, ROWS, COLS), dtype=torch.uint8).pin_memory(), torch.empty((P, ROWS, COLS), dtype=torch.float16).pin_memory()
    import time
    for name, share in SHARES:
        label, conf = _event(share, 11)
        times, counts = [], 0
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_label.copy_(label, non_blocking=True)
            h_conf.copy_(conf, non_blocking=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            lab = h_label.numpy()
            if ndimage is not None:
                def plane(p):
                    ids, n = ndimage.label(lab[p] < NCLASS, structure=np.ones((3, 3), np.int32))
                    flat, cls = ids.reshape(-1), lab[p].reshape(-1)
                    sizes = np.bincount(flat, minlength=n + 1)
                    per_class = [np.bincount(flat[cls == c], minlength=n + 1) for c in range(NCLASS)]
                    return n, sizes, per_class
                with ThreadPoolExecutor(max_workers=P) as ex:
                    counts = sum(r[0] for r in ex.map(plane, range(P)))
            else:
                counts = cluster_ref.reference(lab, h_conf.numpy().view(np.uint16), NCLASS, 255, 8, False)["count"]
            times.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
        tot, dl = [t[0] for t in times], [t[1] for t in times]
        say("host %-10s clusters = %7d  %9.1f ms (spread %.1f), of which the download %6.2f ms" % (name, counts, statistics.median(tot),
                                                                                              max(tot) - min(tot), statistics.median(dl)))


def step_events(a, say):
    import torch
    from ubresnet_amd import deploy
    torch.manual_seed(7)
    m = deploy.load_model(None, "cuda:0", num_classes=NCLASS)
    g = torch.Generator(device="cuda").manual_seed(13)
    view = torch.where(torch.rand((P, 1, ROWS, COLS), device="cuda", generator=g) < 0.013, 50.0, 0.0).contiguous()
    seg = deploy.WholeViewSegmenter(m, rows=ROWS, cols=COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float16, use_graph=True,
                                    output="products")
    cl = _clusterer()
    res = _timed({"products": lambda: seg(view), "products + cl(products)": lambda: cl(seg(view))}, a.reps, a.events)
    found = cl(seg(view))
    say("# UResNet ip16 nc4, 3 x %d x %d event = %d tiles of %d x %d, f16, batch %d, hipGraph replay, 1.3 %% lit: %d clusters"
        % (ROWS, COLS, seg.tiles_per_event, TH, TW, BATCH, int(found.count.item())))
    say("# events/s on the device: median (spread) over %d alternating repetitions of %d events" % (a.reps, a.events))
    eps = {}
    for k, (t, s) in res.items():
        eps[k] = (1e6 / t, 1e6 / (t - s / 2) - 1e6 / (t + s / 2))
        say("%-26s %7.2f events/s (spread %.2f)  %8.1f us/event" % (k, eps[k][0], eps[k][1], t))
    (d, ds), (z, zs) = eps["products"], eps["products + cl(products)"]
    say("clustering behind the products: x%.3f of the products leg, %+.1f us per event (combined spread of the rates %.2f events/s)"
        % (z / d, res["products + cl(products)"][0] - res["products"][0], ds + zs))


def step_launches(a, say):
    import torch
    from torch.profiler import ProfilerActivity, profile
    say("# each launch alone: mean us over 10 calls from the kernel records of torch.profiler; byte bounds at %.1f TB/s" % HBM_TBS)
    for name, share in SHARES:
        label, conf = _event(share, 11)
        cl = _clusterer()
        found = cl(label, conf)
        lit = int((found.ids >= 0).sum().item())
        b = _bounds(lit)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(10):
                cl(label, conf)
            torch.cuda.synchronize()
        seen = {}
        for ev in prof.key_averages():
            total = getattr(ev, "device_time_total", None)
            if total is None:
                total = getattr(ev, "cuda_time_total", 0.0)
            for k in KERNELS:
                if k in ev.key and total > 0:
                    seen[k] = total / max(ev.count, 1)
        for k in KERNELS:
            bound = b[k] / (HBM_TBS * 1e12) * 1e6
            if k in seen:
                say("%-15s %-10s %8.1f us  %6.1f MB  byte bound %6.2f us -> %.2fx the bound" % (k, name, seen[k], b[k] * 1e-6, bound, seen[k] / bound))
            else:
                say("%-15s %-10s not measured (no kernel record)  %6.1f MB  byte bound %6.2f us" % (k, name, b[k] * 1e-6, bound))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(LIMITS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    steps = {"calls": step_calls, "host": step_host, "events": step_events, "launches": step_launches}
    if a.step:
        steps[a.step](a, lambda s: print(s, flush=True))
        return 0
    out = open(a.out, "w") if a.out else None
    head = "# python tools/clusterbench.py --events %d --reps %d\n" % (a.events, a.reps)
    print(head, end="", flush=True)
    if out:
        out.write(head)
    rc = 0
    for step in ("calls", "host", "events", "launches"):
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
