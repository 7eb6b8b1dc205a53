#!/usr/bin/env python3
"""ClusterMoments (libubresnet_moment.so) on a synthetic full-size event, 3 x 1008 x 3456, C = 4, at about 1.3 % lit, at 41 % lit and
all lit (one cluster per plane: every workgroup adds into the same three table rows).

    python tools/momentbench.py [--events N] [--reps R] [--out FILE]

Five steps, each a fresh child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the run
(nothing is tried again).  Within a step the legs are alternated; a figure is the median (spread = max - min) over `--reps`
repetitions of back-to-back calls between device events.  Every leg walks SETS operand sets in turn (ids, label, view, root,
confidence and tables of their own: 4 x 94 MB of moment operands), so that no call finds its operands in the 256 MB last-level
cache.

  calls      ubm_moments (clear + accumulation) and ubi_tabulate (count, scan, number, tally) at the three densities; ubm_moments
             against its byte bound: 9 bytes per pixel (ids, view, label) at HBM_TBS
  launches   the accumulation launch of ubm_moments and the tally launch of ubi_tabulate alone, from the kernel records of
             torch.profiler: the tally is the unchanged yardstick of the contended case (per-wave combination only)
  composite  what a user would write in torch: the weight rule, then one int64 index_add_ per column (1.3 % and 41 % lit; all lit
             is left out: ten times 10.4 M atomic adds on three rows)
  host       the download of ids and view into pinned memory, then np.add.at per column
  events     events/s of a fp16 UResNet event with output="products" + cl(products), with and without cm(found, view) behind it
"""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROWS, COLS, TH, TW, P, NCLASS, BATCH, SCALE = 1008, 3456, 512, 832, 3, 4, 10, 16
N = P * ROWS * COLS
HBM_TBS = 6.0           # the HBM rate the project states its byte bounds against (TB/s)
CALLS = 20              # back-to-back calls between two device events
SETS = 4                # operand sets a leg rotates through
LIMITS = {"calls": 300, "launches": 240, "composite": 300, "host": 360, "events": 360}      # seconds per step
SHARES = (("1.3 % lit", 0.013), ("41 % lit", 0.41), ("all lit", 1.0))


def _timed(legs, reps, calls=CALLS):
    """legs: {name: fn(i)}, i the call's number (the legs pick their operand set by it); alternated; -> {name: (median us, spread)}"""
    import torch
    for fn in legs.values():
        for i in range(SETS):
            fn(i)
    torch.cuda.synchronize()
    runs = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(calls):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            runs[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    return {k: (statistics.median(r), max(r) - min(r)) for k, r in runs.items()}


def _sets(share):
    """SETS clustered events with `share` of the pixels lit: [(label, conf, view, clusterer, moments, found)]"""
    import torch
    from ubresnet_amd import clusters, shapes
    out = []
    for s in range(SETS):
        g = torch.Generator(device="cuda").manual_seed(11 + s)
        lit = torch.rand((P, ROWS, COLS), device="cuda", generator=g) < share
        label = torch.where(lit, torch.randint(0, NCLASS, (P, ROWS, COLS), device="cuda", generator=g), 255).to(torch.uint8).contiguous()
        conf = torch.where(lit, torch.rand((P, ROWS, COLS), device="cuda", generator=g), 0.0).to(torch.float16).contiguous()
        view = torch.where(lit, torch.rand((P, ROWS, COLS), device="cuda", generator=g) * 200.0 + 10.0, 0.0).contiguous()
        cl = clusters.EventClusterer(P, ROWS, COLS, NCLASS, 8, False, 255, 1 << 20, "cuda:0")
        cm = shapes.ClusterMoments(cl, adc_scale=SCALE)
        found = cl(label, conf)
        assert int(found.count.item()) <= cl.capacity, "the table is short"
        out.append((label, conf, view, cl, cm, found))
    return out


def _legs(sets):
    from ubresnet_amd import _cluster as I, _lib as L

    def moments(i):
        label, conf, view, cl, cm, found = sets[i % SETS]
        cm(found, view)

    def tabulate(i):
        label, conf, view, cl, cm, found = sets[i % SETS]
        I.tabulate(label.data_ptr(), conf.data_ptr(), cl.root.data_ptr(), NCLASS, 255, cl.ids.data_ptr(), cl.table.data_ptr(), cl.capacity,
                   cl.count.data_ptr(), cl.scratch.data_ptr(), P, ROWS, COLS, L.stream_ptr())

    return {"ubm_moments": moments, "ubi_tabulate": tabulate}


def step_calls(a, say):
    say("# ubm_moments and ubi_tabulate, 3 x %d x %d = %d pixels, C = %d, adc_scale %d; us per call: median (spread) over %d alternating "
        "repetitions of %d back-to-back calls over %d rotated operand sets, device events; byte bound of ubm_moments: 9 N = %.1f MB at "
        "%.1f TB/s" % (ROWS, COLS, N, NCLASS, SCALE, a.reps, CALLS, SETS, 9 * N * 1e-6, HBM_TBS))
    bound = 9 * N / (HBM_TBS * 1e12) * 1e6
    seen = {}
    for name, share in SHARES:
        sets = _sets(share)
        found = sets[0][5]
        count, lit = int(found.count.item()), int((found.ids >= 0).sum().item())
        res = _timed(_legs(sets), a.reps)
        seen[name] = res
        t, s = res["ubm_moments"]
        say("ubm_moments   %-10s lit = %8d clusters = %7d  %8.1f us (spread %.1f)  byte bound %5.1f us -> %.2fx the bound" % (name, lit, count, t, s, bound, t / bound))
        t, s = res["ubi_tabulate"]
        say("ubi_tabulate  %-10s lit = %8d clusters = %7d  %8.1f us (spread %.1f)" % (name, lit, count, t, s))
    for leg in ("ubm_moments", "ubi_tabulate"):
        (t0, s0), (t1, s1) = seen["1.3 % lit"][leg], seen["all lit"][leg]
        say("%s all lit vs 1.3 %% lit: %.1f us against %.1f us (combined spread %.1f) -> the contended case costs x%.1f the sparse one"
            % (leg, t1, t0, s0 + s1, t1 / t0))


def step_launches(a, say):
    import torch
    from torch.profiler import ProfilerActivity, profile
    say("# the accumulation launch of ubm_moments and the tally launch of ubi_tabulate alone: mean us over %d calls each from the kernel "
        "records of torch.profiler, %d rotated operand sets" % (2 * SETS, SETS))
    for name, share in SHARES:
        sets = _sets(share)
        legs = _legs(sets)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for i in range(2 * SETS):
                legs["ubm_moments"](i)
                legs["ubi_tabulate"](i)
            torch.cuda.synchronize()
        for kernel in ("clear_kernel", "moment_kernel", "tally_kernel"):
            got = None
            for ev in prof.key_averages():
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = getattr(ev, "cuda_time_total", 0.0)
                if kernel in ev.key and total > 0:
                    got = total / max(ev.count, 1)
            say("%-14s %-10s %s" % (kernel, name, "%9.1f us" % got if got is not None else "not measured (no kernel record)"))


def _composite(ids, label, view, table):
    """the torch a user would write: the weight rule, then one int64 index_add_ per column"""
    import torch
    width = table.shape[1]
    q = torch.nonzero(ids.reshape(-1) >= 0).reshape(-1)
    k = ids.reshape(-1)[q].long()
    t = view.reshape(-1)[q] * float(SCALE)
    odd = torch.isnan(t) | (t < 0)
    clipped = ~odd & (t > 65535.0)
    w = torch.where(clipped, 65535.0, torch.where(odd, 0.0, torch.round(t))).long()
    r, c = (q % (ROWS * COLS)) // COLS, q % COLS
    flat = table.reshape(-1)
    flat.zero_()
    for j, col in enumerate(((w > 0).long(), clipped.long(), odd.long(), w, w * r, w * c, w * r * r, w * r * c, w * c * c)):
        flat.index_add_(0, k * width + j, col)
    flat.index_add_(0, k * width + 9 + label.reshape(-1)[q].long(), w)


def step_composite(a, say):
    import torch
    say("# the torch composite (weight rule, then one int64 index_add_ per column into a table of its own); us per call: median "
        "(spread) over %d repetitions of 2 calls, %d rotated operand sets; all lit is left out" % (a.reps, SETS))
    for name, share in SHARES[:2]:
        sets = _sets(share)
        tables = [torch.zeros_like(s[4].table) for s in sets]

        def composite(i):
            label, conf, view, cl, cm, found = sets[i % SETS]
            _composite(found.ids, label, view, tables[i % SETS])

        res = _timed({"torch composite": composite, "ubm_moments": _legs(sets)["ubm_moments"]}, a.reps, 2)
        count = int(sets[0][5].count.item())
        same = bool((tables[0][:count] == sets[0][4].table[:count]).all())
        for k, (t, s) in res.items():
            say("%-16s %-10s %10.1f us (spread %.1f)" % (k, name, t, s))
        say("the composite's table equals ubm_moments': %s; ubm_moments is x%.0f faster" % (same, res["torch composite"][0] / res["ubm_moments"][0]))


def step_host(a, say):
    import time
    import numpy as np
    import torch
    say("# the same table on the host: the %.1f MB download of ids and view into pinned memory, then the weight rule and np.add.at per "
        "column; ms per event, median (spread) over %d events" % (8 * N * 1e-6, a.reps))
    h_ids, h_view = torch.empty((P, ROWS, COLS), dtype=torch.int32).pin_memory(), torch.empty((P, ROWS, COLS), dtype=torch.float32).pin_memory()
    h_label = torch.empty((P, ROWS, COLS), dtype=torch.uint8).pin_memory()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import moment_ref
    for name, share in SHARES:
        label, conf, view, cl, cm, found = _sets(share)[0]
        count = int(found.count.item())
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_ids.copy_(found.ids, non_blocking=True)
            h_view.copy_(view, non_blocking=True)
            h_label.copy_(label, non_blocking=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            moment_ref.table(h_ids.numpy(), h_label.numpy(), h_view.numpy(), NCLASS, SCALE, count, count)
            times.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
        tot, dl = [t[0] for t in times], [t[1] for t in times]
        say("host %-10s clusters = %7d  %9.1f ms (spread %.1f), of which the download %6.2f ms" % (name, count, statistics.median(tot),
                                                                                              max(tot) - min(tot), statistics.median(dl)))


def step_events(a, say):
    import torch
    from ubresnet_amd import clusters, deploy, shapes
    torch.manual_seed(7)
    m = deploy.load_model(None, "cuda:0", num_classes=NCLASS)
    g = torch.Generator(device="cuda").manual_seed(13)
    view = torch.where(torch.rand((P, 1, ROWS, COLS), device="cuda", generator=g) < 0.013, 50.0, 0.0).contiguous()
    seg = deploy.WholeViewSegmenter(m, rows=ROWS, cols=COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float16, use_graph=True,
                                    output="products")
    cl = clusters.EventClusterer(P, ROWS, COLS, NCLASS, 8, False, 255, 1 << 20, "cuda:0")
    cm = shapes.ClusterMoments(cl, adc_scale=SCALE)
    legs = {"products + cl": lambda i: cl(seg(view)), "products + cl + cm": lambda i: cm(cl(seg(view)), view)}
    res = _timed(legs, a.reps, a.events)
    say("# UResNet ip16 nc4, 3 x %d x %d event = %d tiles of %d x %d, f16, batch %d, hipGraph replay, 1.3 %% lit: %d clusters"
        % (ROWS, COLS, seg.tiles_per_event, TH, TW, BATCH, int(cl(seg(view)).count.item())))
    say("# events/s on the device: median (spread) over %d alternating repetitions of %d events" % (a.reps, a.events))
    eps = {}
    for k, (t, s) in res.items():
        eps[k] = (1e6 / t, 1e6 / (t - s / 2) - 1e6 / (t + s / 2))
        say("%-22s %7.2f events/s (spread %.2f)  %8.1f us/event" % (k, eps[k][0], eps[k][1], t))
    (d, ds), (z, zs) = eps["products + cl"], eps["products + cl + cm"]
    say("the moments behind the clusters: x%.3f of the leg without, %+.1f us per event (combined spread of the rates %.2f events/s)"
        % (z / d, res["products + cl + cm"][0] - res["products + cl"][0], ds + zs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(LIMITS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    steps = {"calls": step_calls, "launches": step_launches, "composite": step_composite, "host": step_host, "events": step_events}
    if a.step:
        steps[a.step](a, lambda s: print(s, flush=True))
        return 0
    out = open(a.out, "w") if a.out else None
    head = "# python tools/momentbench.py --events %d --reps %d\n" % (a.events, a.reps)
    print(head, end="", flush=True)
    if out:
        out.write(head)
    rc = 0
    for step in steps:
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
