#!/usr/bin/env python3
"""ClusterOverlap (libubresnet_overlap.so) on a synthetic full-size event, 3 x 1008 x 3456, at about 1.3 % lit, at 41 % lit and all
lit: a predicted-style map (8-connected clusters) against a truth-style one (4-connected, by class) of the same lit pixels.

    python tools/overlapbench.py [--events N] [--reps R] [--out FILE]

Six steps, each a fresh child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the run
(nothing is tried again).  Within a step the legs are alternated; a figure is the median (spread = max - min) over `--reps`
repetitions of back-to-back calls between device events.  Every leg walks SETS operand sets in turn (two id maps, a view, a table
and scratch of their own: 4 x 125 MB of ids and view), so that no call finds its operands in the 256 MB last-level cache.

  calls      ubh_overlap (five launches) at the three densities against its byte bound at HBM_TBS: every one of the insert, count
             and number launches reads both id maps (8 B per pixel each), the insert the view where a group of four takes part,
             the clear writes the slots (40 B each) and the number launch the rows (48 B each)
  launches   each of the five launches alone, from the kernel records of torch.profiler
  composite  what a user would write in torch: a packed int64 key, torch.unique(return_inverse, return_counts), index_add_
  host       the download of both maps and the view into pinned memory, then np.unique (tests/overlap_ref.py)
  events     events/s of a fp16 UResNet event with output="products" and both clusterings, with and without co(a, b, view)
  table      the slot load and the longest probe run on those events, read from scratch after a sync (this tool only)
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
CAPACITY = 1 << 20
LIMITS = {"calls": 300, "launches": 240, "composite": 300, "host": 360, "events": 360, "table": 240}      # seconds per step
SHARES = (("1.3 % lit", 0.013), ("41 % lit", 0.41), ("all lit", 1.0))
KERNELS = ("clear_kernel", "insert_kernel", "count_kernel", "scan_kernel", "number_kernel")


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
    """SETS events with `share` of the pixels lit, clustered two ways: [(ids_a, ids_b, view, ClusterOverlap)]"""
    import torch
    from ubresnet_amd import clusters, overlap
    out = []
    pred = clusters.EventClusterer(P, ROWS, COLS, NCLASS, 8, False, 255, CAPACITY, "cuda:0")
    true = clusters.EventClusterer(P, ROWS, COLS, NCLASS, 4, True, 255, CAPACITY, "cuda:0")       # (ids and count are whole above capacity)
    for s in range(SETS):
        g = torch.Generator(device="cuda").manual_seed(11 + s)
        lit = torch.rand((P, ROWS, COLS), device="cuda", generator=g) < share
        label = torch.where(lit, torch.randint(0, NCLASS, (P, ROWS, COLS), device="cuda", generator=g), 255).to(torch.uint8).contiguous()
        conf = torch.where(lit, 1.0, 0.0).to(torch.float16).contiguous()
        view = torch.where(lit, torch.rand((P, ROWS, COLS), device="cuda", generator=g) * 200.0 + 10.0, 0.0).contiguous()
        a, b = pred(label, conf).ids.clone(), true(label, conf).ids.clone()
        pairs = int(true.count.item())                                # b refines a: the pairs are the clusters of b
        co = overlap.ClusterOverlap(P, ROWS, COLS, max(pairs, 1024), None, SCALE, "cuda:0")
        out.append((a, b, view, co))
    del pred, true
    torch.cuda.empty_cache()
    return out


def _bound_us(a, b, co, count):
    """the byte bound of the five launches and of the call, us at HBM_TBS"""
    part = (a >= 0) | (b >= 0)
    groups = int(part.reshape(-1)[:N // 4 * 4].reshape(-1, 4).any(dim=1).sum().item())
    us = lambda nbytes: nbytes / (HBM_TBS * 1e12) * 1e6
    each = {"clear_kernel": us(40 * co.slots), "insert_kernel": us(8 * N + 16 * groups), "count_kernel": us(8 * N + 4 * N // 1024),
            "scan_kernel": us(8 * N // 1024), "number_kernel": us(8 * N + 48 * count)}
    return each, sum(each.values())


def step_calls(a, say):
    import torch
    say("# ubh_overlap, 3 x %d x %d = %d pixels, adc_scale %d, slots = ubh_default_slots(pairs); us per call: median (spread) over %d "
        "alternating repetitions of %d back-to-back calls over %d rotated operand sets, device events; byte bound at %.1f TB/s"
        % (ROWS, COLS, N, SCALE, a.reps, CALLS, SETS, HBM_TBS))
    for name, share in SHARES:
        sets = _sets(share)
        legs = {"ubh_overlap": lambda i: sets[i % SETS][3](*sets[i % SETS][:3]), "ubh_overlap, no view": lambda i: sets[i % SETS][3](*sets[i % SETS][:2])}
        res = _timed(legs, a.reps)
        ia, ib, view, co = sets[0]
        ov = co(ia, ib, view)
        torch.cuda.synchronize()
        count, status = int(ov.count.item()), ov.status.tolist()
        _, bound = _bound_us(ia, ib, co, count)
        for k, (t, s) in res.items():
            say("%-22s %-10s pairs = %7d slots = %8d status = %s  %8.1f us (spread %.1f)  byte bound %5.1f us -> %.2fx the bound"
                % (k, name, count, co.slots, status, t, s, bound, t / bound))


def step_launches(a, say):
    import torch
    from torch.profiler import ProfilerActivity, profile
    say("# each launch of ubh_overlap alone: mean us over %d calls from the kernel records of torch.profiler, %d rotated operand sets; "
        "its byte bound at %.1f TB/s" % (2 * SETS, SETS, HBM_TBS))
    for name, share in SHARES:
        sets = _sets(share)
        for i in range(SETS):
            sets[i][3](*sets[i][:3])
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for i in range(2 * SETS):
                sets[i % SETS][3](*sets[i % SETS][:3])
            torch.cuda.synchronize()
        each, _ = _bound_us(sets[0][0], sets[0][1], sets[0][3], int(sets[0][3].count.item()))
        for kernel in KERNELS:
            got = None
            for ev in prof.key_averages():
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = getattr(ev, "cuda_time_total", 0.0)
                if kernel in ev.key and total > 0:
                    got = total / max(ev.count, 1)
            say("%-14s %-10s %s  byte bound %6.2f us%s" % (kernel, name, "%9.1f us" % got if got is not None else "not measured (no kernel record)",
                                                          each[kernel], " -> %.2fx the bound" % (got / each[kernel]) if got else ""))


def _composite(ids_a, ids_b, view):
    """the torch a user would write: a packed int64 key, torch.unique, index_add_ of the weights, min of the pixel index"""
    import torch
    a, b = ids_a.reshape(-1).clamp_min(-1).long() + 1, ids_b.reshape(-1).clamp_min(-1).long() + 1
    key = (a << 32) | b
    q = torch.nonzero(key).reshape(-1)
    uniq, inverse, pixels = torch.unique(key[q], return_inverse=True, return_counts=True)
    t = view.reshape(-1)[q] * float(SCALE)
    odd = torch.isnan(t) | (t < 0)
    w = torch.where(~odd & (t > 65535.0), 65535.0, torch.where(odd, 0.0, torch.round(t))).long()
    table = torch.zeros((uniq.numel(), 6), dtype=torch.int64, device=key.device)
    table[:, 0], table[:, 1], table[:, 3] = (uniq >> 32) - 1, (uniq & 0xFFFFFFFF) - 1, pixels
    table[:, 2] = torch.full_like(uniq, N).scatter_reduce_(0, inverse, q, "amin")
    table[:, 4].index_add_(0, inverse, (w > 0).long())
    table[:, 5].index_add_(0, inverse, w)
    return table[torch.argsort(table[:, 2])]


def step_composite(a, say):
    import torch
    say("# the torch composite (packed int64 key, torch.unique(return_inverse, return_counts), index_add_, scatter amin, argsort); us "
        "per call: median (spread) over %d repetitions of 2 calls, %d rotated operand sets" % (a.reps, SETS))
    for name, share in SHARES:
        sets = _sets(share)
        legs = {"torch composite": lambda i: _composite(*sets[i % SETS][:3]), "ubh_overlap": lambda i: sets[i % SETS][3](*sets[i % SETS][:3])}
        res = _timed(legs, a.reps, 2)
        ia, ib, view, co = sets[0]
        ov = co(ia, ib, view)
        want = _composite(ia, ib, view)
        torch.cuda.synchronize()
        count = int(ov.count.item())
        same = count == want.shape[0] and bool((ov.table[:count] == want).all())
        for k, (t, s) in res.items():
            say("%-16s %-10s %10.1f us (spread %.1f)" % (k, name, t, s))
        say("the composite's table equals ubh_overlap's: %s; ubh_overlap is x%.1f faster" % (same, res["torch composite"][0] / res["ubh_overlap"][0]))


def step_host(a, say):
    import time
    import torch
    say("# the same table on the host: the %.1f MB download of both maps and the view into pinned memory, then np.unique and np.add.at; "
        "ms per event, median (spread) over %d events" % (12 * N * 1e-6, a.reps))
    h_a, h_b = (torch.empty((P, ROWS, COLS), dtype=torch.int32).pin_memory() for _ in range(2))
    h_view = torch.empty((P, ROWS, COLS), dtype=torch.float32).pin_memory()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import overlap_ref
    for name, share in SHARES:
        ia, ib, view, co = _sets(share)[0]
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_a.copy_(ia, non_blocking=True)
            h_b.copy_(ib, non_blocking=True)
            h_view.copy_(view, non_blocking=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ref = overlap_ref.table(h_a.numpy(), h_b.numpy(), h_view.numpy(), SCALE)
            times.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
        tot, dl = [t[0] for t in times], [t[1] for t in times]
        say("host %-10s pairs = %7d  %9.1f ms (spread %.1f), of which the download %6.2f ms" % (name, len(ref), statistics.median(tot),
                                                                                           max(tot) - min(tot), statistics.median(dl)))


def step_events(a, say):
    import torch
    from ubresnet_amd import clusters, deploy, overlap
    torch.manual_seed(7)
    m = deploy.load_model(None, "cuda:0", num_classes=NCLASS)
    g = torch.Generator(device="cuda").manual_seed(13)
    view = torch.where(torch.rand((P, 1, ROWS, COLS), device="cuda", generator=g) < 0.013, 50.0, 0.0).contiguous()
    seg = deploy.WholeViewSegmenter(m, rows=ROWS, cols=COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float16, use_graph=True,
                                    output="products")
    cl_a = clusters.EventClusterer(P, ROWS, COLS, NCLASS, 8, False, 255, CAPACITY, "cuda:0")
    cl_b = clusters.EventClusterer(P, ROWS, COLS, NCLASS, 4, True, 255, CAPACITY, "cuda:0")
    co = overlap.ClusterOverlap(P, ROWS, COLS, CAPACITY, None, SCALE, "cuda:0")

    def both(i):
        products = seg(view)
        return cl_a(products), cl_b(products)

    legs = {"products + 2 cl": both, "products + 2 cl + co": lambda i: co(*both(i), view)}
    res = _timed(legs, a.reps, a.events)
    ov = co(*both(0), view)
    say("# UResNet ip16 nc4, 3 x %d x %d event = %d tiles of %d x %d, f16, batch %d, hipGraph replay, 1.3 %% lit: %d pairs, status %s"
        % (ROWS, COLS, seg.tiles_per_event, TH, TW, BATCH, int(ov.count.item()), ov.status.tolist()))
    say("# events/s on the device: median (spread) over %d alternating repetitions of %d events" % (a.reps, a.events))
    eps = {}
    for k, (t, s) in res.items():
        eps[k] = (1e6 / t, 1e6 / (t - s / 2) - 1e6 / (t + s / 2))
        say("%-24s %7.2f events/s (spread %.2f)  %8.1f us/event" % (k, eps[k][0], eps[k][1], t))
    (d, ds), (z, zs) = eps["products + 2 cl"], eps["products + 2 cl + co"]
    say("the overlap behind the two clusterings: x%.3f of the leg without, %+.1f us per event (combined spread of the rates %.2f events/s)"
        % (z / d, res["products + 2 cl + co"][0] - res["products + 2 cl"][0], ds + zs))


def step_table(a, say):
    import torch
    from ubresnet_amd import _overlap as HL
    say("# the table in scratch after a call and a sync: occupied slots over slots, and the longest cyclic run of occupied slots "
        "(a pair probes at most %d)" % HL.MAX_PROBES)
    for name, share in SHARES:
        ia, ib, view, co = _sets(share)[0]
        ov = co(ia, ib, view)
        torch.cuda.synchronize()
        taken = (co.scratch[:co.slots * HL.SLOT_WORDS].reshape(co.slots, HL.SLOT_WORDS)[:, 0] != 0)
        free = torch.nonzero(~taken).reshape(-1)
        gaps = torch.diff(free) - 1
        run = int(max(int(gaps.max().item()) if gaps.numel() else 0, int(free[0].item()) + co.slots - 1 - int(free[-1].item())))
        say("%-10s pairs = %7d slots = %8d load = %.3f longest run = %3d status = %s"
            % (name, int(ov.count.item()), co.slots, float(taken.sum().item()) / co.slots, run, ov.status.tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(LIMITS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    steps = {"calls": step_calls, "launches": step_launches, "composite": step_composite, "host": step_host, "events": step_events,
             "table": step_table}
    if a.step:
        steps[a.step](a, lambda s: print(s, flush=True))
        return 0
    out = open(a.out, "w") if a.out else None
    head = "# python tools/overlapbench.py --events %d --reps %d\n" % (a.events, a.reps)
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
