#!/usr/bin/env python3
"""PlaneMatcher (libubresnet_match.so) on full-size events, 3 x 1008 x 3456: at about 1.3 % lit with min_pixels=20, and on a
synthetic.make_matched_event.

    python tools/matchbench.py [--events N] [--reps R] [--slots S] [--out FILE]

Five steps, each a fresh child process under its own `timeout -k 10`; the first step that fails or runs out of time ends the run
(nothing is tried again).  Within a step the legs are alternated; a figure is the median (spread = max - min) over `--reps`
repetitions of back-to-back calls between device events.  Every leg walks SETS operand sets in turn (an id map, a view, a cluster
table and a matcher of their own: 84 MB of ids and view each), so that no call finds its operands in the 256 MB last-level cache.

  calls      ubu_match (five launches) on both kinds of event against the sum of its byte bounds at HBM_TBS
  launches   each of the five launches alone, from the kernel records of torch.profiler, against its byte bound: the clear writes
             profile, counts and candidates; the select reads two columns of the cluster rows and writes slot_of; the profile reads
             ids (4 B per pixel) and the view where a group of four holds a candidate; the summary reads profile and counts of the
             candidates; the match reads both strips of every tile that has work, once per chunk inside its hulls, and writes 32 B
             per pair.  The match also against its min-add operations: pairs x bins of the chunks it walks, at OPS_TOPS.
  composite  what a user would write in torch from the profile: minimum(prof[:, None], prof[None]).sum(-1) in chunks of candidates
  host       the download of ids and the view into pinned memory, then numpy (tests/match_ref.py)
  events     events/s of a fp16 UResNet event with output="products" and a clusterer, with and without pm(found, view)
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
OPS_TOPS = 40.0         # 256 CUs x 64 lanes x 2.4 GHz: one 32-bit integer operation per lane and cycle (T op/s)
CALLS = 20
SETS = 4
CAPACITY = 1 << 20
MIN_PIXELS = 20
LIMITS = {"calls": 300, "launches": 240, "composite": 240, "host": 300, "events": 360}
KINDS = ("1.3 % lit", "matched")
KERNELS = ("clear_kernel", "select_kernel", "profile_kernel", "summary_kernel", "match_kernel")


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


def _sets(kind, slots):
    """SETS events of one kind, clustered: [(found, view, PlaneMatcher)], each with a clusterer of its own"""
    import numpy as np
    import torch
    from ubresnet_amd import clusters, planes, synthetic
    out = []
    for s in range(SETS):
        cl = clusters.EventClusterer(P, ROWS, COLS, NCLASS, 8, False, 255, CAPACITY, "cuda:0")
        if kind == "matched":
            image, lab, _ = synthetic.make_matched_event(P, ROWS, COLS, 100 + s, objects=40)
            view = torch.from_numpy(image).cuda()
            label = torch.from_numpy(np.where(image > 0, lab, 255).astype(np.uint8)).cuda()
        else:                                                     # blobs of 9 x 9 pixels: 1.3 % lit, clusters of 81 pixels and more
            g = torch.Generator(device="cuda").manual_seed(11 + s)
            seeds = (torch.rand((P, 1, ROWS, COLS), device="cuda", generator=g) < 0.013 / 81).float()
            lit = torch.nn.functional.max_pool2d(seeds, 9, 1, 4)[:, 0] > 0
            label = torch.where(lit, torch.randint(0, NCLASS, (P, ROWS, COLS), device="cuda", generator=g), 255).to(torch.uint8).contiguous()
            view = torch.where(lit, torch.rand((P, ROWS, COLS), device="cuda", generator=g) * 200.0 + 10.0, 0.0).contiguous()
        conf = torch.where(label != 255, 1.0, 0.0).to(torch.float16).contiguous()
        found = cl(label, conf)
        out.append((found, view, planes.PlaneMatcher(cl, slots, MIN_PIXELS, 1, None, SCALE)))
    return out


def _bounds(found, view, pm, m):
    """({kernel: byte bound us}, min-add operations of the match launch, its pairs) from what the call left on the device"""
    import torch
    from ubresnet_amd import _match as UL
    n = min(int(m.ncand.item()), pm.slots)
    cand = m.candidates[:n].cpu()
    slot_of = torch.full((pm.capacity,), -1, dtype=torch.int64, device="cuda")
    slot_of[m.candidates[:n, 0]] = torch.arange(n, device="cuda")
    ids = found.ids.reshape(-1)
    held = (ids >= 0) & (slot_of[ids.clamp_min(0)] >= 0)
    groups = int(held[:N // 4 * 4].reshape(-1, 4).any(dim=1).sum().item())
    clusters_read = min(int(found.count.item()), pm.capacity)
    strip_bytes, ops, pairs = 0, 0, 0
    for ti in range(-(-n // UL.TILE)):
        for tj in range(ti, -(-n // UL.TILE)):
            a, b = cand[ti * UL.TILE:(ti + 1) * UL.TILE], cand[tj * UL.TILE:(tj + 1) * UL.TILE]
            pairs += len(a) * (len(a) - 1) // 2 if ti == tj else len(a) * len(b)
            lo, hi = max(int(a[:, 4].min()), int(b[:, 4].min())), min(int(a[:, 5].max()), int(b[:, 5].max()))
            if int(a[0, 1]) == int(b[-1, 1]) or lo > hi:
                continue
            chunks = hi // UL.CHUNK_BINS - lo // UL.CHUNK_BINS + 1
            strip_bytes += chunks * 2 * UL.TILE * UL.CHUNK_BINS * 4
            ops += chunks * UL.TILE * UL.TILE * UL.CHUNK_BINS
    us = lambda nbytes: nbytes / (HBM_TBS * 1e12) * 1e6
    each = {"clear_kernel": us(8 * pm.slots * pm.T + 48 * pm.slots), "select_kernel": us(16 * clusters_read + 4 * pm.capacity),
            "profile_kernel": us(4 * N + 16 * groups), "summary_kernel": us(8 * n * pm.T), "match_kernel": us(strip_bytes + 32 * pairs)}
    return each, ops, pairs


def step_calls(a, say):
    import torch
    say("# ubu_match, 3 x %d x %d = %d pixels, slots %d, min_pixels %d, time_bin 1, adc_scale %d; us per call: median (spread) over %d "
        "alternating repetitions of %d back-to-back calls over %d rotated operand sets, device events; byte bound at %.1f TB/s"
        % (ROWS, COLS, N, a.slots, MIN_PIXELS, SCALE, a.reps, CALLS, SETS, HBM_TBS))
    for kind in KINDS:
        sets = _sets(kind, a.slots)
        res = _timed({"ubu_match": lambda i: sets[i % SETS][2](*sets[i % SETS][:2])}, a.reps)
        found, view, pm = sets[0]
        m = pm(found, view)
        torch.cuda.synchronize()
        each, ops, pairs = _bounds(found, view, pm, m)
        t, s = res["ubu_match"]
        say("%-10s %-10s clusters = %6d candidates = %4d pairs = %6d status = %s  %8.1f us (spread %.1f)  byte bound %5.1f us -> %.2fx the bound"
            % ("ubu_match", kind, int(found.count.item()), int(m.ncand.item()), pairs, m.status.tolist(), t, s, sum(each.values()), t / sum(each.values())))


def step_launches(a, say):
    import torch
    from torch.profiler import ProfilerActivity, profile
    say("# each launch of ubu_match alone: mean us over %d calls from the kernel records of torch.profiler, %d rotated operand sets; its "
        "byte bound at %.1f TB/s; the match launch also against its min-add operations at %.0f T op/s" % (2 * SETS, SETS, HBM_TBS, OPS_TOPS))
    for kind in KINDS:
        sets = _sets(kind, a.slots)
        for i in range(SETS):
            sets[i][2](*sets[i][:2])
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for i in range(2 * SETS):
                m = sets[i % SETS][2](*sets[i % SETS][:2])
            torch.cuda.synchronize()
        found, view, pm = sets[(2 * SETS - 1) % SETS]
        each, ops, pairs = _bounds(found, view, pm, m)
        for kernel in KERNELS:
            got = None
            for ev in prof.key_averages():
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = getattr(ev, "cuda_time_total", 0.0)
                if kernel in ev.key and total > 0:
                    got = total / max(ev.count, 1)
            more = ""
            if kernel == "match_kernel" and got:
                more = "; %.3g min-adds = %.2f us at %.0f T op/s -> %.1fx that" % (ops, ops / (OPS_TOPS * 1e6), OPS_TOPS, got / max(ops / (OPS_TOPS * 1e6), 1e-9))
            say("%-15s %-10s %s  byte bound %6.2f us%s%s" % (kernel, kind, "%9.1f us" % got if got is not None else "not measured (no kernel record)",
                                                            each[kernel], " -> %.2fx the bound" % (got / each[kernel]) if got else "", more))


def _composite(prof, chunk=32):
    """the torch a user would write from the profile: I[i, j] = sum_t min(p_i[t], p_j[t]), in chunks of `chunk` candidates"""
    import torch
    n = prof.shape[0]
    out = torch.empty((n, n), dtype=torch.int64, device=prof.device)
    for i0 in range(0, n, chunk):
        out[i0:i0 + chunk] = torch.minimum(prof[i0:i0 + chunk, None], prof[None]).sum(-1)
    return out


def step_composite(a, say):
    import torch
    say("# the torch composite on the int64 profile [n, T]: minimum(prof[i0:i0+32, None], prof[None]).sum(-1) in a chunk loop (the unchunked "
        "form materialises n^2 T integers); I alone, without the shared bins and the profile itself; us per call: median (spread) over %d "
        "repetitions of 2 calls" % a.reps)
    for kind in KINDS:
        sets = _sets(kind, a.slots)
        profs = []
        for found, view, pm in sets:
            m = pm(found, view)
            n = min(int(m.ncand.item()), pm.slots)
            profs.append((m.profile[:n].to(torch.int64) & 0xFFFFFFFF).contiguous())
        res = _timed({"torch composite": lambda i: _composite(profs[i % SETS]), "ubu_match": lambda i: sets[i % SETS][2](*sets[i % SETS][:2])}, a.reps, 2)
        found, view, pm = sets[0]
        m, want = pm(found, view), _composite(profs[0])
        n = profs[0].shape[0]
        upper = torch.triu(torch.ones((n, n), dtype=torch.bool, device="cuda"), 1) & (m.candidates[:n, 1][:, None] != m.candidates[:n, 1][None])
        same = bool((m.pairs[:n, :n, 1][upper] == want[upper]).all())
        for k, (t, s) in res.items():
            say("%-16s %-10s n = %4d %10.1f us (spread %.1f)" % (k, kind, n, t, s))
        say("the composite's I equals ubu_match's on the pairs of two planes: %s; the whole of ubu_match is x%.1f faster than this part" % (same, res["torch composite"][0] / res["ubu_match"][0]))


def step_host(a, say):
    import time
    import torch
    say("# the same tables on the host: the %.1f MB download of ids and the view into pinned memory and of the cluster table, then numpy "
        "(np.add.at, whole-array minimum); ms per event, median (spread) over %d events" % (8 * N * 1e-6, a.reps))
    h_ids = torch.empty((P, ROWS, COLS), dtype=torch.int32).pin_memory()
    h_view = torch.empty((P, ROWS, COLS), dtype=torch.float32).pin_memory()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import match_ref
    for kind in KINDS:
        found, view, pm = _sets(kind, a.slots)[0]
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_ids.copy_(found.ids, non_blocking=True)
            h_view.copy_(view, non_blocking=True)
            count = int(found.count.item())
            table = found.table[:min(count, pm.capacity)].cpu()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ref = match_ref.match(h_ids.numpy(), table.numpy(), count, pm.capacity, h_view.numpy(), SCALE, MIN_PIXELS, 1, (0,) * P, a.slots)
            times.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
        tot, dl = [t[0] for t in times], [t[1] for t in times]
        say("host %-10s candidates = %4d  %9.1f ms (spread %.1f), of which the download %6.2f ms" % (kind, ref["ncand"], statistics.median(tot),
                                                                                                max(tot) - min(tot), statistics.median(dl)))


def step_events(a, say):
    import torch
    from ubresnet_amd import clusters, deploy, planes
    torch.manual_seed(7)
    model = deploy.load_model(None, "cuda:0", num_classes=NCLASS)
    g = torch.Generator(device="cuda").manual_seed(13)
    seeds = (torch.rand((P, 1, ROWS, COLS), device="cuda", generator=g) < 0.013 / 81).float()
    view = torch.where(torch.nn.functional.max_pool2d(seeds, 9, 1, 4) > 0, 50.0, 0.0).contiguous()
    seg = deploy.WholeViewSegmenter(model, rows=ROWS, cols=COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float16, use_graph=True,
                                    output="products")
    cl = clusters.EventClusterer(P, ROWS, COLS, NCLASS, 8, False, 255, CAPACITY, "cuda:0")
    pm = planes.PlaneMatcher(cl, a.slots, MIN_PIXELS, 1, None, SCALE)
    legs = {"products + cl": lambda i: cl(seg(view)), "products + cl + pm": lambda i: pm(cl(seg(view)), view)}
    res = _timed(legs, a.reps, a.events)
    m = pm(cl(seg(view)), view)
    say("# UResNet ip16 nc4, 3 x %d x %d event = %d tiles of %d x %d, f16, batch %d, hipGraph replay, 1.3 %% lit: %d clusters, %d candidates, "
        "status %s" % (ROWS, COLS, seg.tiles_per_event, TH, TW, BATCH, int(cl.count.item()), int(m.ncand.item()), m.status.tolist()))
    say("# events/s on the device: median (spread) over %d alternating repetitions of %d events" % (a.reps, a.events))
    eps = {}
    for k, (t, s) in res.items():
        eps[k] = (1e6 / t, 1e6 / (t - s / 2) - 1e6 / (t + s / 2))
        say("%-20s %7.2f events/s (spread %.2f)  %8.1f us/event" % (k, eps[k][0], eps[k][1], t))
    (d, ds), (z, zs) = eps["products + cl"], eps["products + cl + pm"]
    say("the matcher behind the clusterer: x%.3f of the leg without, %+.1f us per event (combined spread of the rates %.2f events/s)"
        % (z / d, res["products + cl + pm"][0] - res["products + cl"][0], ds + zs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", type=int, default=2048)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(LIMITS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    steps = {"calls": step_calls, "launches": step_launches, "composite": step_composite, "host": step_host, "events": step_events}
    if a.step:
        steps[a.step](a, lambda s: print(s, flush=True))
        return 0
    out = open(a.out, "w") if a.out else None
    head = "# python tools/matchbench.py --events %d --reps %d --slots %d\n" % (a.events, a.reps, a.slots)
    print(head, end="", flush=True)
    if out:
        out.write(head)
    rc = 0
    for step in steps:
        cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--events", str(a.events),
               "--reps", str(a.reps), "--slots", str(a.slots)]
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
