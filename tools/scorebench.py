#!/usr/bin/env python3
"""EventScorer (libubresnet_score.so): ubq_score_event alone against its byte bound and against the torch composite a user would
write instead, and events/s of a full-size fp16 UResNet event (3 x 1008 x 3456 = 30 tiles of 512 x 832, batch 10, hipGraph
replay, output="products") with and without scorer.add().

    python tools/scorebench.py [--events N] [--reps R] [--out FILE]

Two steps, each a fresh child process under its own time limit; the first step that fails or runs out of time ends the run
(nothing is tried again):

  kernel   one 3 x 1008 x 3456 event per call, C = 4, 10 bins, interface_from = 1: both truth types, radius 0 / 2 / 8, on operand
           A (a synthetic event, about 2 % of the pixels lit, labels right on 90 % of them) and operand B (every pixel lit, one
           class, one confidence: every lane of every wave counts into the same words).  Operand sets are rotated so that a
           call does not find its image in the 256 MB Infinity Cache.  The byte bound at HBM_TBS is 3 B per pixel of label and
           confidence plus 1 or 8 B of truth.  Then the torch composite (masks, max_pool2d for the window, bincount for the
           confusion, the reliability sums) on operand A.
  events   events/s with output="products", with and without scorer.add() behind every event, alternated in one process, the
           result left on the device.  Device events around `--events` events per repetition after warm-up; median and spread
           (max - min) over the repetitions.
"""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROWS, COLS, TH, TW, P, NCLASS, BATCH = 1008, 3456, 512, 832, 3, 4, 10
BINS, FROM = 10, 1
HBM_TBS = 6.0           # the HBM rate the project states its byte bounds against (TB/s)
LIMITS = {"kernel": 400, "events": 420}      # seconds per step


def synthetic_event(seed0):
    """-> adc float32 [P,1,rows,cols], truth int64 [P,rows,cols]: one synthetic.make_crop per plane"""
    import numpy as np
    from ubresnet_amd import synthetic
    adc = np.zeros((P, 1, ROWS, COLS), np.float32)
    truth = np.zeros((P, ROWS, COLS), np.int64)
    for p in range(P):
        adc[p, 0], truth[p], _ = synthetic.make_crop(ROWS, COLS, seed0 + p)
    return adc, truth


def time_us(fn, nset, reps_n=40, reps=5):
    import torch
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


def step_kernel(a, say):
    import numpy as np
    import torch
    from ubresnet_amd import _score as S
    from ubresnet_amd import scoring
    nset = 8
    px = P * ROWS * COLS
    adc, truth = synthetic_event(5000)
    rs = np.random.RandomState(1)
    lit = adc[:, 0] > 10.0
    wrong = rs.uniform(size=truth.shape) < 0.1
    label = np.where(lit, np.where(wrong, rs.randint(0, NCLASS, truth.shape), truth), 255).astype(np.uint8)
    conf = np.where(lit, rs.uniform(0.3, 1.0, truth.shape), 0.0).astype(np.float16)
    A = dict(label=torch.from_numpy(label).cuda(), conf=torch.from_numpy(conf).cuda(), i64=torch.from_numpy(truth).cuda())
    A["u8"] = A["i64"].to(torch.uint8)
    B = dict(label=torch.zeros((P, ROWS, COLS), dtype=torch.uint8, device="cuda"),
             conf=torch.full((P, ROWS, COLS), 0.75, dtype=torch.float16, device="cuda"),
             i64=torch.zeros((P, ROWS, COLS), dtype=torch.int64, device="cuda"))
    B["u8"] = B["i64"].to(torch.uint8)

    def sets(op, roll):
        """nset copies of the operand, each rolled by another offset so that no two calls read the same image"""
        return [dict((k, torch.roll(v, (17 * i, 131 * i), (1, 2)).contiguous() if roll else v.clone()) for k, v in op.items())
                for i in range(nset)]

    ops = {"A": sets(A, True), "B": sets(B, False)}
    edges = scoring.equal_width_edges(BINS)
    edges_c = S.edges_array(edges)
    words = S.table_words(P, NCLASS, BINS)
    table = torch.zeros(words, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(op, kind, radius):
        tk = "u8" if kind == S.TRUTH_U8 else "i64"

        def fn(i):
            o = ops[op][i % nset]
            S.score_event(o["label"].data_ptr(), o["conf"].data_ptr(), o[tk].data_ptr(), kind, NCLASS, 255, radius, FROM, edges_c,
                          BINS, table.data_ptr(), P, ROWS, COLS, st)
        return fn

    def composite(radius, tk):
        C2 = NCLASS * NCLASS

        def fn(i):
            o = ops["A"][i % nset]
            lab, tr, cf = o["label"].long(), o[tk].long(), o["conf"].float()
            valid = (tr >= 0) & (tr < NCLASS)
            scored = (lab != 255) & valid & (lab < NCLASS)
            s = torch.zeros_like(scored)
            if radius > 0:
                for c in range(FROM, NCLASS):
                    near = torch.nn.functional.max_pool2d((tr == c).float()[None], 2 * radius + 1, 1, radius)[0] > 0
                    s |= near & valid & (tr >= FROM) & (tr != c)
            key = (s.long() * C2 + tr * NCLASS + lab)[scored]
            cm = torch.bincount(key, minlength=2 * C2)
            b = torch.clamp((cf[scored] * BINS).long(), max=BINS - 1) + BINS * s[scored].long()
            n = torch.bincount(b, minlength=2 * BINS)
            ok = torch.bincount(b, weights=(lab[scored] == tr[scored]).double(), minlength=2 * BINS)
            sm = torch.bincount(b, weights=cf[scored].double(), minlength=2 * BINS)
            dark = ((lab == 255) & valid & (tr >= 1)).sum()
            return cm, n, ok, sm, dark
        return fn

    lit_share = float(lit.mean())
    say("# one %d x %d x %d event per call (%.1f Mpixel, %.2f %% lit in operand A), C = %d, %d bins, interface_from = %d; %d operand sets "
        "rotated; us per call: median (spread) over 5 repetitions of 40 back-to-back calls, device events, alone on the device; byte "
        "bounds at %.1f TB/s" % (P, ROWS, COLS, px * 1e-6, 100 * lit_share, NCLASS, BINS, FROM, nset, HBM_TBS))
    for op in ("A", "B"):
        for kind, tk, per in ((S.TRUTH_U8, "uint8", 4), (S.TRUTH_I64, "int64", 11)):
            for radius in (0, 2, 8):
                t, sp = time_us(call(op, kind, radius), nset)
                bound = px * per / (HBM_TBS * 1e12) * 1e6
                say("ubq_score_event operand %s truth %-5s radius %d  %8.1f us (spread %.1f)  %2d B/pixel  byte bound %5.1f us  -> %.2fx the "
                    "bound, %.2f TB/s" % (op, tk, radius, t, sp, per, bound, t / bound, px * per / (t * 1e-6) * 1e-12))
    for tk in ("u8", "i64"):
        for radius in (0, 2):
            t, sp = time_us(composite(radius, tk), nset, reps_n=5)
            say("torch composite     operand A truth %-5s radius %d  %8.1f us (spread %.1f)" % ("uint8" if tk == "u8" else "int64", radius, t, sp))
    say("# (the composite: masks, max_pool2d per class for the window, bincount for the confusion and the reliability sums in "
        "float64; it bins by multiplication, not by half edges, and its sums are not reproducible)")


def step_events(a, say):
    import torch
    from ubresnet_amd import deploy, scoring
    torch.manual_seed(7)
    m = deploy.load_model(None, "cuda:0", num_classes=NCLASS)
    adc, truth = synthetic_event(5000)
    view, truth = torch.from_numpy(adc).cuda(), torch.from_numpy(truth).cuda()
    seg = deploy.WholeViewSegmenter(m, rows=ROWS, cols=COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=torch.float16,
                                    use_graph=True, output="products")
    scorer = scoring.EventScorer(num_classes=NCLASS, planes=P, bins=BINS, radius=2, interface_from=FROM, capacity=max(a.events, 2))
    variants = ("products", "products + scorer.add")

    def run(v, events):
        scorer.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(events):
            prod = seg(view)
            if v != "products":
                scorer.add(prod, truth)
        e1.record()
        torch.cuda.synchronize()
        return events / (e0.elapsed_time(e1) * 1e-3)

    for v in variants:
        run(v, 2)
    runs = {v: [] for v in variants}
    for _ in range(a.reps):
        for v in variants:                # alternating
            runs[v].append(run(v, a.events))
    say("# UResNet ip16 nc4, 3 x %d x %d event = %d tiles of %d x %d, f16, batch %d, hipGraph replay, output=\"products\", result left "
        "on the device; EventScorer(bins=%d, radius=2, interface_from=%d), int64 truth" % (ROWS, COLS, seg.tiles_per_event, TH, TW, BATCH, BINS, FROM))
    say("# events/s: median (spread = max - min) over %d alternating repetitions of %d events = %d timed events per line"
        % (a.reps, a.events, a.reps * a.events))
    med = {v: (statistics.median(runs[v]), max(runs[v]) - min(runs[v])) for v in variants}
    for v in variants:
        say("%-22s %7.2f events/s (spread %.2f)  %6.2f ms/event   runs: %s"
            % (v, med[v][0], med[v][1], 1e3 / med[v][0], " ".join("%.2f" % x for x in runs[v])))
    d = med[variants[0]][0] - med[variants[1]][0]
    say("difference %.2f events/s against spreads of %.2f and %.2f: %s" % (d, med[variants[0]][1], med[variants[1]][1],
        "below the spread, nothing is claimed" if abs(d) <= max(med[variants[0]][1], med[variants[1]][1]) else "above the spread"))
    print(scorer.read(), file=sys.stderr)


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
