#!/usr/bin/env python3
"""ASPP_ResNet whole-view inference: tiles/s of a stacked 3 x 1008 x 3456 event (10 tiles of 3 x 512 x 832, fp16, one hipGraph
replay per event) and the per-launch breakdown of one batch.

    python tools/aspp_inferprobe.py [--fold 0|1] [--front fused|split] [--events N] [--reps R] [--out FILE]
    python tools/aspp_inferprobe.py --compare [--out FILE]      # the three schedules alternated in one process

  --fold 0        eval forward on the training schedule (BatchNorm on load, separate block tails; UBR_INFER_FOLD=0)
  --fold 1        Engine.aspp_infer (BatchNorm folded into the packed weights)
  --front split   probe-only: an ASPP level's front as five launches (four ops.conv + ops.maxpool_fwd) reading the SAME folded
                  weights and biases as the fused ubr_aspp_front launch -- what the fused kernel has to beat

Event timing, launch profiler off while tiles/s is measured; every repetition times `--events` events after warm-up, and the
spread is max - min over the repetitions.  The breakdown is a separate eager pass with the launch profiler on."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ubresnet_amd import deploy, engine, ops, synthetic

ROWS, COLS, TH, TW, P = 1008, 3456, 512, 832, 3
HBM_TBS = 6.29          # achievable HBM bandwidth the byte bounds are stated against (TB/s)
_FUSED = ops.aspp_front


def split_front(e, wp, bias, acat):
    """the five launches ubr_aspp_front replaces, on the same packed image: B1 | B2 | B3 | B4 | pool"""
    Cn = e.shape[3]
    t0 = 0
    for b, (k, dil) in enumerate(((1, 1), (3, 1), (3, 3), (3, 5))):
        ops.conv(e, wp[t0:t0 + k * k], acat[..., 16 * b:16 * b + 16], ops.conv_taps(k, dil, dil * (k // 2)), 16,
                 bias=bias[16 * b:16 * b + 16], act=1)
        t0 += k * k
    ops.maxpool_fwd(e, None, acat[..., 64:64 + Cn], None, 1)


def configure(fold, front):
    engine._INFER_FOLD = bool(fold)
    ops.aspp_front = _FUSED if front == "fused" else split_front


def build(fold, front, view, batch=10):
    """a segmenter whose graph is captured under (fold, front); replays no longer depend on the switches"""
    configure(fold, front)
    try:
        torch.manual_seed(7)
        m = deploy.load_model(None, "cuda:0", num_classes=3, input_channels=3, arch="aspp")
        seg = deploy.WholeViewSegmenter(m, ROWS, COLS, planes=P, tile=(TH, TW), batch=batch, dtype=torch.float16, use_graph=True)
        seg(view)
        torch.cuda.synchronize()
    finally:
        configure(1, "fused")
    return seg


def time_events(seg, view, events):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(events):
        seg(view)
    e1.record()
    torch.cuda.synchronize()
    return seg.tiles_per_event * events / (e0.elapsed_time(e1) * 1e-3)


def breakdown(fold, front, say, batch=10):
    configure(fold, front)
    torch.manual_seed(7)
    m = deploy.load_model(None, "cuda:0", num_classes=3, input_channels=3, arch="aspp")
    m.compute_dtype = torch.float16
    x = torch.from_numpy(synthetic.make_batch(batch, TH, TW, 1000, planes=P)[0]).cuda()
    with torch.no_grad():
        m(x)
        torch.cuda.synchronize()
        prof = ops.LaunchProfiler()
        ops._prof = prof
        try:
            m(x)
            agg = prof.summary(by="shape")
        finally:
            ops._prof = None
            configure(1, "fused")
    tot = sum(a[1] for a in agg.values())
    say("# per-launch breakdown, fold=%d front=%s, one batch of %d tiles, eager with the launch profiler: %d operator calls, %.3f ms"
        % (fold, front, batch, sum(a[0] for a in agg.values()), tot * 1e3))
    say("# %-12s %-58s %5s %9s %8s %8s" % ("op", "shapes", "calls", "us", "GB", "TB/s"))
    for (name, sig), a in sorted(agg.items(), key=lambda kv: -kv[1][1])[:24]:
        say("  %-12s %-58s %5d %9.1f %8.3f %8.2f" % (name, sig[:58], a[0], a[1] * 1e6, a[2] * 1e-9, a[2] / max(a[1], 1e-12) * 1e-12))
    if not fold:
        return
    # an ASPP level's front (one fused launch, or the five launches of --front split) against its byte bound: e read once,
    # the (64 + C)-channel concat tensor written once, the 28-tap weight image read once
    for lvl, Cn in ((3, 128), (4, 256), (5, 512)):
        h, w = TH >> lvl, TW >> lvl
        e = "%dx%dx%dx%d" % (batch, h, w, Cn)
        sec, n = 0.0, 0
        for (name, sig), a in agg.items():
            t = sig.split()
            mine = (name == "aspp_front" and t[0] == e) or (name == "conv" and t[0] == e and t[2] == "%dx%dx%dx16" % (batch, h, w)) \
                or (name == "maxpool_fwd" and t[0] == e and t[1] == e)
            if mine:
                sec, n = sec + a[1], n + a[0]
        nbytes = 2 * (batch * h * w * (Cn + 64 + Cn) + 28 * Cn * 16)
        bound = nbytes / (HBM_TBS * 1e12)
        say("  front of level %d (%s, %d launch%s): %8.1f us, byte bound %5.1f us at %.2f TB/s (%.0f%% of the bound's rate)"
            % (lvl, e, n, "" if n == 1 else "es", sec * 1e6, bound * 1e6, HBM_TBS, 100 * bound / max(sec, 1e-12)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fold", type=int, default=1, choices=[0, 1])
    ap.add_argument("--front", default="fused", choices=["fused", "split"])
    ap.add_argument("--compare", action="store_true", help="alternate fold 0 | fold 1 split | fold 1 fused in one process")
    ap.add_argument("--events", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-breakdown", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.fold == 0 and a.front == "split":
        ap.error("--front split needs the folded weights (--fold 1)")
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    adc = np.zeros((P, 1, ROWS, COLS), np.float32)
    for p in range(P):
        adc[p, 0] = synthetic.make_crop(ROWS, COLS, 5000 + p)[0]
    view = torch.from_numpy(adc).cuda()
    cfgs = [(0, "fused"), (1, "split"), (1, "fused")] if a.compare else [(a.fold, a.front)]
    names = {(0, "fused"): "(a) training schedule in eval mode (fold 0)", (1, "split"): "(b) folded, front split in five launches",
             (1, "fused"): "(c) folded, front fused (ubr_aspp_front)"}
    segs = [build(f, fr, view) for f, fr in cfgs]
    for s in segs:                       # warm-up of every graph
        time_events(s, view, 2)
    runs = [[] for _ in cfgs]
    for _ in range(max(a.reps, 1)):
        for i, s in enumerate(segs):     # alternating
            runs[i].append(time_events(s, view, a.events))
    say("# ASPP_ResNet ip16, stacked 3 x %d x %d event = %d tiles of 3 x %d x %d, f16, hipGraph replay; tiles/s: median (spread = max - min) "
        "over %d alternating repetitions of %d events" % (ROWS, COLS, segs[0].tiles_per_event, TH, TW, len(runs[0]), a.events))
    med = []
    for c, r in zip(cfgs, runs):
        med.append((statistics.median(r), max(r) - min(r)))
        say("%-48s %8.1f tiles/s (spread %.1f)   runs: %s" % (names[c], med[-1][0], med[-1][1], " ".join("%.1f" % v for v in r)))
    if a.compare:
        (ta, sa), (tb, sb), (tc, sc) = med
        say("(c) vs (a): x%.3f, %+.1f tiles/s against a combined spread of %.1f -> %s" % (tc / ta, tc - ta, sa + sc, "FASTER" if tc - ta > sa + sc else "NOT faster beyond the spreads"))
        say("(c) vs (b): x%.3f, %+.1f tiles/s against a combined spread of %.1f -> %s" % (tc / tb, tc - tb, sb + sc, "FASTER" if tc - tb > sb + sc else ("SLOWER" if tb - tc > sb + sc else "level within the spreads")))
    if not a.no_breakdown:
        del segs
        for c in cfgs:
            breakdown(c[0], c[1], say)
    if out:
        out.close()


if __name__ == "__main__":
    main()
