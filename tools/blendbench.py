#!/usr/bin/env python3
"""Overlap-tile inference (libubresnet_blend.so, deploy.WholeViewSegmenter(margin=, blend=)): the two launches against their byte
bounds and against the torch composite a user would write instead, events/s of a full-size fp16 UResNet event (3 x 1008 x 3456,
tiles of 512 x 832, batch 10, hipGraph replay) for margin 0 / None, 64 / None, 64 / "linear" and 64 / "hann", the worst
error-to-bound ratio of the blend over the cases of tests/blend_ref.py, and the seam effect on a view the network accepts whole.

    python tools/blendbench.py [--events N] [--reps R] [--out FILE]

Four steps, each a fresh child process under its own time limit; the first step that fails or runs out of time ends the run
(nothing is tried again):

  exact    every case of tests/blend_ref.py (those of tests/test_gpu_blend_exact.py) on the device against the fp64 reference:
           the worst |error| / bound.
  kernel   ubv_blend_tiles on 10 tiles x 4 classes x 512 x 832 (one chunk's log-probabilities, 68 MB: the first ten tiles of the
           margin-64 tiling of the event, with the "linear" tables) into a 3 x 4 x 1008 x 3456 buffer, and ubv_blend_begin on that
           buffer, against their byte bounds at HBM_TBS and against torch (logaddexp over slices; fill_).  Four operand sets are
           rotated so that a launch does not find its operands in the 256 MB Infinity Cache.
  events   events/s of the four settings with output="scores", and of products with "linear", alternated in one process, the
           result left on the device.  Device events around `--events` events per repetition after warm-up; median and spread
           (max - min) over the repetitions; each leg against the margin 0 / None leg of the same run.
  seam     UResNet ip16 nc3 with SEEDED weights, fp32, a 3 x 480 x 736 view (the network accepts it whole), tiles of 256 x 256
           (2 x 3 at margin 0, 3 x 5 at margin 64): max and mean |log p| difference to the single whole-view forward over the lit pixels, for the same
           four settings.  Reported as measured; not a claim about trained weights.
"""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROWS, COLS, TH, TW, P, NCLASS, BATCH, MARGIN = 1008, 3456, 512, 832, 3, 4, 10, 64
HBM_TBS = 6.0           # the HBM rate the project states its byte bounds against (TB/s)
LIMITS = {"exact": 240, "kernel": 300, "events": 480, "seam": 240}      # seconds per step
SETTINGS = (("margin 0 / None", 0, None), ("margin 64 / None", MARGIN, None), ("margin 64 / linear", MARGIN, "linear"),
            ("margin 64 / hann", MARGIN, "hann"))


def step_exact(a, say):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import blend_ref as R
    from ubresnet_amd import _blend as V
    from ubresnet_amd import _lib as L
    worst, at, elements = 0.0, None, 0
    for name, c in R.CASES.items():
        host = R.case_inputs(name)
        Pn, rows, cols = c["view"]
        th, tw = c["tile"]

        def dev(arr):
            full = torch.empty(arr.size + 64 + c["offset"], dtype=torch.float32, device="cuda")
            t = full[64 + c["offset"]:].view(arr.shape)
            t.copy_(torch.from_numpy(arr))
            return t

        out = dev(np.zeros((Pn, c["C"], rows, cols), np.float32))
        V.blend_begin(out.data_ptr(), out.numel(), L.stream_ptr())
        keep = []
        for logp, desc, lwr, lwc in host:
            keep.append((dev(logp), dev(lwr), dev(lwc)))
            V.blend_tiles(keep[-1][0].data_ptr(), c["C"], th, tw, V.desc3(desc), len(desc), keep[-1][1].data_ptr(), keep[-1][2].data_ptr(),
                          out.data_ptr(), Pn, rows, cols, L.stream_ptr())
        torch.cuda.synchronize()
        ref, lim, count = R.blend(np.full((Pn, c["C"], rows, cols), -np.inf, np.float32), host)
        fin = np.isfinite(ref) & (lim > 0)
        ratio = np.abs(out.cpu().numpy().astype(np.float64)[fin] - ref[fin]) / lim[fin]
        elements += int(fin.sum())
        if float(ratio.max()) > worst:
            worst, at = float(ratio.max()), name
    say("# ubv_blend_tiles against the fp64 reference and the derived bound of tests/blend_ref.py (2 ulp per expf / log1pf, half an ulp per add)")
    say("worst |error| / bound over %d cases, %d elements: %.3f  (%s)" % (len(R.CASES), elements, worst, at))


def _time_us(torch, fn, nset, reps_n=40, reps=5):
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
    import torch
    from ubresnet_amd import _blend as V
    from ubresnet_amd import _lib as L
    from ubresnet_amd import deploy
    nset = 4
    ro, co = deploy.margin_tiling(ROWS, COLS, TH, TW, MARGIN)
    tiles = deploy.view_tiles(ROWS, COLS, P, TH, TW, False, MARGIN)[:BATCH]
    lr = V.axis_log_weights(ro, TH, ROWS, MARGIN, "linear")
    lc = V.axis_log_weights(co, TW, COLS, MARGIN, "linear")
    lwr = torch.tensor([r for r in lr for _ in co][:BATCH], dtype=torch.float64).float().cuda()
    lwc = torch.tensor([c for _ in ro for c in lc][:BATCH], dtype=torch.float64).float().cuda()
    cover = torch.zeros((ROWS, COLS), dtype=torch.int32)
    for (_, r0, c0, *_) in tiles:
        cover[r0:r0 + TH, c0:c0 + TW] += 1
    covered, visits = int((cover > 0).sum()), int(cover.sum())
    g = torch.Generator(device="cuda").manual_seed(3)
    logp = [torch.log_softmax(torch.randn((BATCH, NCLASS, TH, TW), device="cuda", generator=g) * 4, 1) for _ in range(nset)]
    outs = [torch.full((P, NCLASS, ROWS, COLS), float("-inf"), device="cuda") for _ in range(nset)]
    desc = V.desc3(tiles)

    def blend(i):
        V.blend_tiles(logp[i % nset].data_ptr(), NCLASS, TH, TW, desc, BATCH, lwr.data_ptr(), lwc.data_ptr(), outs[i % nset].data_ptr(),
                      P, ROWS, COLS, L.stream_ptr())

    def torch_blend(i):
        o, x = outs[i % nset], logp[i % nset]
        for t, (p, r0, c0, *_) in enumerate(tiles):
            s = o[p, :, r0:r0 + TH, c0:c0 + TW]
            torch.logaddexp(s, x[t] + (lwr[t][:, None] + lwc[t][None, :]), out=s)

    def begin(i):
        V.blend_begin(outs[i % nset].data_ptr(), outs[0].numel(), L.stream_ptr())

    def torch_begin(i):
        outs[i % nset].fill_(float("-inf"))

    tile_bytes = BATCH * NCLASS * TH * TW * 4
    blend_bytes = tile_bytes + covered * NCLASS * 8
    say("# ubv_blend_tiles: %d tiles x %d classes x %d x %d fp32 (%.1f MB) of the margin-%d tiling, %d view pixels covered, %d tile pixels "
        "(%.2f per covered pixel); bytes = the tiles once + 8 per covered pixel and class = %.1f MB.  Four operand sets rotated; us per "
        "call: median (spread) over 5 repetitions of 40 back-to-back calls, device events, alone on the device; byte bounds at %.1f TB/s"
        % (BATCH, NCLASS, TH, TW, tile_bytes * 1e-6, MARGIN, covered, visits, visits / covered, blend_bytes * 1e-6, HBM_TBS))
    begin_bytes = outs[0].numel() * 4
    for name, fn, nbytes in (("ubv_blend_tiles", blend, blend_bytes), ("torch: logaddexp over %d slices" % BATCH, torch_blend, blend_bytes),
                             ("ubv_blend_begin (%.0f MB)" % (begin_bytes * 1e-6), begin, begin_bytes), ("torch: fill_(-inf)", torch_begin, begin_bytes)):
        for o in outs:
            o.fill_(float("-inf"))
        t, s = _time_us(torch, fn, nset)
        bound = nbytes / (HBM_TBS * 1e12) * 1e6
        say("%-34s %8.1f us (spread %.1f)  byte bound %6.1f us  -> %.2fx the bound, %.2f TB/s" % (name, t, s, bound, t / bound, nbytes / (t * 1e-6) * 1e-12))
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
    variants = [("scores", s[0]) for s in SETTINGS] + [("products", SETTINGS[0][0]), ("products", SETTINGS[2][0])]
    by_name = {s[0]: s for s in SETTINGS}
    segs = {v: deploy.WholeViewSegmenter(m, output=v[0], margin=by_name[v[1]][1], blend=by_name[v[1]][2], **kw) for v in variants}

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
    say("# UResNet ip16 nc4, 3 x %d x %d event, tiles of %d x %d, f16, batch %d, hipGraph replay, result left on the device" % (ROWS, COLS, TH, TW, BATCH))
    say("# events/s: median (spread = max - min) over %d alternating repetitions of %d events = %d timed events per line" % (a.reps, a.events, a.reps * a.events))
    med = {v: (statistics.median(runs[v]), max(runs[v]) - min(runs[v])) for v in variants}
    for v in variants:
        base = med[(v[0], SETTINGS[0][0])][0]
        tiles = segs[v].tiles_per_event
        say("%-9s %-19s %3d tiles  %7.2f events/s (spread %.2f)  %6.2f ms/event = x%.3f of margin 0 / None (tiles: x%.3f)   runs: %s"
            % (v[0], v[1], tiles, med[v][0], med[v][1], 1e3 / med[v][0], base / med[v][0], tiles / segs[(v[0], SETTINGS[0][0])].tiles_per_event,
               " ".join("%.2f" % x for x in runs[v])))


def step_seam(a, say):
    import numpy as np
    import torch
    from oracle import uresnet_oracle as O
    from ubresnet_amd import deploy, synthetic
    rows, cols, th, tw = 480, 736, 256, 256          # overlaps of 144 and 136 at margin 64: wider than 2 * margin, so the ramps meet
    sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
    m = deploy.load_model(None, "cuda:0", num_classes=3, state_dict=sd)
    adc = np.zeros((P, 1, rows, cols), np.float32)
    for p in range(P):
        adc[p, 0] = synthetic.make_crop(rows, cols, 7000 + p)[0]
    view = torch.from_numpy(adc).cuda()
    m.compute_dtype = torch.float32
    with torch.no_grad():
        whole = m(view).double()
    m.compute_dtype = None
    lit = (view[:, 0] > 10.0)[:, None].expand_as(whole)
    say("# UResNet ip16 nc3, SEEDED weights (not trained), fp32; view 3 x %d x %d (%d lit pixels), tiles of %d x %d, batch 6; |log p| difference "
        "to the single whole-view forward over the lit pixels, all classes" % (rows, cols, int(lit[:, 0].sum()), th, tw))
    for name, margin, blend in SETTINGS:
        seg = deploy.WholeViewSegmenter(m, rows, cols, planes=P, tile=(th, tw), batch=6, dtype=torch.float32, margin=margin, blend=blend)
        d = (seg(view).double() - whole).abs()[lit]
        say("%-19s %3d tiles   max %.3e   mean %.3e" % (name, seg.tiles_per_event, float(d.max()), float(d.mean())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(LIMITS), help="run one step in this process (what the driver starts)")
    a = ap.parse_args()
    if a.events * a.reps < 20:
        ap.error("at least 20 timed events per variant (--events x --reps)")
    steps = {"exact": step_exact, "kernel": step_kernel, "events": step_events, "seam": step_seam}
    if a.step:
        steps[a.step](a, lambda s: print(s, flush=True))
        return 0
    out = open(a.out, "w") if a.out else None
    rc = 0
    for step in ("exact", "kernel", "events", "seam"):
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
