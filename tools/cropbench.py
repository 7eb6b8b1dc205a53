#!/usr/bin/env python3
"""Event crops (libubresnet_crop.so) on full-size views, 3 x 1008 x 3456, K = 16 crops of 512 x 512 and 512 x 832: the launches
alone against their byte bounds, the torch composite a user would write without them, what the sampler buys in lit pixels per
crop, and batches/s of EventCropStager against BatchStager.

    python tools/cropbench.py [--events N] [--reps R] [--batches B] [--steps S] [--only-train-leg LEG] [--out FILE]

Legs are alternated; a figure is the median (spread = max - min) over `--reps` repetitions of 50 back-to-back calls between
device events; the operand sets (two views) rotate from call to call.

  calls      ubn_occupancy without and with a class mask, ubn_choose, ubn_gather, each alone, against its byte bound at HBM_TBS
  composite  what a user would write in torch: host-drawn offsets, slices, stack, flip, .to(int64)
  sampler    from the tables of `--events` seeded synthetic events (exact integers): mean lit pixels and pixels of the rarest
             class per crop for min_lit = 0 against a min_lit and against classes = {rarest}
  stagers    batches/s of EventCropStager from pinned host events, dense and sparse, against BatchStager on pre-cropped
             synthetic batches of the same size, served from a cache built before the clock starts
  train      the bf16 16 x 1 x 512 x 512 guarded train step fed by a resident batch, by BatchStager and by EventCropStager (dense
             and sparse events), in one run: wall clock over --steps steps, alternated; --only-train-leg LEG runs one leg alone
             (what a kernel trace of that leg is taken from)
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

P, ROWS, COLS, K = 3, 1008, 3456, 16
NENTRIES = 64          # entries of the pre-cropped loader, all cached before a timed leg
CROPS = ((512, 512), (512, 832))
HBM_TBS = 6.0           # the HBM rate the project states its byte bounds against (TB/s)
CALLS = 50              # back-to-back calls between two device events
MIN_LIT = 4000


def _timed(legs, reps, calls=CALLS):
    """legs: {name: fn(i)}; alternated; -> {name: (median us per call, spread)}"""
    import torch
    for fn in legs.values():
        fn(0)
        fn(1)
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


def _events(n, seed0=4000):
    import torch
    from ubresnet_amd import synthetic
    out = []
    for i in range(n):
        image, label = synthetic.make_labelled_event(P, ROWS, COLS, seed0 + 10 * i)
        out.append((torch.from_numpy(image), torch.from_numpy(label)))
    return out


def step_calls(a, say, views):
    import torch
    from ubresnet_amd import _crop as NL
    from ubresnet_amd import _lib as L
    n = P * ROWS * COLS
    say("# the launches alone, %d x %d x %d = %d pixels (%.1f %% lit), K = %d, uint8 labels; us per call: median (spread) over %d alternating "
        "repetitions of %d back-to-back calls, device events, two views in rotation; byte bounds at %.1f TB/s"
        % (P, ROWS, COLS, n, 100.0 * float((views[0][0] > 10).float().mean()), K, a.reps, CALLS, HBM_TBS))
    for H, W in CROPS:
        g = NL.largest_cell(ROWS, COLS, H, W)
        shape = NL.sat_shape(P, ROWS, COLS, g)
        sats = [torch.empty(shape, dtype=torch.int32, device="cuda") for _ in views]
        tables = [torch.empty((K, 8), dtype=torch.int32, device="cuda") for _ in views]
        outs = [(torch.empty((K, 1, H, W), device="cuda"), torch.empty((K, H, W), dtype=torch.int64, device="cuda"),
                 torch.empty((K, H, W), device="cuda")) for _ in views]
        wgt = [torch.rand((P, ROWS, COLS), device="cuda") for _ in views]
        status = torch.zeros(1, dtype=torch.int64, device="cuda")

        def occ(i, masked):
            im, lb = views[i % 2]
            NL.occupancy(im.data_ptr(), lb.data_ptr() if masked else None, NL.LABEL_U8 if masked else NL.LABEL_NONE, 0, 0b110, False, 10.0,
                         P, ROWS, COLS, g, sats[i % 2].data_ptr(), L.stream_ptr())

        def choose(i):
            NL.choose(sats[i % 2].data_ptr(), P, ROWS, COLS, H, W, g, None, K, 8, MIN_LIT, 5, i, True, True, tables[i % 2].data_ptr(), L.stream_ptr())

        def gather(i):
            im, lb = views[i % 2]
            o = outs[i % 2]
            NL.gather(im.data_ptr(), lb.data_ptr(), NL.LABEL_U8, 0, wgt[i % 2].data_ptr(), False, P, ROWS, COLS, H, W, tables[i % 2].data_ptr(), K,
                      o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), status.data_ptr(), L.stream_ptr())

        for i in (0, 1):
            occ(i, False), choose(i)
        lit = sum(int((v[0] > 10).sum()) for v in views) // 2
        nsat = shape[0] * shape[1] * shape[2]
        # occupancy: the image read once, the table written and walked once more; with a mask the labels of the lit quads are read
        # as well (bounded here by every label); choose: a few table words per try; gather: per output pixel the image (4), the
        # uint8 label (1) and the weight (4) read, image (4), int64 label (8) and weight (4) written
        nbytes = {"ubn_occupancy": 4 * n + 12 * nsat, "ubn_occupancy, mask": 4 * n + n + 12 * nsat, "ubn_choose": 32 * K + 16 * 8 * K,
                  "ubn_gather": K * H * W * (4 + 1 + 4 + 4 + 8 + 4)}
        res = _timed({"ubn_occupancy": lambda i: occ(i, False), "ubn_occupancy, mask": lambda i: occ(i, True), "ubn_choose": choose,
                      "ubn_gather": gather}, a.reps)
        assert int(status) == 0
        for k, (t, s) in res.items():
            bound = nbytes[k] / (HBM_TBS * 1e12) * 1e6
            if k == "ubn_choose":                               # a few KB: one launch's latency, no byte bound to hold it against
                say("%-20s %d x %d  cell %2d  %8.1f us (spread %.1f)  %7.2f KB  one workgroup of %d threads: launch latency" % (k, H, W, g, t, s, nbytes[k] * 1e-3, K))
                continue
            say("%-20s %d x %d  cell %2d  %8.1f us (spread %.1f)  %7.2f MB  byte bound %6.2f us -> %.2fx the bound, %.2f TB/s"
                % (k, H, W, g, t, s, nbytes[k] * 1e-6, bound, t / bound, nbytes[k] / (t * 1e-6) * 1e-12))
        say("# (mean lit pixels of a view: %d; ubn_occupancy is two launches, its figure the pair)" % lit)


def step_composite(a, say, views):
    import numpy as np
    import torch
    from ubresnet_amd import crops
    say("# the torch composite a user would write today against the three calls together (EventCropper, min_lit = 0), per event of K = %d "
        "crops, same timing" % K)
    rs = np.random.RandomState(1)
    for H, W in CROPS:
        cropper = crops.EventCropper(crop=(H, W), per_event=K, min_lit=0, flip_rows=True, flip_cols=True)

        def composite(i):
            im, lb = views[i % 2]
            xs, ls = [], []
            for _ in range(K):
                p, r, c = rs.randint(0, P), rs.randint(0, ROWS - H + 1), rs.randint(0, COLS - W + 1)
                x, l = im[p, r:r + H, c:c + W], lb[p, r:r + H, c:c + W]
                dims = [d for d, on in ((0, rs.randint(0, 2)), (1, rs.randint(0, 2))) if on]
                if dims:
                    x, l = torch.flip(x, dims), torch.flip(l, dims)
                xs.append(x), ls.append(l)
            return torch.stack(xs)[:, None], torch.stack(ls).to(torch.int64), torch.ones((K, H, W), device="cuda")

        res = _timed({"torch composite": composite, "EventCropper": lambda i: cropper(views[i % 2][0], views[i % 2][1], number=i)}, a.reps)
        for k, (t, s) in res.items():
            say("%-20s %d x %d  %8.1f us (spread %.1f)" % (k, H, W, t, s))


def step_sampler(a, say, events):
    import torch
    from ubresnet_amd import crops
    say("# what the sampler buys: %d seeded synthetic events (seeds 4000, 4010, ...), K = %d crops each, tries = 8; exact integers from "
        "the gathered crops" % (len(events), K))
    totals = torch.zeros(3, dtype=torch.int64)
    for _, lb in events:
        totals += torch.bincount(lb.reshape(-1).long(), minlength=3)[:3]
    rare = int(totals[1:].argmin()) + 1
    say("# labelled pixels over the events: class 1 %d, class 2 %d -> the rarest class is %d" % (int(totals[1]), int(totals[2]), rare))
    for H, W in CROPS:
        modes = {"min_lit = 0": dict(min_lit=0), "min_lit = %d" % MIN_LIT: dict(min_lit=MIN_LIT),
                 "classes = {%d}, min_lit = %d" % (rare, MIN_LIT // 4): dict(min_lit=MIN_LIT // 4, classes={rare})}
        for name, kw in modes.items():
            cropper = crops.EventCropper(crop=(H, W), per_event=K, tries=8, seed=3, **kw)
            lit = rarest = accepted = 0
            for n, (im, lb) in enumerate(events):
                b = cropper(im.cuda(), lb.cuda(), number=n)
                lit += int((b.adc > 10.0).sum())
                rarest += int((b.label == rare).sum())
                accepted += int(b.table[:, 5].sum())
            crops_n = K * len(events)
            say("%-32s %d x %d  lit pixels per crop %9.1f   class-%d pixels per crop %9.1f   accepted %d of %d"
                % (name, H, W, lit / crops_n, rare, rarest / crops_n, accepted, crops_n))


def step_stagers(a, say, events):
    import torch
    from ubresnet_amd import crops, synthetic
    from ubresnet_amd.sparse import SparseEvent
    from ubresnet_amd.staging import BatchStager
    H, W = CROPS[0]
    say("# batches/s of %d x 1 x %d x %d, %d batches after 3 of warm-up, median (spread) of %d alternating repetitions; the consumer "
        "only waits for each batch" % (K, H, W, a.batches, a.reps))
    dense = [crops.LabelledEvent(im.pin_memory(), lb.pin_memory()) for im, lb in events[:4]]
    sparse = [crops.LabelledEvent(SparseEvent.from_dense(im), SparseEvent.from_dense(lb.float())) for im, lb in events[:4]]
    for ev in sparse:
        for s in (ev.image, ev.label):
            s.index, s.value = s.index.pin_memory(), s.value.pin_memory()
    loader = _cached_loader(H, W)
    kw = dict(crop=(H, W), per_event=K, min_lit=MIN_LIT, tries=8, flip_rows=True, flip_cols=True)
    stagers = {"EventCropStager, dense events": crops.EventCropStager(dense, crops.EventCropper(**kw)),
               "EventCropStager, sparse events": crops.EventCropStager(sparse, crops.EventCropper(**kw)),
               "BatchStager, pre-cropped": BatchStager(loader, K, H, W, tag="train", threads=4)}
    runs = {k: [] for k in stagers}
    try:
        for st in stagers.values():
            for _ in range(3):
                st.next()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, st in stagers.items():
                t0 = time.perf_counter()
                for _ in range(a.batches):
                    st.next()
                torch.cuda.synchronize()
                runs[k].append(a.batches / (time.perf_counter() - t0))
    finally:
        for st in stagers.values():
            st.close()
    for k, r in runs.items():
        say("%-32s %8.1f batches/s (spread %.1f)" % (k, statistics.median(r), max(r) - min(r)))
    say("# (BatchStager's loader serves crops from a cache of %d entries built before the clock starts: its producers only assemble and copy "
        "the batch; the event stagers upload a whole %.0f MB view, or its lists, per batch of %d crops)" % (NENTRIES, P * ROWS * COLS * 5e-6, K))


def _cached_loader(H, W):
    from ubresnet_amd import synthetic
    ld = synthetic.SyntheticLArCVDataset(H, W, tag="train", nentries=NENTRIES, cache=NENTRIES)
    ld.start(K)
    for i in range(NENTRIES):
        ld._entry(i)                       # fill the cache: the generator never runs inside a timed leg
    return ld


STEP_LEGS = ("resident batch", "BatchStager, pre-cropped", "EventCropStager, dense events", "EventCropStager, sparse events")


def step_train(a, say, events, only=None):
    """the bf16 guarded train step fed each way, in one run: ms per step, wall clock over --steps steps between two synchronisations,
    median (spread) over --reps alternating repetitions.  only=LEG runs that leg alone (for a kernel trace) and reports nothing else."""
    import torch
    from ubresnet_amd import crops, synthetic
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.sparse import SparseEvent
    from ubresnet_amd.staging import BatchStager
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    H, W = CROPS[0]
    torch.manual_seed(0)
    model = UResNet(num_classes=3, input_channels=1, inplanes=16).cuda()
    model.compute_dtype = torch.bfloat16
    model.train()
    crit = PixelWiseNLLLoss()
    opt = FlatAdam(model, lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)

    def step(x, lab, wgt):
        loss = crit.forward(model.forward(x), lab, wgt)
        opt.zero_grad()
        loss.backward()
        opt.step()

    kw = dict(crop=(H, W), per_event=K, min_lit=MIN_LIT, tries=8, flip_rows=True, flip_cols=True)
    dense = [crops.LabelledEvent(im.pin_memory(), lb.pin_memory()) for im, lb in events[:4]]
    sparse = [crops.LabelledEvent(SparseEvent.from_dense(im), SparseEvent.from_dense(lb.float())) for im, lb in events[:4]]
    for ev in sparse:
        for sp in (ev.image, ev.label):
            sp.index, sp.value = sp.index.pin_memory(), sp.value.pin_memory()
    resident = tuple(torch.from_numpy(t).cuda() for t in synthetic.make_batch(K, H, W, 1000))
    names = [n for n in STEP_LEGS if only is None or n == only]
    feeds = {}
    if "BatchStager, pre-cropped" in names:
        feeds["BatchStager, pre-cropped"] = BatchStager(_cached_loader(H, W), K, H, W, tag="train", threads=2)
    if "EventCropStager, dense events" in names:
        feeds["EventCropStager, dense events"] = crops.EventCropStager(dense, crops.EventCropper(**kw))
    if "EventCropStager, sparse events" in names:
        feeds["EventCropStager, sparse events"] = crops.EventCropStager(sparse, crops.EventCropper(**kw))

    def run(name, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step(*(resident if name == "resident batch" else feeds[name].next()))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    try:
        for name in names:
            run(name, 4)                   # warm-up: launch plans, pinned slots, allocator
        runs = {name: [] for name in names}
        for _ in range(a.reps):
            for name in names:             # alternating
                runs[name].append(run(name, a.steps))
        crit.flush()
    finally:
        for st in feeds.values():
            st.close()
    say("# the bf16 %d x 1 x %d x %d guarded train step (UResNet ip16, FlatAdam(max_grad_norm=1, skip_nonfinite)) fed each way in one run; ms per step, "
        "wall clock over %d steps between two synchronisations: median (spread = max - min) over %d alternating repetitions" % (K, H, W, a.steps, a.reps))
    med = {n: statistics.median(r) for n, r in runs.items()}
    spread = {n: max(r) - min(r) for n, r in runs.items()}
    for n in names:
        say("%-32s %7.2f ms (spread %.2f)   runs: %s" % (n, med[n], spread[n], " ".join("%.2f" % x for x in runs[n])))
    base = "BatchStager, pre-cropped"
    for n in names:
        if n.startswith("EventCropStager") and base in med:
            delta, allowed = med[n] - med[base], spread[n] + spread[base]
            say("%s against %s: %+.2f ms, %s the two legs' combined spread of %.2f ms" % (n, base, delta, "within" if abs(delta) <= allowed else "OUTSIDE", allowed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--only-train-leg", default=None, choices=STEP_LEGS, help="run that leg of the train step alone, for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "cropbench needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("# tools/cropbench.py --events %d --reps %d --batches %d --steps %d on %s" % (a.events, a.reps, a.batches, a.steps, torch.cuda.get_device_name(0)))
    if a.only_train_leg:
        step_train(a, say, _events(4), only=a.only_train_leg)
        return
    events = _events(max(a.events, 4))
    views = [(im.cuda(), lb.cuda()) for im, lb in events[:2]]
    step_calls(a, say, views)
    step_composite(a, say, views)
    step_sampler(a, say, events[:a.events])
    step_stagers(a, say, events)
    step_train(a, say, events)


if __name__ == "__main__":
    main()
