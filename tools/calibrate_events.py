#!/usr/bin/env python3
"""Fit a temperature per wire plane on labelled events and show what it does to the calibration of the event products.

    python tools/calibrate_events.py [--events N] [--train-steps S] [--checkpoint CHECKPOINT] [--rows R --cols C]

Synthetic labelled events -- every plane one synthetic.make_crop of the view's size, its label image the truth -- go through
WholeViewSegmenter(output="scores") with tta, blend and temperature off and a calibration.TemperatureFit; the NLL curve and the
temperature of every plane are printed after one host sync.  Then the same events are scored by an EventScorer from
output="products" without and with the fitted temperature, and the expected calibration error (ECE) of both is printed.

Without a checkpoint the network is a UResNet that this tool trains for --train-steps steps on synthetic crops first (a seeded,
untrained network saturates every probability and has nothing to calibrate).  That shows the mechanism; it says nothing about a
real trained network."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def brief_training(model, classes, steps, log):
    import torch
    from ubresnet_amd import synthetic
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
    crit = PixelWiseNLLLoss()
    for step in range(steps):
        x, lab, wgt = synthetic.make_batch(4, 128, 128, 100 + step)
        out = model(torch.from_numpy(x).cuda())
        loss = crit(out, torch.from_numpy(lab).cuda(), torch.from_numpy(wgt).cuda())
        opt.zero_grad()
        loss.backward()
        opt.step()
        if step % 20 == 0 or step == steps - 1:
            log("# training step %3d  loss %.4f" % (step, float(loss)))
    model.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=4)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--cols", type=int, default=832)
    ap.add_argument("--planes", type=int, default=3)
    ap.add_argument("--tile", default="256x416", help="tile rows x cols, multiples of 32")
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--train-steps", type=int, default=60)
    ap.add_argument("--bins", type=int, default=10)
    ap.add_argument("--seed", type=int, default=9000)
    a = ap.parse_args()
    import numpy as np
    import torch
    from ubresnet_amd import calibration, deploy, scoring, synthetic
    th, tw = (int(v) for v in a.tile.split("x"))
    torch.manual_seed(7)
    model = deploy.load_model(a.checkpoint, "cuda:0", num_classes=a.classes)
    if not a.checkpoint:
        brief_training(model, a.classes, a.train_steps, print)
    kw = dict(rows=a.rows, cols=a.cols, planes=a.planes, tile=(th, tw), batch=a.batch, dtype=torch.float32)
    events = []
    for n in range(a.events):
        adc = np.zeros((a.planes, 1, a.rows, a.cols), np.float32)
        truth = np.zeros((a.planes, a.rows, a.cols), np.int64)
        for p in range(a.planes):
            adc[p, 0], truth[p], _ = synthetic.make_crop(a.rows, a.cols, a.seed + n * a.planes + p)
        events.append((torch.from_numpy(adc).cuda(), torch.from_numpy(truth).cuda()))
    seg = deploy.WholeViewSegmenter(model, output="scores", **kw)           # the single-view network: tta, blend, temperature off
    fit = calibration.TemperatureFit(a.classes, groups=a.planes)
    for view, truth in events:
        fit.add(seg(view), truth, lit=view)
    cal = fit.read()
    print("# %d synthetic events of %d x %d x %d, %s" % (a.events, a.planes, a.rows, a.cols, "weights of %s" % a.checkpoint if a.checkpoint
          else "a UResNet trained here for %d steps on synthetic crops: the mechanism, not a real network" % a.train_steps))
    print("%8s " % "T" + " ".join("%12s" % ("NLL[plane %d]" % g) for g in range(a.planes)))
    for k, t in enumerate(cal.temps):
        print("%8.4f " % t + " ".join("%12.6f" % cal.nll(g)[k] for g in range(a.planes)))
    print(cal)
    for name, temperature in (("before", None), ("after", cal)):
        prod = deploy.WholeViewSegmenter(model, output="products", temperature=temperature, **kw)
        scorer = scoring.EventScorer(num_classes=a.classes, planes=a.planes, bins=a.bins, capacity=a.events)
        for view, truth in events:
            scorer.add(prod(view), truth)
        score = scorer.read()
        check = calibration.TemperatureFit(a.classes, groups=a.planes, temps=[1.0])
        tempered = deploy.WholeViewSegmenter(model, output="scores", temperature=temperature, **kw)
        for view, truth in events:
            check.add(tempered(view), truth, lit=view)
        c = check.read()
        print("%-6s ECE %.4f  (per plane %s)   NLL per lit pixel %s" % (name, score.ece(), " ".join("%.4f" % score.ece(plane=p) for p in range(a.planes)),
                                                                       " ".join("%.5f" % c.nll(g)[0] for g in range(a.planes))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
