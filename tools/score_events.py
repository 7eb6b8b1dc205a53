#!/usr/bin/env python3
"""Score whole-view inference on labelled events: the analysis script the reference left empty (ana/dllee_ssnet_comparison.py, the
"current standard" caller of the stub caffe/analyze_accuracy.py).

    python tools/score_events.py [--events N] [--tta cols,rows] [--ema CHECKPOINT | --checkpoint CHECKPOINT] [--rows R --cols C]

Synthetic labelled events -- every plane one synthetic.make_crop of the view's size, its label image the truth -- go through
WholeViewSegmenter(output="products", tta=...) and an EventScorer; the Score is printed after one host sync.  Without a checkpoint
the network is a seeded, untrained UResNet: the numbers then say nothing about a trained one, the table is what is shown.
--ema loads the averaged weights of a checkpoint that ParamEMA saved (deploy.load_model(..., ema=True))."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=4)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--cols", type=int, default=832)
    ap.add_argument("--planes", type=int, default=3)
    ap.add_argument("--tile", default="256x416", help="tile rows x cols, multiples of 32")
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--tta", default=None, help="comma-separated views out of rows, cols, both")
    ap.add_argument("--dtype", default="f32", choices=["f16", "f32"], help="compute type of the network (seeded untrained weights overflow in f16)")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--ema", default=None, metavar="CHECKPOINT", help="a checkpoint with averaged weights; they are the ones loaded")
    ap.add_argument("--bins", type=int, default=10)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--interface-from", type=int, default=1)
    ap.add_argument("--seed", type=int, default=9000)
    a = ap.parse_args()
    import numpy as np
    import torch
    from ubresnet_amd import deploy, scoring, synthetic
    if a.checkpoint and a.ema:
        ap.error("--checkpoint and --ema name the same thing twice")
    tta = tuple(a.tta.split(",")) if a.tta else None
    th, tw = (int(v) for v in a.tile.split("x"))
    torch.manual_seed(7)
    model = deploy.load_model(a.ema or a.checkpoint, "cuda:0", num_classes=a.classes, ema=bool(a.ema))
    seg = deploy.WholeViewSegmenter(model, rows=a.rows, cols=a.cols, planes=a.planes, tile=(th, tw), batch=a.batch, output="products",
                                    dtype=torch.float16 if a.dtype == "f16" else torch.float32,
                                    tta=tta)
    scorer = scoring.EventScorer(num_classes=a.classes, planes=a.planes, bins=a.bins, radius=a.radius,
                                 interface_from=a.interface_from, capacity=a.events)
    for n in range(a.events):
        adc = np.zeros((a.planes, 1, a.rows, a.cols), np.float32)
        truth = np.zeros((a.planes, a.rows, a.cols), np.int64)
        for p in range(a.planes):
            adc[p, 0], truth[p], _ = synthetic.make_crop(a.rows, a.cols, a.seed + n * a.planes + p)
        scorer.add(seg(torch.from_numpy(adc).cuda()), torch.from_numpy(truth).cuda())
    print("# %d synthetic events of %d x %d x %d, %s, tta %s" % (a.events, a.planes, a.rows, a.cols,
          "weights of %s%s" % (a.ema or a.checkpoint, " (averaged)" if a.ema else "") if (a.ema or a.checkpoint) else "seeded untrained weights",
          tta or "off"))
    print(scorer.read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
