#!/usr/bin/env python
"""Augmentation fixture, made by the REFERENCE's own ``padandcropandflip`` (training/train_ubresnet2018_wlarcv1.py:59-68).

augment_padcropflip.npz: for seeds k = 0..15, ``np.random.seed(k)`` and then the reference's function on plane 0 of
``synthetic.make_batch(1, 256, 256, 1000 + k)``; the 256 x 256 outputs and the seeds.  The driver is Python 2 and can be
neither imported nor parsed whole, so the function's text is cut out of the file -- from its ``def`` line to the next line
that starts in column 0 -- and executed alone with ``np`` in scope.  Needs the reference checkout (as make_golden.py does);
nothing of its text is stored here or in the fixture.

    python tests/golden/make_golden_augment.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from ubresnet_amd import synthetic  # noqa: E402

REF = "/root/reference"
DRIVER = os.path.join(REF, "training", "train_ubresnet2018_wlarcv1.py")
NAME = "padandcropandflip"
SEEDS = list(range(16))
SIZE = 256


def reference_function():
    lines = open(DRIVER).read().split("\n")
    start = [i for i, l in enumerate(lines) if l.startswith("def %s(" % NAME)]
    assert len(start) == 1, "expected one definition of %s in %s" % (NAME, DRIVER)
    end = start[0] + 1
    while end < len(lines) and (not lines[end] or lines[end][0] in " \t"):
        end += 1
    scope = {"np": np}
    exec(compile("\n".join(lines[start[0]:end]) + "\n", DRIVER, "exec"), scope)
    return scope[NAME]


def main():
    fn = reference_function()
    outs = []
    for k in SEEDS:
        x = synthetic.make_batch(1, SIZE, SIZE, 1000 + k)[0][0, 0]
        np.random.seed(k)
        y = np.array(fn(x), np.float32)
        assert y.shape == (SIZE, SIZE)
        outs.append(y)
    path = os.path.join(HERE, "augment_padcropflip.npz")
    np.savez_compressed(path, seeds=np.array(SEEDS, np.int64), outputs=np.stack(outs))
    print("wrote %s (%d bytes), %d outputs, %.2f%% of the pixels lit" % (
        path, os.path.getsize(path), len(outs), 100.0 * float((np.stack(outs) != 0).mean())))


if __name__ == "__main__":
    main()
