"""Per-image augmentation parameters of a training batch: zero-pad, flip each axis, cut a window at a random offset.

The reference's LArCV1 drivers open with ``padandcropandflip`` (training/train_ubresnet2018_wlarcv1.py:59-68): a crop is padded
by 4 pixels per side, each axis is flipped with probability 1/2 and a window of the crop's size is cut at an offset in
``[0, 8)`` per axis.  There it takes the image alone and is never called.  Here the draws are made on the host, four small
integers per image, and the transform runs on the device for image, label and weight together (``uba_augment_batch`` of
libubresnet_aug.so, through ``BatchStager(..., augment=Augment())``).

    aug = Augment(pad=4, seed=base_seed + rank)
    aug.params(seq, batchsize)          # int32 [B, 4]: (flip_rows, flip_cols, off_r, off_c) per image

``params`` is a pure function of ``(seed, seq)``, `seq` being the batch's sequence number: thread timing and a resume that
skips batches cannot change what a batch looks like.  No torch here.
"""
from __future__ import annotations

import numpy as np

__all__ = ["Augment"]


class Augment(object):
    def __init__(self, pad=4, flip_rows=True, flip_cols=True, seed=0, pad_label=0, pad_weight=0.0):
        self.pad = int(pad)
        if self.pad < 0:
            raise ValueError("Augment: pad must be >= 0")
        self.flip_rows, self.flip_cols = bool(flip_rows), bool(flip_cols)
        self.seed = int(seed)
        if not 0 <= self.seed < 2 ** 32:
            raise ValueError("Augment: seed must fit 32 bits")
        self.pad_label, self.pad_weight = int(pad_label), float(pad_weight)

    def draw(self, rs, batchsize):
        """int32 [B, 4] from the caller's numpy RandomState, per image in the reference's order: rand() > 0.5 for the rows,
        rand() > 0.5 for the columns, randint(0, 2*pad) for the rows, randint(0, 2*pad) for the columns.  A disabled flip
        draws nothing and gives 0; pad == 0 draws no offsets."""
        out = np.zeros((int(batchsize), 4), np.int32)
        for i in range(int(batchsize)):
            if self.flip_rows:
                out[i, 0] = rs.rand() > 0.5
            if self.flip_cols:
                out[i, 1] = rs.rand() > 0.5
            if self.pad > 0:
                out[i, 2] = rs.randint(0, 2 * self.pad)
                out[i, 3] = rs.randint(0, 2 * self.pad)
        return out

    def params(self, seq, batchsize):
        """the parameters of batch number `seq`: a pure function of (seed, seq)"""
        seq = int(seq)
        if not 0 <= seq < 2 ** 32:
            raise ValueError("Augment: seq must fit 32 bits")
        return self.draw(np.random.RandomState(np.array([self.seed, seq], np.uint32)), batchsize)
