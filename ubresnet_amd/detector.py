"""Detector effects of a training batch: dead wires, a gain per plane, electronics noise.

``Augment`` (ubresnet_amd/augment.py) moves pixels; nothing in the loader path touched their values.  Real wire-plane images
differ from training crops where geometry cannot reach: runs of dead wires zero whole columns of a view, the gain differs from
plane to plane and from run to run, and lit pixels carry noise.  ``DetectorEffects`` draws, per image and plane, a few runs of
dead columns and one gain on the host -- a table of ``1 + ceil(W/32)`` words per plane -- and ``ubx_apply`` of
libubresnet_det.so (include/ubresnet_det.h) applies the table and adds the noise on the device, in place, through
``BatchStager(..., detector=DetectorEffects(...))``.

    det = DetectorEffects(dead_runs=(0, 3), run_len=(1, 32), gain=(0.9, 1.1), noise_sigma=1.5, seed=base_seed + rank)
    det.table(seq, batchsize, planes, width)    # uint32 [B, P, 1 + ceil(W/32)]

Row ``(b, p)`` of the table: word 0 holds the bits of the float32 gain; bit ``c & 31`` of word ``1 + (c >> 5)`` set means column
``c`` of that plane is dead; bits at or beyond ``W`` are zero.  A pixel whose column is dead in EVERY plane of its image gets
``dead_label`` and ``dead_weight`` (None: keep what is there).  ``noise_on="lit"`` adds noise to nonzero pixels only, which keeps
the zeros of thresholded crops zero; ``"all"`` adds it to every live pixel.

``table`` is a pure function of ``(seed, seq)``, `seq` being the batch's sequence number, and the noise of a pixel a pure function
of ``(seed, seq)`` and its place in the batch: thread timing and a resume that skips batches cannot change what a batch looks
like.  No torch here.
"""
from __future__ import annotations

import math

import numpy as np

__all__ = ["DetectorEffects"]

STREAM_TAG = 0x55425844      # third word of the seed array ("UBXD"): keeps these draws apart from Augment's under the same seed


def _int_range(name, v, least):
    try:
        lo, hi = v
    except (TypeError, ValueError):
        raise ValueError("DetectorEffects: %s must be a (lo, hi) pair (got %r)" % (name, v))
    for x in (lo, hi):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise ValueError("DetectorEffects: %s must hold ints (got %r)" % (name, v))
    if not least <= lo <= hi:
        raise ValueError("DetectorEffects: %s must satisfy %d <= lo <= hi (got %r)" % (name, least, v))
    return int(lo), int(hi)


class DetectorEffects(object):
    def __init__(self, dead_runs=(0, 0), run_len=(1, 32), gain=(1.0, 1.0), noise_sigma=0.0, noise_on="lit", dead_label=0,
                 dead_weight=None, seed=0):
        self.dead_runs = _int_range("dead_runs", dead_runs, 0)
        self.run_len = _int_range("run_len", run_len, 1)
        try:
            glo, ghi = (float(g) for g in gain)
        except (TypeError, ValueError):
            raise ValueError("DetectorEffects: gain must be a (lo, hi) pair of numbers (got %r)" % (gain,))
        if not (math.isfinite(glo) and math.isfinite(ghi) and glo <= ghi):
            raise ValueError("DetectorEffects: gain must be finite with lo <= hi (got %r)" % (gain,))
        self.gain = (glo, ghi)
        self.noise_sigma = float(noise_sigma)
        if not (math.isfinite(self.noise_sigma) and self.noise_sigma >= 0.0):
            raise ValueError("DetectorEffects: noise_sigma must be finite and >= 0 (got %r)" % (noise_sigma,))
        if noise_on not in ("lit", "all"):
            raise ValueError("DetectorEffects: noise_on must be 'lit' or 'all' (got %r)" % (noise_on,))
        self.noise_on = noise_on
        self.dead_label = None if dead_label is None else int(dead_label)
        if self.dead_label is not None and not -2 ** 63 <= self.dead_label < 2 ** 63:
            raise ValueError("DetectorEffects: dead_label must fit 64 bits")
        self.dead_weight = None if dead_weight is None else float(dead_weight)
        if self.dead_weight is not None and not math.isfinite(self.dead_weight):
            raise ValueError("DetectorEffects: dead_weight must be finite (got %r)" % (dead_weight,))
        self.seed = int(seed)
        if not 0 <= self.seed < 2 ** 32:
            raise ValueError("DetectorEffects: seed must fit 32 bits")

    @staticmethod
    def row_words(width):
        return 1 + (int(width) + 31) // 32

    def runs(self, rs, width):
        """the dead runs of one plane from the caller's RandomState, as [(start, length)] before clipping: randint(lo, hi + 1)
        runs; per run randint(lo, hi + 1) for its length, then randint(0, W) for its start.  dead_runs == (0, 0) draws nothing."""
        if self.dead_runs == (0, 0):
            return []
        out = []
        for _ in range(int(rs.randint(self.dead_runs[0], self.dead_runs[1] + 1))):
            length = int(rs.randint(self.run_len[0], self.run_len[1] + 1))
            out.append((int(rs.randint(0, int(width))), length))
        return out

    def draw(self, rs, batchsize, planes, width):
        """uint32 [B, P, 1 + ceil(W/32)] from the caller's numpy RandomState.  Per image, then per plane, in this order: the runs
        (see runs(); a run is clipped at W), then the gain, np.float32(rs.uniform(lo, hi)).  gain == (1.0, 1.0) draws nothing and
        gives the bits of 1.0f."""
        b, p, w = int(batchsize), int(planes), int(width)
        if b < 1 or p < 1 or w < 1:
            raise ValueError("DetectorEffects: batchsize, planes and width must be >= 1")
        nw = (w + 31) // 32
        out = np.zeros((b, p, 1 + nw), np.uint32)
        dead = np.zeros(32 * nw, np.uint8)
        for i in range(b):
            for j in range(p):
                runs = self.runs(rs, w)
                if runs:
                    dead[:] = 0
                    for start, length in runs:
                        dead[start:min(start + length, w)] = 1
                    out[i, j, 1:] = np.packbits(dead, bitorder="little").view("<u4")
                g = np.float32(1.0) if self.gain == (1.0, 1.0) else np.float32(rs.uniform(self.gain[0], self.gain[1]))
                out[i, j, 0] = g.view(np.uint32)
        return out

    def table(self, seq, batchsize, planes, width):
        """the table of batch number `seq`: a pure function of (seed, seq)"""
        seq = int(seq)
        if not 0 <= seq < 2 ** 32:
            raise ValueError("DetectorEffects: seq must fit 32 bits")
        return self.draw(np.random.RandomState(np.array([self.seed, seq, STREAM_TAG], np.uint32)), batchsize, planes, width)

    def launch(self, image_ptr, label_ptr, weight_ptr, shape, table_ptr, seq, stream=None):
        """ubx_apply on raw device addresses: `shape` is (B, P, H, W), `table_ptr` the device copy of table(seq, B, P, W)"""
        from . import _det
        _det.apply(image_ptr, label_ptr, weight_ptr, shape, table_ptr, sigma=self.noise_sigma, noise_all=self.noise_on == "all",
                   seed=self.seed, seq=seq, dead_label=self.dead_label, dead_weight=self.dead_weight, stream=stream)
