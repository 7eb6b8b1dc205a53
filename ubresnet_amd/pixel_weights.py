"""Pixel weights for ``PixelWiseNLLLoss`` made on the device from the label images alone.

The reference trains on a stored weight product (``ts_keyspweight``) that "helps balance out the number of classes per image"
and up-weights "points of interest"; where the wire carries none, ``prep_data`` falls back to all ones
(training/train_ubresnet2018_wlarcv2.py:602-605), which on crops that are 97-99 % background trains a background detector.
``PixelWeights`` makes such an image per batch with ``ubw_pixel_weights`` (libubresnet_weight.so, include/ubresnet_weight.h):

* per image, class ``c`` with ``n_c`` valid pixels out of ``V`` in ``K`` present classes weighs
  ``min(V / (K * n_c), max_weight)`` -- with no cap the weights of an image's valid pixels have mean 1, so the loss keeps
  the scale it has with all-ones weights; an invalid label (anything outside ``[0, num_classes)``) weighs 0;
* a pixel of a class ``>= interface_from`` with a different class ``>= interface_from`` inside the ``(2 radius + 1)^2`` window
  around it (clipped at the image edges) is multiplied by ``gain``: ``interface_from=1`` marks track/shower contacts,
  ``interface_from=0`` every edge against background; ``radius=0`` turns the gain off.

    pw = PixelWeights(num_classes=3, radius=1, gain=2.0)
    weight = pw(label)                          # label: int64 CUDA [B,H,W]; runs on the current stream
    pw.counts                                   # [B,16] int64 on the device: n_c of the last call, for logging

``BatchStager(..., weights=pw)`` launches it on the copy stream behind the batch preparation; ``when`` says for which
batches: ``"missing"`` only where the wire has no ``weight_<tag>`` entry (the batches that get ones today), ``"always"`` for
every batch, replacing wire weights.  Every output is reproducible bit for bit (integer counts, one fp64 divide, one
conversion, one fp32 multiply); tests/weights_ref.py is the numpy statement of the rule.  There is no fallback: a missing
library is a RuntimeError.
"""
from __future__ import annotations

import math

from . import _weight

__all__ = ["PixelWeights"]


class PixelWeights(object):
    def __init__(self, num_classes=3, max_weight=float("inf"), radius=0, gain=1.0, interface_from=1, when="missing"):
        for name, v in (("num_classes", num_classes), ("radius", radius), ("interface_from", interface_from)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError("PixelWeights: %s must be an int (got %r)" % (name, v))
        if not 1 <= num_classes <= _weight.MAX_CLASSES:
            raise ValueError("PixelWeights: num_classes must be 1..%d (got %d)" % (_weight.MAX_CLASSES, num_classes))
        if not 0 <= radius <= _weight.MAX_RADIUS:
            raise ValueError("PixelWeights: radius must be 0..%d (got %d)" % (_weight.MAX_RADIUS, radius))
        if not 0 <= interface_from <= num_classes:
            raise ValueError("PixelWeights: interface_from must be 0..num_classes (got %d)" % interface_from)
        max_weight, gain = float(max_weight), float(gain)
        if math.isnan(max_weight) or max_weight <= 0.0:
            raise ValueError("PixelWeights: max_weight must be > 0, inf for no cap (got %r)" % max_weight)
        if math.isnan(gain) or math.isinf(gain) or gain < 0.0:
            raise ValueError("PixelWeights: gain must be finite and >= 0 (got %r)" % gain)
        if when not in ("missing", "always"):
            raise ValueError("PixelWeights: when must be 'missing' or 'always' (got %r)" % (when,))
        self.num_classes, self.max_weight, self.radius, self.gain = num_classes, max_weight, radius, gain
        self.interface_from, self.when = interface_from, when
        self.counts = None

    def launch(self, label_ptr, weight_ptr, counts_ptr, shape, stream=None):
        """ubw_pixel_weights on raw device addresses: `shape` is (B, H, W), `counts_ptr` a [B,16] int64 workspace"""
        _weight.pixel_weights(label_ptr, weight_ptr, counts_ptr, shape, self.num_classes, self.max_weight, self.radius, self.gain,
                              self.interface_from, stream=stream)

    def __call__(self, label, out=None):
        import torch
        if not (label.is_cuda and label.dtype == torch.int64 and label.dim() == 3 and label.is_contiguous()):
            raise ValueError("PixelWeights: label must be a contiguous int64 CUDA tensor [B,H,W]")
        if out is None:
            out = torch.empty(label.shape, dtype=torch.float32, device=label.device)
        elif not (out.is_cuda and out.device == label.device and out.dtype == torch.float32 and out.shape == label.shape
                  and out.is_contiguous()):
            raise ValueError("PixelWeights: out must be a contiguous float32 tensor of label's shape on label's device")
        counts = torch.empty((label.shape[0], _weight.MAX_CLASSES), dtype=torch.int64, device=label.device)
        with torch.cuda.device(label.device):
            self.launch(label.data_ptr(), out.data_ptr(), counts.data_ptr(), tuple(label.shape),
                        torch.cuda.current_stream(label.device).cuda_stream)
        self.counts = counts
        return out
