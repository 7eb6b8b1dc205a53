"""PixelWiseFocalLoss: the focal loss with the forward contract of PixelWiseNLLLoss, HIP kernels (libubresnet_loss.so).

    crit = PixelWiseFocalLoss(weight=None, gamma=2.0, ignore_index=-100, normalize="pixels")
    loss = crit.forward(predict, target, pixelweights)      # or crit(...)

predict: (b,c,h,w) float32 log-softmax; target: (b,h,w) int64; pixelweights: (b,h,w) float32.
loss = sum over the contributing pixels of  -(1 - p_t)^gamma * predict[b,target,h,w] * weight[target] * pixelweights,  p_t =
exp(predict[b,target,h,w]), divided by
    "pixels":   b*h*w, ignored pixels included (the reference's mean; with gamma=0 this is PixelWiseNLLLoss),
    "valid":    the number of pixels that contributed (target not ignore_index and inside [0,c)),
    "weights":  the sum of weight[target] * pixelweights over them (what torch's nll_loss(weight=...) divides by).
The denominator stays on the device: the step has no host sync and captures into a graph.  A batch in which nothing contributed
has loss 0 and a zero gradient.  crit.read() is the one opt-in host sync.
"""
import math

import torch
import torch.nn as nn

from ubresnet_amd import _lib as L
from ubresnet_amd import _loss as K
from ubresnet_amd.training.pixelwise_nllloss import _assert_no_grad, _label_check

_workspaces = {}       # one per device, reused: its use is ordered by the stream


def _workspace(device):
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.empty(K.WORKSPACE_BYTES // 8, dtype=torch.float64, device=device)
    return ws


class _FocalBwdFn(torch.autograd.Function):
    """the backward as a Function of its own, so that differentiating it raises instead of returning a silent zero"""

    @staticmethod
    def forward(ctx, g_loss, predict, target, pixelweights, ctl, classw, ignore_index, gamma):
        g = torch.empty_like(predict)
        g_loss = g_loss.contiguous().to(torch.float32)
        N, Cn, H, W = predict.shape
        K.focal_bwd(g_loss.data_ptr(), ctl.data_ptr(), predict.data_ptr(), target.data_ptr(), pixelweights.data_ptr(), L.ptr(classw),
                    N, Cn, H, W, ignore_index, gamma, g.data_ptr(), L.stream_ptr())
        return g

    @staticmethod
    def backward(ctx, *_):
        raise RuntimeError("PixelWiseFocalLoss: double backward is not implemented")


class _PixelFocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, predict, target, pixelweights, classw, ignore_index, gamma, mode, report_now, owner):
        if predict.dtype != torch.float32 or pixelweights.dtype != torch.float32 or target.dtype != torch.int64:
            raise RuntimeError("PixelWiseFocalLoss: expected predict/pixelweights float32 and target int64, got %s/%s/%s"
                               % (predict.dtype, pixelweights.dtype, target.dtype))
        if predict.dim() != 4 or tuple(target.shape) != (predict.shape[0], predict.shape[2], predict.shape[3]) \
                or tuple(pixelweights.shape) != tuple(target.shape):
            raise RuntimeError("PixelWiseFocalLoss: shape mismatch predict %s target %s pixelweights %s"
                               % (tuple(predict.shape), tuple(target.shape), tuple(pixelweights.shape)))
        N, Cn, H, W = predict.shape
        if not 1 <= Cn <= K.MAX_CLASSES:
            raise RuntimeError("PixelWiseFocalLoss: %d classes; the kernels take 1 to %d" % (Cn, K.MAX_CLASSES))
        L.require_cuda(predict, "predict")                       # (after the checks that need no device)
        predict, target, pixelweights = predict.contiguous(), target.contiguous(), pixelweights.contiguous()
        _label_check.poll()
        ctl = torch.empty(K.CTL_WORDS, dtype=torch.float64, device=predict.device)       # per call: a saved tensor of this step
        loss = torch.empty((), dtype=torch.float32, device=predict.device)
        K.focal_fwd(predict.data_ptr(), target.data_ptr(), pixelweights.data_ptr(), L.ptr(classw), N, Cn, H, W, ignore_index, gamma, mode,
                    _workspace(predict.device).data_ptr(), ctl.data_ptr(), loss.data_ptr(), L.stream_ptr())
        _label_check.watch(ctl[K.CTL["BAD"]:K.CTL["BAD"] + 1], Cn, ignore_index)
        if report_now:
            # a loss nobody back-propagates: report now, as PixelWiseNLLLoss does
            _label_check.flush()
        owner._last = (ctl, Cn)
        ctx.save_for_backward(predict, target, pixelweights, ctl)
        ctx.classw, ctx.ignore_index, ctx.gamma = classw, ignore_index, gamma
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        predict, target, pixelweights, ctl = ctx.saved_tensors
        g = _FocalBwdFn.apply(g_loss, predict, target, pixelweights, ctl, ctx.classw, ctx.ignore_index, ctx.gamma)
        return g, None, None, None, None, None, None, None, None


class PixelWiseFocalLoss(nn.modules.loss._WeightedLoss):
    def __init__(self, weight=None, gamma=2.0, ignore_index=-100, normalize="pixels"):
        super(PixelWiseFocalLoss, self).__init__(weight, None, None, "mean")
        gamma = float(gamma)
        if not math.isfinite(gamma) or gamma < 0.0:
            raise ValueError("PixelWiseFocalLoss: gamma must be finite and >= 0, got %r" % (gamma,))
        if normalize not in K.MODES:
            raise ValueError("PixelWiseFocalLoss: normalize must be one of %s, got %r" % (sorted(K.MODES), normalize))
        self.gamma = gamma
        self.ignore_index = ignore_index
        self.normalize = normalize
        self._last = None

    @staticmethod
    def flush():
        """Out-of-range target labels are counted on the device and reported one loss call later, or immediately for a loss
        computed without gradients; this raises for the outstanding batches now (PixelWiseNLLLoss.flush: it is the same check)."""
        _label_check.flush()

    def forward(self, predict, target, pixelweights):
        """
        predict: (b,c,h,w) tensor with output from logsoftmax
        target:  (b,h,w) tensor with correct class
        pixelweights: (b,h,w) tensor with weights for each pixel
        """
        _assert_no_grad(target)
        _assert_no_grad(pixelweights)
        classw = self.weight
        if classw is not None:
            classw = classw.to(device=predict.device, dtype=torch.float32).contiguous()
            if predict.dim() == 4 and classw.numel() != predict.shape[1]:
                raise RuntimeError("PixelWiseFocalLoss: weight has %d entries for %d classes" % (classw.numel(), predict.shape[1]))
        report_now = not (torch.is_grad_enabled() and predict.requires_grad)      # (decided here: grad mode is off inside Function.forward)
        return _PixelFocalFn.apply(predict, target, pixelweights, classw, self.ignore_index, self.gamma, K.MODES[self.normalize],
                                   report_now, self)

    def read(self):
        """The by-products of the last forward, copied to the host (this waits for the device: call it when logging, not per
        step): loss, denom, valid (contributing pixels), per_class_loss (mean of the terms per class, nan where a class has no
        pixel) and per_class_pixels."""
        if self._last is None:
            raise RuntimeError("PixelWiseFocalLoss.read(): no forward yet")
        ctl, Cn = self._last
        c = K.read_ctl(ctl.cpu().numpy().tobytes())
        pix = c["class_pixels"][:Cn]
        return dict(loss=c["loss"], denom=c["denom"], valid=c["valid"],
                    per_class_loss=[s / n if n else float("nan") for s, n in zip(c["class_loss"][:Cn], pix)], per_class_pixels=pix)
