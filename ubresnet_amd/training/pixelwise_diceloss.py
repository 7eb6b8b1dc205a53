"""PixelWiseDiceLoss: the soft Dice / Tversky region loss with the forward contract of PixelWiseNLLLoss, HIP kernels
(libubresnet_dice.so), and WeightedSumLoss, which adds criteria of that contract.

    dice = PixelWiseDiceLoss(weight=None, alpha=0.5, beta=0.5, eps=1.0, ignore_index=-100, present_only=True)
    crit = WeightedSumLoss([(1.0, PixelWiseNLLLoss()), (0.5, dice)])
    loss = crit.forward(predict, target, pixelweights)      # or crit(...)

predict: (b,c,h,w) float32 log-softmax; target: (b,h,w) int64; pixelweights: (b,h,w) float32, not negative.
Over the pixels that contribute (target not ignore_index and inside [0,c)), batch-wide and per class, with p = exp(predict):
    TP_c = sum pixelweights * p_c  over the pixels of class c,   FN_c = sum pixelweights * (1 - p_c)  over the same pixels,
    FP_c = sum pixelweights * p_c  over the pixels of the other classes,
    T_c = (TP_c + eps) / (TP_c + alpha FP_c + beta FN_c + eps),   loss = sum_c a_c (1 - T_c),   a_c = weight[c] present_c / sum of those.
alpha = beta = 0.5 is soft Dice; beta > alpha (Tversky) prices a missed pixel above a false alarm.  present_only=True leaves a
class without a pixel in the batch out of the mean (decided on the device from the integer count: no host sync); with
present_only=False such a class pulls its false positives down through T_c = eps / (alpha FP_c + eps).  A batch in which nothing
contributed has loss 0 and a zero gradient.  The step has no host sync and captures into a graph; read() is the one opt-in sync.
"""
import math

import torch
import torch.nn as nn

from ubresnet_amd import _dice as K
from ubresnet_amd import _lib as L
from ubresnet_amd.training.pixelwise_nllloss import _assert_no_grad, _label_check

_workspaces = {}       # one per device, reused: its use is ordered by the stream


def _workspace(device):
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.empty(K.WORKSPACE_BYTES // 8, dtype=torch.float64, device=device)
    return ws


class _DiceBwdFn(torch.autograd.Function):
    """the backward as a Function of its own, so that differentiating it raises instead of returning a silent zero"""

    @staticmethod
    def forward(ctx, g_loss, predict, target, pixelweights, ctl, ignore_index):
        g = torch.empty_like(predict)
        g_loss = g_loss.contiguous().to(torch.float32)
        N, Cn, H, W = predict.shape
        K.dice_bwd(g_loss.data_ptr(), ctl.data_ptr(), predict.data_ptr(), target.data_ptr(), pixelweights.data_ptr(), N, Cn, H, W,
                   ignore_index, g.data_ptr(), L.stream_ptr())
        return g

    @staticmethod
    def backward(ctx, *_):
        raise RuntimeError("PixelWiseDiceLoss: double backward is not implemented")


class _PixelDiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, predict, target, pixelweights, classw, ignore_index, alpha, beta, eps, present_only, report_now, owner):
        if predict.dtype != torch.float32 or pixelweights.dtype != torch.float32 or target.dtype != torch.int64:
            raise RuntimeError("PixelWiseDiceLoss: expected predict/pixelweights float32 and target int64, got %s/%s/%s"
                               % (predict.dtype, pixelweights.dtype, target.dtype))
        if predict.dim() != 4 or tuple(target.shape) != (predict.shape[0], predict.shape[2], predict.shape[3]) \
                or tuple(pixelweights.shape) != tuple(target.shape):
            raise RuntimeError("PixelWiseDiceLoss: shape mismatch predict %s target %s pixelweights %s"
                               % (tuple(predict.shape), tuple(target.shape), tuple(pixelweights.shape)))
        N, Cn, H, W = predict.shape
        if not 1 <= Cn <= K.MAX_CLASSES:
            raise RuntimeError("PixelWiseDiceLoss: %d classes; the kernels take 1 to %d" % (Cn, K.MAX_CLASSES))
        L.require_cuda(predict, "predict")                       # (after the checks that need no device)
        predict, target, pixelweights = predict.contiguous(), target.contiguous(), pixelweights.contiguous()
        _label_check.poll()
        ctl = torch.empty(K.CTL_WORDS, dtype=torch.float64, device=predict.device)       # per call: a saved tensor of this step
        loss = torch.empty((), dtype=torch.float32, device=predict.device)
        K.dice_fwd(predict.data_ptr(), target.data_ptr(), pixelweights.data_ptr(), L.ptr(classw), N, Cn, H, W, ignore_index, alpha, beta, eps,
                   present_only, _workspace(predict.device).data_ptr(), ctl.data_ptr(), loss.data_ptr(), L.stream_ptr())
        _label_check.watch(ctl[K.CTL["BAD"]:K.CTL["BAD"] + 1], Cn, ignore_index)
        if report_now:
            # a loss nobody back-propagates: report now, as PixelWiseNLLLoss does
            _label_check.flush()
        owner._last = (ctl, Cn)
        ctx.save_for_backward(predict, target, pixelweights, ctl)
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        predict, target, pixelweights, ctl = ctx.saved_tensors
        g = _DiceBwdFn.apply(g_loss, predict, target, pixelweights, ctl, ctx.ignore_index)
        return g, None, None, None, None, None, None, None, None, None, None


class PixelWiseDiceLoss(nn.modules.loss._WeightedLoss):
    def __init__(self, weight=None, alpha=0.5, beta=0.5, eps=1.0, ignore_index=-100, present_only=True):
        super(PixelWiseDiceLoss, self).__init__(weight, None, None, "mean")
        for name, v in (("alpha", alpha), ("beta", beta), ("eps", eps)):
            if not math.isfinite(float(v)) or float(v) < 0.0:
                raise ValueError("PixelWiseDiceLoss: %s must be finite and >= 0, got %r" % (name, v))
        self.alpha, self.beta, self.eps = float(alpha), float(beta), float(eps)
        self.ignore_index = ignore_index
        self.present_only = bool(present_only)
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
                raise RuntimeError("PixelWiseDiceLoss: weight has %d entries for %d classes" % (classw.numel(), predict.shape[1]))
        report_now = not (torch.is_grad_enabled() and predict.requires_grad)      # (decided here: grad mode is off inside Function.forward)
        return _PixelDiceFn.apply(predict, target, pixelweights, classw, self.ignore_index, self.alpha, self.beta, self.eps,
                                  self.present_only, report_now, self)

    def read(self):
        """The by-products of the last forward, copied to the host (this waits for the device: call it when logging, not per
        step): loss, valid (contributing pixels) and, per class, tp, fp, fn (the weighted soft counts), pixels, index (the
        Tversky index T_c) and soft_iou = tp / (tp + fp + fn) (nan where all three are 0)."""
        if self._last is None:
            raise RuntimeError("PixelWiseDiceLoss.read(): no forward yet")
        ctl, Cn = self._last
        c = K.read_ctl(ctl.cpu().numpy().tobytes())
        tp, fp, fn = c["tp"][:Cn], c["fp"][:Cn], c["fn"][:Cn]
        return dict(loss=c["loss"], valid=c["valid"], tp=tp, fp=fp, fn=fn, pixels=c["pixels"][:Cn], index=c["T"][:Cn],
                    soft_iou=[a / (a + b + d) if a + b + d != 0 else float("nan") for a, b, d in zip(tp, fp, fn)])


class WeightedSumLoss(nn.Module):
    """sum_i w_i * crit_i(predict, target, pixelweights) over criteria with PixelWiseNLLLoss's forward contract, for epoch.train.
    Host-only: every part runs its own kernels and autograd adds the gradient images.  flush() and read() fan out to the parts."""

    def __init__(self, parts):
        super(WeightedSumLoss, self).__init__()
        parts = list(parts)
        if not parts:
            raise ValueError("WeightedSumLoss: no parts")
        for w, crit in parts:
            if not math.isfinite(float(w)):
                raise ValueError("WeightedSumLoss: weight %r is not finite" % (w,))
            if not callable(getattr(crit, "forward", None)):
                raise ValueError("WeightedSumLoss: %r has no forward" % (crit,))
        self.weights = [float(w) for w, _ in parts]
        self.parts = nn.ModuleList([crit for _, crit in parts])

    def forward(self, predict, target, pixelweights):
        total = None
        for w, crit in zip(self.weights, self.parts):
            term = crit.forward(predict, target, pixelweights)
            term = term if w == 1.0 else w * term
            total = term if total is None else total + term
        return total

    def flush(self):
        for crit in self.parts:
            flush = getattr(crit, "flush", None)
            if flush is not None:
                flush()

    def read(self):
        """[(weight, part's read() or None for a part without one)] in the order of the parts (each read() is a host sync)"""
        return [(w, crit.read() if hasattr(crit, "read") else None) for w, crit in zip(self.weights, self.parts)]
