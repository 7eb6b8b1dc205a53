"""Gradient accumulation at replay speed: several micro-batches per optimizer step, summed on the device in one flat buffer.

    acc = GradAccumulator(model, every=4, average=True)       # after model.to(device)
    for micro in range(...):
        loss = criterion(model(x), y, w)
        loss.backward()
        if reducer is not None: reducer.finish()
        if acc.add():             # True on every `every`-th call: the flat gradient now holds the mean (average=False: the sum)
            opt.step(); ema.update()
        opt.zero_grad()           # set_to_none=True, the default: the next pass is a plain, replayed one

Every backward of this package leaves the gradients as views of ONE flat fp32 buffer (``model._ubr_flat_grad``), which a replayed
launch plan writes at the same address pass after pass.  ``zero_grad()`` between the micro-batches sets every ``.grad`` to ``None``,
so each micro-batch is a plain pass: the launch tape, the flat buffer and, under data parallelism, the bucketed exchange are all
kept.  (A backward onto existing ``.grad`` tensors still works, but it is scheduled from Python into a fresh buffer and added with
one launch per parameter, and under data parallelism it is exchanged in one blocking all-reduce.)  ``add()`` is one launch of
libubresnet_accum.so on the current stream over the whole flat buffer, padding included:

  * call 1 of a cycle            ``ubc_set``     accumulator = gradient, bit for bit
  * calls 2 .. every - 1         ``ubc_add``     accumulator += gradient
  * call `every`                 ``ubc_finish``  gradient = (accumulator + gradient) * scale, IN PLACE in the flat gradient buffer

with ``scale = float32(1 / every)`` (``average=False``: 1.0).  After the last call the ``.grad`` tensors are still the views of the
flat buffer and hold the mean, so ``FlatAdam`` / ``FlatSGD`` (plain, guarded, grouped), ``optim.grad_norm``, ``GradAllReducer`` and
``ParamEMA`` work unchanged.  Which call a micro-batch gets is the host's count: nothing is read back, nothing is allocated after
construction, and a cycle captures into a graph.  With ``every=1`` nothing is launched.

The sum is a plain left-to-right fp32 sum, each addition rounded once.  A non-finite micro-batch makes the mean non-finite; a
guarded optimizer then skips the whole step.  A parameter without a gradient (frozen, or left out of a grouped step) is allowed:
its stale bytes in the flat buffer are summed like any others and stay ignored by the grouped optimizer.

Data parallel.  Every micro-batch is exchanged bucket by bucket under its backward exactly as a plain step is; call
``reducer.finish()`` before ``add()``.  The average over ranks commutes with the sum over micro-batches up to rounding.

There is no ``state_dict``: an open cycle holds gradients of parameters that a checkpoint does not describe.  Checkpoint at cycle
boundaries (``pending == 0``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _accum as A
from . import _lib as L

__all__ = ["GradAccumulator"]


def _kind_of(model) -> str:
    return "aspp" if hasattr(model, "ASPP_layer_enc3") else "uresnet"


class GradAccumulator(object):
    """sums `every` micro-batch gradients in a flat device buffer and leaves their mean (``average=False``: their sum) in the flat
    gradient buffer of the last one; see the module docstring"""

    def __init__(self, model, every, average=True):
        if int(every) != every or int(every) < 1:
            raise ValueError("every must be an integer >= 1, got %r" % (every,))
        self._every, self._average = int(every), bool(average)
        self.model = model
        self._scale = float(np.float32(1.0 / self._every)) if self._average else 1.0
        self._pending = 0
        self._layout = self.buffer = None
        if self._every > 1:
            from .autograd_fn import _engine
            params = list(model.parameters())
            if not params or not all(p.is_cuda and p.device == params[0].device for p in params):
                raise RuntimeError("ubresnet_amd.accum: the model's parameters must be on one ROCm device (move the model first)")
            eng = _engine(model, _kind_of(model))
            self._layout = [(name, p, eng.grad_offsets[name]) for name, p in eng.grad_order]
            self.buffer = torch.zeros(eng.grad_numel, dtype=torch.float32, device=params[0].device)

    every = property(lambda self: self._every)
    average = property(lambda self: self._average)
    pending = property(lambda self: self._pending, doc="micro-batches of the open cycle (0: none is open)")

    def reset(self):
        """drop an open cycle: the next add() starts one"""
        self._pending = 0

    def _flat_grad(self):
        g = self.model.__dict__.get("_ubr_flat_grad")
        if g is None:
            raise RuntimeError("GradAccumulator.add(): no backward has run (the model has no flat gradient buffer)")
        if g.numel() != self.buffer.numel() or g.device != self.buffer.device or g.dtype != torch.float32:
            raise RuntimeError("GradAccumulator.add(): the flat gradient buffer is %d %s values on %s, the accumulator %d float32 on %s"
                               % (g.numel(), str(g.dtype).replace("torch.", ""), g.device, self.buffer.numel(), self.buffer.device))
        cure = ("a backward onto existing .grad tensors takes the legacy accumulating path (scheduled from Python, one add per "
                "parameter), and what the flat gradient buffer then holds is not one micro-batch.  Call optimizer.zero_grad() "
                "(set_to_none=True) after every add(), then reset()")
        if self.model.__dict__.get("_ubr_grad_accumulated"):
            raise RuntimeError("GradAccumulator.add(): the last backward added into existing .grad tensors -- a missing zero_grad(): " + cure)
        base = g.data_ptr()
        for name, p, o in self._layout:
            if p.grad is not None and p.grad.data_ptr() != base + 4 * o:
                raise RuntimeError("GradAccumulator.add(): the gradient of %s is not the view of the flat gradient buffer at its offset.  "
                                   "The usual cause is a missing zero_grad(): %s" % (name, cure))
        return g

    @torch.no_grad()
    def add(self) -> bool:
        """take in the gradient of the backward that just ran: one launch on the current stream.  -> True when this was the last
        micro-batch of a cycle: the flat gradient buffer (every ``.grad``) now holds the mean or the sum, step the optimizer"""
        if self._every == 1:
            return True
        g = self._flat_grad()
        n, stream = g.numel(), L.stream_ptr()
        k = self._pending + 1
        if k == self._every:
            A.finish(g.data_ptr(), self.buffer.data_ptr(), n, self._scale, stream)
            self._pending = 0
            return True
        if k == 1:
            A.set_(self.buffer.data_ptr(), g.data_ptr(), n, stream)
        else:
            A.add(self.buffer.data_ptr(), g.data_ptr(), n, stream)
        self._pending = k
        return False
