"""Weight averaging: an exponential moving average (EMA) of the parameters kept on the device, for validation and deployment.

    opt = FlatAdam(model, lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    ema = ParamEMA(opt, decay=0.999, warmup=10, buffers="average")   # or buffers="share"
    loss.backward(); reducer.finish(); opt.step(); ema.update()
    with ema.applied():            # the model computes with the averaged weights; swapped back on exit, on exceptions too
        validate(...)

The average lives in a SHADOW of the flat parameter buffer of a ``FlatAdam`` / ``FlatSGD`` (plain, guarded or grouped), so an
update is three launches of libubresnet_ema.so on the current stream, whatever the number of tensors: ``ube_advance`` decides on
the device whether this update is applied and with which weight, ``ube_update`` streams ``shadow += w * (param - shadow)`` over
the flat buffers, and with ``buffers="average"`` ``ube_update_segs`` does the same for the BatchNorm running statistics, which are
in no flat buffer, through a table of addresses built once.  ``update()`` allocates nothing and reads nothing back, and no launch
argument depends on the count of updates, so ``opt.step(); ema.update()`` can be captured in a graph.

The weight.  After ``u`` applied updates the next one uses ``d = min(decay, (1 + u) / (warmup + u))`` (``warmup >= 2``; else
``d = decay``) and ``w = 1 - d``: early in training the average follows the weights closely and settles at ``decay``.

A guarded optimizer (``opt.guard`` is set) decides on the device whether its step is applied; the update reads that decision
there and a skipped step does not move the average (``held`` counts these).  Without a guard every update is applied: an
unguarded optimizer that writes NaN into the parameters poisons the average as it poisons the model.

A parameter that is frozen, or inactive in a grouped optimizer, is averaged like any other: the average of a constant is that
constant.

Evaluating.  ``applied()`` / ``swap()`` exchange the bytes of the flat parameter buffer and the shadow IN PLACE
(``buffers="average"``: the running statistics and their shadows too; ``"share"``: the statistics are left alone and the averaged
weights run on the live statistics).  No ``parameter.data`` is re-pointed: the optimizer's views, the addresses in launch plans
and in captured inference graphs all stay valid, and since no pass caches anything derived from the weights the next forward
simply computes with what is there.  While swapped, ``update()`` raises.

Data parallel.  Every rank holds identical parameters and takes the same decisions, hence identical shadows; no collective is
needed.  Statistics shadows are per rank, exactly like the running statistics themselves: ``reducer.average_bn_stats()`` applies
as before (call it before a checkpoint; it averages the live statistics, the shadows follow over the next updates).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import _ema as E
from . import _lib as L
from .optim import FlatAdam, FlatSGD

__all__ = ["ParamEMA"]


class ParamEMA(object):
    """the exponential moving average of the parameters of a FlatAdam / FlatSGD (and, with ``buffers="average"``, of the model's
    floating-point buffers); see the module docstring"""

    def __init__(self, optimizer, decay=0.999, warmup=0, buffers="average"):
        if not isinstance(optimizer, (FlatAdam, FlatSGD)):
            raise TypeError("ParamEMA needs a ubresnet_amd.optim.FlatAdam or FlatSGD (the average is kept over their flat parameter "
                            "buffer), got %s" % type(optimizer).__name__)
        self._set_schedule(decay, warmup)
        if buffers not in ("average", "share"):
            raise ValueError("buffers must be \"average\" or \"share\", got %r" % (buffers,))
        self.buffers = buffers
        self.opt = optimizer
        self.model = optimizer.model
        optimizer._check_views()
        dev = optimizer.flat.device
        self.shadow = optimizer.flat.clone()
        names = {id(p): n for n, p in self.model.named_parameters()}             # the model's state_dict names
        self._params = [(names[id(p)], p, o) for _, p, o in optimizer._layout]
        self._swapped = False
        self.ctl = torch.zeros(E.CTL_BYTES, dtype=torch.uint8, device=dev)
        E.ctl_init(self.ctl.data_ptr(), 0, L.stream_ptr())
        # the floating-point buffers (BatchNorm running_mean / running_var), one run each in a small flat shadow of their own
        self._stats = []                           # (state_dict name, live tensor, offset in self.stats)
        self.stats = self._table = self._table_of = None
        if buffers == "average":
            off = 0
            for name, b in self.model.named_buffers():
                if b.is_floating_point():
                    if b.dtype != torch.float32 or b.device != dev or not b.is_contiguous():
                        raise RuntimeError("ubresnet_amd.ema: buffer %s must be contiguous float32 on %s" % (name, dev))
                    self._stats.append((name, b, off))
                    off += b.numel()
            if self._stats:
                self.stats = torch.empty(off, dtype=torch.float32, device=dev)
                self._copy_stats_in()
                self._upload_table()

    # ---- helpers ----
    def _set_schedule(self, decay, warmup):
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError("decay must lie in [0, 1), got %r" % (decay,))
        if int(warmup) != warmup or int(warmup) < 0:
            raise ValueError("warmup must be an integer >= 0, got %r" % (warmup,))
        self.decay, self.warmup = decay, int(warmup)

    def _stat_view(self, b, off):
        return self.stats[off:off + b.numel()].view(b.shape)

    @torch.no_grad()
    def _copy_stats_in(self):
        for _, b, off in self._stats:
            self._stat_view(b, off).copy_(b)

    def _upload_table(self):
        base = self.stats.data_ptr()
        ptrs = [b.data_ptr() for _, b, _ in self._stats]
        t = E.seg_table([base + 4 * off for _, _, off in self._stats], ptrs, [b.numel() for _, b, _ in self._stats])
        self._table = torch.from_numpy(t.view(np.int64).reshape(-1, 4).copy()).to(self.stats.device)
        self._table_of = ptrs

    def _check_table(self):
        """the table holds the addresses of the live statistics: if a storage was replaced (``.to()``, an assigning
        ``load_state_dict``) it is built and uploaded again -- the one case in which ``update()`` allocates"""
        for (_, b, _), ptr in zip(self._stats, self._table_of):
            if b.data_ptr() != ptr:
                self._upload_table()
                return

    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError("ParamEMA.%s while the averaged weights are swapped into the model (inside applied(), or after an "
                               "odd number of swap() calls)" % what)

    # ---- the average ----
    @torch.no_grad()
    def update(self):
        """one update on the current stream, after ``optimizer.step()``: three launches, no allocation, no read-back.  Every
        parameter is averaged, a frozen one or one that is inactive in a grouped optimizer included: the average of a constant is
        that constant.  With a guarded optimizer the update is withheld, on the device, when the step was skipped"""
        self._not_swapped("update()")
        opt = self.opt
        opt._check_views()
        stream, ctl = L.stream_ptr(), self.ctl.data_ptr()
        flag = None if opt.guard is None else opt.guard.ctl.data_ptr() + E.APPLY_OFFSET
        E.advance(ctl, flag, self.decay, self.warmup, stream)
        E.update(self.shadow.data_ptr(), opt.flat.data_ptr(), opt.flat.numel(), ctl, stream)
        if self.stats is not None:
            self._check_table()
            E.update_segs(self._table.data_ptr(), len(self._stats), ctl, stream)

    @torch.no_grad()
    def swap(self):
        """exchange the live and the averaged values in place, on the current stream; a second call restores them"""
        opt = self.opt
        opt._check_views()
        E.swap(self.shadow.data_ptr(), opt.flat.data_ptr(), opt.flat.numel(), L.stream_ptr())
        if self.stats is not None:
            self._check_table()
            E.swap_segs(self._table.data_ptr(), len(self._stats), L.stream_ptr())
        self._swapped = not self._swapped
        # (how many averages are swapped into this model now: a StatsGuard refuses to resolve over them)
        self.model.__dict__["_ube_swapped"] = self.model.__dict__.get("_ube_swapped", 0) + (1 if self._swapped else -1)

    @contextlib.contextmanager
    def applied(self):
        """``with ema.applied():`` the model computes with the averaged weights; they are swapped back on exit, on exceptions
        too.  It does not nest: a second entry is a RuntimeError"""
        self._not_swapped("applied()")
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    @torch.no_grad()
    def copy_to_model(self):
        """one way: the model's parameters (and under ``buffers="average"`` its statistics) become the averaged ones"""
        self._not_swapped("copy_to_model()")
        self.opt._check_views()
        self.opt.flat.copy_(self.shadow)
        for _, b, off in self._stats:
            b.copy_(self._stat_view(b, off))

    @torch.no_grad()
    def reset(self, updates=0):
        """start the average again from the live weights, with `updates` updates on the count (0: the warm-up starts again)"""
        self._not_swapped("reset()")
        self.opt._check_views()
        self.shadow.copy_(self.opt.flat)
        if self.stats is not None:
            self._copy_stats_in()
        E.ctl_init(self.ctl.data_ptr(), int(updates), L.stream_ptr())

    # ---- what the device knows (these sync) ----
    def head(self):
        """the control block's fields as they are now (syncs)"""
        return E.read_ctl(self.ctl.cpu().numpy().tobytes())

    def counts(self):
        """(updates applied, updates withheld) (syncs)"""
        h = self.head()
        return int(h.updates), int(h.held)

    @property
    def updates(self):
        return self.counts()[0]

    @property
    def held(self):
        return self.counts()[1]

    # ---- checkpoints ----
    def _shadow_views(self):
        return {name: self.shadow[o:o + p.numel()].view(p.shape) for name, p, o in self._params}

    def state_dict(self):
        """{"decay", "warmup", "buffers", "updates", "shadow": {parameter name: tensor}, "stats": {buffer name: tensor}}, keyed by
        the model's ``state_dict`` names; "stats" is empty under ``buffers="share"``"""
        self._not_swapped("state_dict()")
        return {"decay": self.decay, "warmup": self.warmup, "buffers": self.buffers, "updates": self.updates,
                "shadow": {name: v.clone() for name, v in self._shadow_views().items()},
                "stats": {name: self._stat_view(b, off).clone() for name, b, off in self._stats}}

    @torch.no_grad()
    def load_state_dict(self, sd):
        """the tensors, the schedule and the count of a ``state_dict()``; ``buffers`` stays what this object was built with"""
        self._not_swapped("load_state_dict()")
        views = self._shadow_views()
        missing = [n for n in views if n not in sd["shadow"]] + [n for n, _, _ in self._stats if n not in sd["stats"]]
        if missing:
            raise KeyError("ParamEMA.load_state_dict: no averaged tensor for %s" % missing[:8])
        self._set_schedule(sd["decay"], sd["warmup"])
        for name, v in views.items():
            v.copy_(sd["shadow"][name])
        for name, b, off in self._stats:
            self._stat_view(b, off).copy_(sd["stats"][name])
        E.ctl_init(self.ctl.data_ptr(), int(sd["updates"]), L.stream_ptr())

    @torch.no_grad()
    def averaged_state_dict(self):
        """a complete model ``state_dict`` with the averaged values in place (``num_batches_tracked``, and under
        ``buffers="share"`` the running statistics, are the live model's)"""
        self._not_swapped("averaged_state_dict()")
        self.opt._check_views()
        out = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        for name, v in self._shadow_views().items():
            out[name].copy_(v)
        for name, b, off in self._stats:
            out[name].copy_(self._stat_view(b, off))
        return out
