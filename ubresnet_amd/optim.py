"""Flat optimizers: the whole network's parameters in ONE fp32 buffer, one HIP launch per step.

The reference trains with ``torch.optim.Adam(model.parameters(), lr=1e-5, weight_decay=1e-4)``
(training/train_ubresnet2018_wlarcv2.py:155-157) and, in the LArCV1 scripts, ``torch.optim.SGD(..., momentum=0.9,
weight_decay=1e-4)`` (training/train_ubresnet2018_wlarcv1.py:127-129).  The backward pass of this package already
leaves every gradient as a view of one flat buffer (ordered by completion time, so data-parallel buckets can leave
early); ``FlatAdam`` / ``FlatSGD`` re-point every ``parameter.data`` at a view of a parameter buffer with the SAME
layout, so an optimizer step is a single streaming kernel over (param, grad, state) -- ``ubr_adam_step`` /
``ubr_sgd_step`` -- instead of a multi-tensor launch sequence over 165 tensors.

    opt = FlatAdam(model, lr=1e-5, weight_decay=1e-4)        # after model.to(device)
    loss.backward(); reducer.finish(); opt.step(); opt.zero_grad()

Arithmetic is torch.optim's (L2 weight decay added to the gradient; Adam bias corrections; SGD's first step copies
the gradient into the momentum buffer).  ``state_dict()`` / ``load_state_dict()`` use torch.optim's layout (per
parameter ``step`` / ``exp_avg`` / ``exp_avg_sq`` or ``momentum_buffer``, parameters numbered in
``model.parameters()`` order), so optimizer state in a reference checkpoint
(``{"iter","epoch","state_dict","best_prec1","optimizer"}``, wlarcv2.py:474-479) loads and saves unchanged.

Guarded step.  ``FlatAdam(..., max_grad_norm=1.0, skip_nonfinite=True)`` (either argument, likewise on ``FlatSGD``) makes
``step()`` two calls into libubresnet_opt.so on the current stream: ``ubo_grad_norm`` takes the global L2 norm of the flat
gradient (fp64 accumulation, bitwise reproducible) and decides ON THE DEVICE whether the step is applied and by how much the
gradient is scaled (torch's ``clip_grad_norm_`` coefficient); ``ubo_adam_step`` / ``ubo_sgd_step`` then do the arithmetic of
the unguarded kernels, or nothing at all.  The host reads nothing: no sync, no allocation after the first step, and no launch
argument depends on the step count (Adam's bias corrections come from a table on the device, indexed by the count of APPLIED
steps), so the pair can be captured in a graph.  ``opt.steps`` counts attempts; ``opt.guard`` has the device control block,
``row()`` for recorders and ``read()`` (which syncs).  With both arguments at their defaults nothing changes.

Data parallel: call ``step()`` after ``reducer.finish()``, as ``training.epoch.train`` does.  Every rank then holds the same
reduced gradient bytes, the norm is a deterministic function of those bytes, and all ranks take the same decision without a
collective of their own.  A skipped step does not undo what the forward pass already did: BatchNorm running statistics were
updated there.

Parameter groups and frozen parameters.  ``groups=[{"params": [...], "lr": ...}, ...]`` (torch.optim's list of dicts; see also
``split_decay``) moves the step to libubresnet_group.so: still one launch over the flat buffers, which a static tile table cuts
at the parameters' boundaries, with the learning rate, the weight decay, an on/off switch and the count of applied steps PER
PARAMETER on the device.  A group may override ``lr`` and ``weight_decay``; every other hyper-parameter is optimizer-wide.
``opt.param_groups`` is torch.optim's list, so ``lr_scheduler`` and ``g["lr"] = ...`` work per group; the next ``step()`` uploads
what changed.  At each ``step()`` a parameter whose ``.grad is None`` (``requires_grad=False``, or a gradient set to ``None``),
like one that is in no group, is inactive for that step: no byte of the parameter, its moments or momentum buffer is read or
written, its count stays, and its stale bytes in the flat gradient buffer do not enter the gradient norm.  The set may change
from step to step; a parameter unfrozen at step 100 starts at ``step = 1`` with the bias corrections of a first step, as under
torch.optim.  The guard acts on the norm over the active parameters; a skipped step advances no count.  ``state_dict()`` has
torch's layout and numbering (across the groups in the order given, no state entry for a parameter that never stepped) and
interchanges with ``torch.optim.Adam(groups)`` / ``torch.optim.SGD(groups)``.  Under a captured graph the learning rates are the
ones uploaded before the capture: change them outside the graph.  Data parallel: nothing new -- every rank holds the same
reduced bytes and the same ``.grad is None`` pattern, so all ranks decide alike.  With ``groups=None`` (the default) nothing of
this is used and every path, launch and error is as before.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _group as G
from . import _lib as L
from . import _opt as O

__all__ = ["FlatAdam", "FlatSGD", "grad_norm", "split_decay"]


def _kind_of(model) -> str:
    return "aspp" if hasattr(model, "ASPP_layer_enc3") else "uresnet"


def _flat_grad_of(model, layout, numel, device, scratch):
    """-> (flat gradient, scratch): the flat gradient buffer of the last backward if every .grad is still its view, else a
    gathered copy in `scratch` (allocated on first use); (None, scratch) if no parameter has a gradient"""
    g = model.__dict__.get("_ubr_flat_grad")
    ok = g is not None and g.numel() == numel and g.device == device
    if ok:
        base = g.data_ptr()
        for _, p, o in layout:
            if p.grad is None or p.grad.data_ptr() != base + 4 * o:
                ok = False
                break
    if ok:
        return g, scratch
    have = [p.grad is not None for _, p, _ in layout]
    if not any(have):
        return None, scratch          # torch.optim skips parameters without a gradient: nothing to do
    if not all(have):
        raise RuntimeError("ubresnet_amd.optim: some parameters have no gradient (frozen / requires_grad=False); the flat "
                           "one-launch step updates every parameter -- use torch.optim for partially frozen models")
    if scratch is None:
        scratch = torch.zeros(numel, dtype=torch.float32, device=device)
    else:
        scratch.zero_()
    for _, p, o in layout:
        scratch[o:o + p.numel()].copy_(p.grad.reshape(-1))
    return scratch, scratch


class _Guard(object):
    """the device side of a guarded optimizer: the control block of libubresnet_opt.so and the bias-correction table"""

    def __init__(self, device, max_grad_norm, skip_nonfinite):
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError("max_grad_norm must be None or >= 0, got %r" % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ctl = torch.zeros(O.CTL_BYTES, dtype=torch.uint8, device=device)
        self._row = self.ctl[64:80].view(torch.float32)[:3]
        self._betas = self._table = None
        self.set_applied(0)

    def set_applied(self, applied):
        """zero the block and start counting applied steps from `applied`"""
        O.ctl_init(self.ctl.data_ptr(), applied, L.stream_ptr())

    def table(self, beta1=0.0, beta2=0.0):
        """(address, rows) of the device table for these betas; uploaded once and again whenever they change"""
        key = (float(beta1), float(beta2))
        if key != self._betas:
            self._table = torch.from_numpy(O.bias_table(*key)).to(self.ctl.device)
            self._betas = key
        return self._table.data_ptr(), self._table.shape[0]

    def norm(self, g, grad_scale, bc):
        O.grad_norm(g.data_ptr(), g.numel(), grad_scale, self.max_grad_norm, self.skip_nonfinite, bc[0], bc[1],
                    self.ctl.data_ptr(), L.stream_ptr())

    def row(self):
        """device fp32 view of [norm, scale, apply (0.0 / 1.0)] of the last step"""
        return self._row

    def head(self):
        """the block's fields as they are now (syncs)"""
        return O.read_ctl(self.ctl[:O.CTL_HEAD_BYTES].cpu().numpy().tobytes())

    def read(self):
        """-> dict of norm, scale, applied, skipped, clipped_total (syncs)"""
        h = self.head()
        return dict(norm=h.norm, scale=h.scale, applied=h.applied, skipped=h.skipped, clipped_total=h.clipped_total)


def grad_norm(model):
    """global L2 norm of the model's gradients as a 0-dim fp32 device tensor: ubo_grad_norm's reduction (fp64 accumulation,
    bitwise reproducible, no host sync) over the flat gradient buffer of the last backward, or over a gathered copy if the
    .grad tensors are no longer its views -- for training loops that step with torch.optim"""
    from .autograd_fn import _engine
    st = model.__dict__.get("_ubo_grad_norm")
    if st is None:
        eng = _engine(model, _kind_of(model))
        layout = [(name, p, eng.grad_offsets[name]) for name, p in eng.grad_order]
        st = model.__dict__["_ubo_grad_norm"] = dict(layout=layout, numel=eng.grad_numel, scratch=None, guard=None)
    dev = st["layout"][0][1].device
    g, st["scratch"] = _flat_grad_of(model, st["layout"], st["numel"], dev, st["scratch"])
    if g is None:
        raise RuntimeError("ubresnet_amd.optim.grad_norm: no parameter has a gradient")
    if st["guard"] is None or st["guard"].ctl.device != dev:
        st["guard"] = _Guard(dev, None, False)
    guard = st["guard"]
    guard.norm(g, 1.0, guard.table())
    return guard.row()[0].clone()


def split_decay(model, weight_decay):
    """-> two groups for ``groups=``: the weights of the convolutions and transposed convolutions with `weight_decay`, every
    BatchNorm weight and every bias with 0.0 (parameters in ``model.parameters()`` order inside each group)"""
    from torch.nn.modules.conv import _ConvNd
    decay = set()
    for mod in model.modules():
        if isinstance(mod, _ConvNd) and mod.weight is not None:
            decay.add(id(mod.weight))
    params = list(model.parameters())
    return [{"params": [p for p in params if id(p) in decay], "weight_decay": float(weight_decay)},
            {"params": [p for p in params if id(p) not in decay], "weight_decay": 0.0}]


def _same_value(a, b):
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        return isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same_value(x, y) for x, y in zip(a, b))
    return a == b


def _check_groups(model_params, groups, defaults):
    """torch.optim's list of group dicts, checked against the model: -> a list of fresh dicts.  ValueError for a group without
    "params", a parameter listed twice or not of the model, a key that is no hyper-parameter, and an override of anything but
    lr and weight_decay"""
    if isinstance(groups, dict) or not isinstance(groups, (list, tuple)) or not groups or not all(isinstance(g, dict) for g in groups):
        raise ValueError("groups must be a non-empty list of dicts, each with \"params\"")
    of_model = {id(p) for p in model_params}
    seen, out = set(), []
    for k, g in enumerate(groups):
        if "params" not in g:
            raise ValueError("group %d has no \"params\"" % k)
        ps = g["params"]
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        for p in ps:
            if id(p) not in of_model:
                raise ValueError("group %d lists a parameter that does not belong to the model" % k)
            if id(p) in seen:
                raise ValueError("group %d lists a parameter that is already in a group" % k)
            seen.add(id(p))
        for key, val in g.items():
            if key in ("params", "lr", "weight_decay"):
                continue
            if key not in defaults:
                raise ValueError("group %d: %r is not a hyper-parameter of this optimizer" % (k, key))
            if not _same_value(val, defaults[key]):
                raise ValueError("group %d: %r is optimizer-wide (%r); a group may override lr and weight_decay only" % (k, key, defaults[key]))
        out.append(dict(g, params=ps))
    return out


class _Grouped(object):
    """the device side of a grouped optimizer (libubresnet_group.so): the tile table, the per-segment hyper-parameters (host
    written) and step counts (device written), the control block and the bias-correction table.  One segment per entry of the
    gradient layout.  It has _Guard's interface (ctl, row(), head(), read()), so recorders treat it as one."""

    def __init__(self, layout, device, max_grad_norm, skip_nonfinite):
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError("max_grad_norm must be None or >= 0, got %r" % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = max_grad_norm is not None or bool(skip_nonfinite)
        self.nseg = len(layout)
        tiles = G.plan_tiles([o // 4 for _, _, o in layout], [(p.numel() + 3) // 4 for _, p, _ in layout])
        self.ntiles = len(tiles)
        self.tiles = torch.from_numpy(tiles.view(np.int32).reshape(-1, 4).copy()).to(device)       # built once, uploaded once
        self._pinned = torch.zeros((self.nseg, 4), dtype=torch.int32).pin_memory()
        self._host = self._pinned.numpy().reshape(-1).view(G.HYPER)
        self._sent = None                                   # what the device holds
        self._copied = torch.cuda.Event()
        self.hyper = torch.zeros((self.nseg, 4), dtype=torch.int32, device=device)
        self.state = torch.zeros((self.nseg, 4), dtype=torch.int32, device=device)
        self.ctl = torch.zeros(G.CTL_BYTES, dtype=torch.uint8, device=device)
        self._row = self.ctl[64:80].view(torch.float32)[:3]
        self._betas = self._table = None

    def table(self, beta1=0.0, beta2=0.0):
        """(address, rows) of the device table for these betas; uploaded once and again whenever they change"""
        key = (float(beta1), float(beta2))
        if key != self._betas:
            self._table = torch.from_numpy(O.bias_table(*key)).to(self.ctl.device)
            self._betas = key
        return self._table.data_ptr(), self._table.shape[0]

    def set_hyper(self, lr, weight_decay, active):
        """per-segment arrays -> the device, from pinned memory on the current stream, only if anything changed"""
        want = np.zeros(self.nseg, dtype=G.HYPER)
        want["lr"], want["weight_decay"], want["active"] = lr, weight_decay, active
        if self._sent is not None and want.tobytes() == self._sent:
            return
        self._copied.synchronize()                          # the last upload has left the pinned buffer
        self._host[:] = want
        self.hyper.copy_(self._pinned, non_blocking=True)
        self._copied.record()
        self._sent = want.tobytes()

    def set_counts(self, counts, bc):
        """zero the control block and seed every segment's count (a checkpoint's); the head counts from the largest"""
        counts = np.asarray(counts, dtype=np.int64)
        dev = torch.from_numpy(counts).to(self.ctl.device)
        G.state_set(self.state.data_ptr(), self.nseg, 0, self.nseg, dev.data_ptr(), bc[0], bc[1], L.stream_ptr())
        self.ctl.zero_()
        self.ctl[40:48].view(torch.int64).fill_(int(counts.max()))
        torch.cuda.current_stream(self.ctl.device).synchronize()        # `dev` is freed on return

    def counts(self):
        """applied steps per segment (syncs)"""
        return G.state_get(self.state.data_ptr(), self.nseg, L.stream_ptr())["applied"]

    def decide(self, g, numel, grad_scale, bc):
        """the guarded norm over the active segments, or the bookkeeping launch alone"""
        if self.guarded:
            G.grad_norm(g.data_ptr(), numel, self.tiles.data_ptr(), self.ntiles, self.hyper.data_ptr(), self.state.data_ptr(), self.nseg,
                        grad_scale, self.max_grad_norm, self.skip_nonfinite, bc[0], bc[1], self.ctl.data_ptr(), L.stream_ptr())
        else:
            G.advance(self.hyper.data_ptr(), self.state.data_ptr(), self.nseg, grad_scale, bc[0], bc[1], self.ctl.data_ptr(), L.stream_ptr())

    def row(self):
        """device fp32 view of [norm, scale, apply (0.0 / 1.0)] of the last step"""
        return self._row

    def head(self):
        """the block's fields as they are now (syncs)"""
        return G.read_ctl(self.ctl[:G.CTL_HEAD_BYTES].cpu().numpy().tobytes())

    def read(self):
        """-> dict of norm, scale, applied, skipped, clipped_total (syncs)"""
        h = self.head()
        return dict(norm=h.norm, scale=h.scale, applied=h.applied, skipped=h.skipped, clipped_total=h.clipped_total)


class _FlatOptimizer(torch.optim.Optimizer):
    def __init__(self, model, defaults, max_grad_norm=None, skip_nonfinite=False, groups=None):
        from .autograd_fn import _engine
        params = list(model.parameters())
        if not params:
            raise ValueError("optimizer got a model without parameters")
        dev = params[0].device
        for p in params:
            if p.dtype != torch.float32 or p.device != dev or not p.is_cuda:
                raise RuntimeError("ubresnet_amd.optim: parameters must be float32 on one ROCm device (move the model first)")
        if groups is not None:
            groups = _check_groups(params, groups, defaults)
        super().__init__(params if groups is None else groups, defaults)
        self.model = model
        eng = _engine(model, _kind_of(model))
        self._layout = [(name, p, eng.grad_offsets[name]) for name, p in eng.grad_order]
        self._numel = eng.grad_numel
        if len(self._layout) != len(params):
            raise RuntimeError("ubresnet_amd.optim: gradient layout does not cover every parameter")
        # torch.optim numbering (state_dict): model.parameters() order, or across the groups in the order given
        numbered = params if groups is None else [p for g in self.param_groups for p in g["params"]]
        self._index = {id(p): i for i, p in enumerate(numbered)}
        self.flat = torch.zeros(self._numel, dtype=torch.float32, device=dev)
        self._adopt()
        self._scratch = None
        self.steps = 0
        # both at their defaults: the unguarded ubr_*_step path, unchanged; else the device-side guard
        if groups is not None:
            self._grouped = _Grouped(self._layout, dev, max_grad_norm, skip_nonfinite)
            self.guard = self._grouped if self._grouped.guarded else None
        else:
            self._grouped = None
            self.guard = _Guard(dev, max_grad_norm, skip_nonfinite) if (max_grad_norm is not None or skip_nonfinite) else None

    # parameters become views of self.flat (values preserved)
    def _adopt(self):
        with torch.no_grad():
            for _, p, o in self._layout:
                n = p.numel()
                v = self.flat[o:o + n].view(p.shape)
                if p.data_ptr() != v.data_ptr():
                    v.copy_(p.data)
                    p.data = v

    def _flat_grad(self):
        """the flat gradient buffer of the last backward if every .grad is still its view, else a gathered copy"""
        g, self._scratch = _flat_grad_of(self.model, self._layout, self._numel, self.flat.device, self._scratch)
        return g

    def _check_views(self):
        base = self.flat.data_ptr()
        for _, p, o in self._layout:
            if p.data_ptr() != base + 4 * o:
                self._adopt()            # e.g. load_state_dict / .to() replaced parameter storage
                return

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none=set_to_none)

    # ---- torch.optim-compatible state (per-parameter views of the flat state buffers) ----
    def _state_views(self, buf):
        return {self._index[id(p)]: buf[o:o + p.numel()].view(p.shape) for _, p, o in self._layout if id(p) in self._index}

    # ---- parameter groups (libubresnet_group.so) ----
    _SHARED = ()            # the hyper-parameters no group may override

    def _grouped_begin(self):
        """what a grouped step() needs: -> the flat gradient, or None if no parameter of a group has a gradient.  Uploads the
        per-segment lr / weight_decay / active switch if they changed"""
        first = self.param_groups[0]
        for k, grp in enumerate(self.param_groups):
            for key in self._SHARED:
                if not _same_value(grp[key], first[key]):
                    raise ValueError("group %d: %r differs from group 0's; it is optimizer-wide" % (k, key))
        of = {id(p): k for k, grp in enumerate(self.param_groups) for p in grp["params"]}
        seg_group = [of.get(id(p), -1) for _, p, _ in self._layout]
        active = [k >= 0 and p.grad is not None for k, (_, p, _) in zip(seg_group, self._layout)]
        if not any(active):
            return None
        g = self.model.__dict__.get("_ubr_flat_grad")
        ok = g is not None and g.numel() == self._numel and g.device == self.flat.device
        if ok:
            base = g.data_ptr()
            ok = all(p.grad.data_ptr() == base + 4 * o for a, (_, p, o) in zip(active, self._layout) if a)
        if not ok:                                          # gather the active gradients; the rest of the scratch is never read
            if self._scratch is None:
                self._scratch = torch.zeros(self._numel, dtype=torch.float32, device=self.flat.device)
            else:
                self._scratch.zero_()
            for a, (_, p, o) in zip(active, self._layout):
                if a:
                    self._scratch[o:o + p.numel()].copy_(p.grad.reshape(-1))
            g = self._scratch
        lr = [float(self.param_groups[k]["lr"]) if k >= 0 else 0.0 for k in seg_group]
        wd = [float(self.param_groups[k]["weight_decay"]) if k >= 0 else 0.0 for k in seg_group]
        self._grouped.set_hyper(lr, wd, [1 if a else 0 for a in active])
        return g

    def _grouped_param_groups(self):
        out = []
        for grp in self.param_groups:
            d = {k: v for k, v in grp.items() if k != "params"}
            d["params"] = [self._index[id(p)] for p in grp["params"]]
            out.append(d)
        return out

    def _grouped_load_groups(self, sd, keys):
        saved = sd["param_groups"]
        if len(saved) != len(self.param_groups):
            raise ValueError("loaded state dict has %d parameter groups, the optimizer has %d" % (len(saved), len(self.param_groups)))
        for grp, mine in zip(saved, self.param_groups):
            if len(grp["params"]) != len(mine["params"]):
                raise ValueError("loaded state dict has a parameter group whose size does not match the optimizer's")
            for k in keys:
                if k in grp:
                    mine[k] = grp[k]

    def _segment_of(self):
        """torch.optim number -> segment"""
        return {self._index[id(p)]: s for s, (_, p, _) in enumerate(self._layout) if id(p) in self._index}


class FlatAdam(_FlatOptimizer):
    _SHARED = ("betas", "eps")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False,
                 groups=None):
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_grad_norm, skip_nonfinite, groups)
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        if self.guard is not None or self._grouped is not None:
            (self.guard or self._grouped).table(float(betas[0]), float(betas[1]))         # uploaded here: step() allocates nothing

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = closure() if closure is not None else None
        self._check_views()
        if self._grouped is not None:
            g = self._grouped_begin()
            if g is None:
                return loss
            grp, gr = self.param_groups[0], self._grouped
            self.steps += 1
            b1, b2 = float(grp["betas"][0]), float(grp["betas"][1])
            gr.decide(g, self._numel, grad_scale, gr.table(b1, b2))
            G.adam_step(self.flat.data_ptr(), g.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self._numel,
                        gr.tiles.data_ptr(), gr.ntiles, gr.hyper.data_ptr(), gr.state.data_ptr(), gr.nseg, b1, b2, grp["eps"],
                        gr.ctl.data_ptr(), L.stream_ptr())
            return loss
        g = self._flat_grad()
        if g is None:
            return loss
        grp = self.param_groups[0]
        self.steps += 1
        if self.guard is not None:
            b1, b2 = float(grp["betas"][0]), float(grp["betas"][1])
            self.guard.norm(g, grad_scale, self.guard.table(b1, b2))
            O.adam_step(self.flat.data_ptr(), g.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self._numel,
                        grp["lr"], b1, b2, grp["eps"], grp["weight_decay"], self.guard.ctl.data_ptr(), L.stream_ptr())
            return loss
        L.check(L.lib().ubr_adam_step(self.flat.data_ptr(), g.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                      self._numel, float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1]), float(grp["eps"]),
                                      float(grp["weight_decay"]), self.steps, float(grad_scale), L.stream_ptr()), "adam_step")
        return loss

    def state_dict(self):
        m, v = self._state_views(self.exp_avg), self._state_views(self.exp_avg_sq)
        if self._grouped is not None:                   # per-parameter step counts, from the device
            counts = self._grouped.counts()
            state = {i: {"step": torch.tensor(float(counts[s])), "exp_avg": m[i].clone(), "exp_avg_sq": v[i].clone()}
                     for i, s in sorted(self._segment_of().items()) if counts[s] > 0}
            return {"state": state, "param_groups": self._grouped_param_groups()}
        n = len(self._index)
        state = {}
        if self.steps > 0:
            step = self.steps if self.guard is None else self.guard.head().applied     # a guarded step may have been skipped
            state = {i: {"step": torch.tensor(float(step)), "exp_avg": m[i].clone(), "exp_avg_sq": v[i].clone()} for i in range(n)}
        grp = {k: v_ for k, v_ in self.param_groups[0].items() if k != "params"}
        grp["params"] = list(range(n))
        return {"state": state, "param_groups": [grp]}

    def load_state_dict(self, sd):
        if self._grouped is not None:
            self._grouped_load_groups(sd, ("lr", "betas", "eps", "weight_decay"))
            self.exp_avg.zero_()                    # a parameter without a saved state starts from zeros, as under torch.optim
            self.exp_avg_sq.zero_()
            m, v = self._state_views(self.exp_avg), self._state_views(self.exp_avg_sq)
            seg, counts = self._segment_of(), np.zeros(self._grouped.nseg, dtype=np.int64)
            for i, st in sd.get("state", {}).items():
                i = int(i)
                m[i].copy_(st["exp_avg"])
                v[i].copy_(st["exp_avg_sq"])
                counts[seg[i]] = int(float(st["step"]))
            self.steps = int(counts.max())
            betas = self.param_groups[0]["betas"]
            self._grouped.set_counts(counts, self._grouped.table(float(betas[0]), float(betas[1])))
            return
        grp = sd["param_groups"][0]
        for k in ("lr", "betas", "eps", "weight_decay"):
            if k in grp:
                self.param_groups[0][k] = grp[k]
        m, v = self._state_views(self.exp_avg), self._state_views(self.exp_avg_sq)
        self.steps = 0
        for i, st in sd.get("state", {}).items():
            i = int(i)
            m[i].copy_(st["exp_avg"])
            v[i].copy_(st["exp_avg_sq"])
            self.steps = max(self.steps, int(float(st["step"])))
        if self.guard is not None:
            self.guard.set_applied(self.steps)


class FlatSGD(_FlatOptimizer):
    _SHARED = ("momentum", "dampening", "nesterov")

    def __init__(self, model, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, max_grad_norm=None,
                 skip_nonfinite=False, groups=None):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(model, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov),
                         max_grad_norm, skip_nonfinite, groups)
        self.momentum_buffer = torch.zeros_like(self.flat) if momentum != 0 else None
        if self.guard is not None or self._grouped is not None:
            (self.guard or self._grouped).table()                      # one row: SGD has no bias correction

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = closure() if closure is not None else None
        self._check_views()
        if self._grouped is not None:               # a segment's first step is its own first APPLIED one: the device knows
            g = self._grouped_begin()
            if g is None:
                return loss
            grp, gr = self.param_groups[0], self._grouped
            if (grp["momentum"] != 0) != (self.momentum_buffer is not None):
                raise ValueError("momentum cannot be switched on or off after construction")
            self.steps += 1
            gr.decide(g, self._numel, grad_scale, gr.table())
            G.sgd_step(self.flat.data_ptr(), g.data_ptr(), L.ptr(self.momentum_buffer), self._numel, gr.tiles.data_ptr(), gr.ntiles,
                       gr.hyper.data_ptr(), gr.state.data_ptr(), gr.nseg, grp["momentum"], grp["dampening"], grp["nesterov"],
                       gr.ctl.data_ptr(), L.stream_ptr())
            return loss
        g = self._flat_grad()
        if g is None:
            return loss
        grp = self.param_groups[0]
        first = self.steps == 0
        self.steps += 1
        if self.guard is not None:              # the first step is the first APPLIED one: the device knows which that is
            self.guard.norm(g, grad_scale, self.guard.table())
            O.sgd_step(self.flat.data_ptr(), g.data_ptr(), L.ptr(self.momentum_buffer), self._numel, grp["lr"], grp["momentum"],
                       grp["dampening"], grp["weight_decay"], grp["nesterov"], self.guard.ctl.data_ptr(), L.stream_ptr())
            return loss
        L.check(L.lib().ubr_sgd_step(self.flat.data_ptr(), g.data_ptr(), L.ptr(self.momentum_buffer), self._numel, float(grp["lr"]),
                                     float(grp["momentum"]), float(grp["dampening"]), float(grp["weight_decay"]),
                                     1 if grp["nesterov"] else 0, 1 if first else 0, float(grad_scale), L.stream_ptr()), "sgd_step")
        return loss

    def state_dict(self):
        if self._grouped is not None:
            state = {}
            if self.momentum_buffer is not None:
                b, counts = self._state_views(self.momentum_buffer), self._grouped.counts()
                state = {i: {"momentum_buffer": b[i].clone()} for i, s in sorted(self._segment_of().items()) if counts[s] > 0}
            return {"state": state, "param_groups": self._grouped_param_groups()}
        n = len(self._index)
        state = {}
        if self.momentum_buffer is not None and self.steps > 0 and (self.guard is None or self.guard.head().applied > 0):
            b = self._state_views(self.momentum_buffer)
            state = {i: {"momentum_buffer": b[i].clone()} for i in range(n)}
        grp = {k: v_ for k, v_ in self.param_groups[0].items() if k != "params"}
        grp["params"] = list(range(n))
        return {"state": state, "param_groups": [grp]}

    def load_state_dict(self, sd):
        if self._grouped is not None:               # a parameter with a momentum buffer has had its first step
            self._grouped_load_groups(sd, ("lr", "momentum", "dampening", "weight_decay", "nesterov"))
            seg, counts = self._segment_of(), np.zeros(self._grouped.nseg, dtype=np.int64)
            if self.momentum_buffer is not None:
                self.momentum_buffer.zero_()
                b = self._state_views(self.momentum_buffer)
                for i, st in sd.get("state", {}).items():
                    if st.get("momentum_buffer") is not None:
                        b[int(i)].copy_(st["momentum_buffer"])
                        counts[seg[int(i)]] = 1
            self.steps = int(counts.max())
            self._grouped.set_counts(counts, self._grouped.table())
            return
        grp = sd["param_groups"][0]
        for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov"):
            if k in grp:
                self.param_groups[0][k] = grp[k]
        if self.momentum_buffer is not None:
            b = self._state_views(self.momentum_buffer)
            for i, st in sd.get("state", {}).items():
                if st.get("momentum_buffer") is not None:
                    b[int(i)].copy_(st["momentum_buffer"])
                    self.steps = max(self.steps, 1)
        if self.guard is not None:
            self.guard.set_applied(min(self.steps, 1))
