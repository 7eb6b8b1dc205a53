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
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import _opt as O

__all__ = ["FlatAdam", "FlatSGD", "grad_norm"]


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


class _FlatOptimizer(torch.optim.Optimizer):
    def __init__(self, model, defaults, max_grad_norm=None, skip_nonfinite=False):
        from .autograd_fn import _engine
        params = list(model.parameters())
        if not params:
            raise ValueError("optimizer got a model without parameters")
        dev = params[0].device
        for p in params:
            if p.dtype != torch.float32 or p.device != dev or not p.is_cuda:
                raise RuntimeError("ubresnet_amd.optim: parameters must be float32 on one ROCm device (move the model first)")
        super().__init__(params, defaults)
        self.model = model
        eng = _engine(model, _kind_of(model))
        self._layout = [(name, p, eng.grad_offsets[name]) for name, p in eng.grad_order]
        self._numel = eng.grad_numel
        if len(self._layout) != len(params):
            raise RuntimeError("ubresnet_amd.optim: gradient layout does not cover every parameter")
        self._index = {id(p): i for i, p in enumerate(params)}          # torch.optim numbering (state_dict)
        self.flat = torch.zeros(self._numel, dtype=torch.float32, device=dev)
        self._adopt()
        self._scratch = None
        self.steps = 0
        # both at their defaults: the unguarded ubr_*_step path, unchanged; else the device-side guard
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
        return {self._index[id(p)]: buf[o:o + p.numel()].view(p.shape) for _, p, o in self._layout}


class FlatAdam(_FlatOptimizer):
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False):
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_grad_norm, skip_nonfinite)
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        if self.guard is not None:
            self.guard.table(float(betas[0]), float(betas[1]))         # uploaded here: step() allocates nothing

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = closure() if closure is not None else None
        self._check_views()
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
        n = len(self._index)
        state = {}
        if self.steps > 0:
            step = self.steps if self.guard is None else self.guard.head().applied     # a guarded step may have been skipped
            state = {i: {"step": torch.tensor(float(step)), "exp_avg": m[i].clone(), "exp_avg_sq": v[i].clone()} for i in range(n)}
        grp = {k: v_ for k, v_ in self.param_groups[0].items() if k != "params"}
        grp["params"] = list(range(n))
        return {"state": state, "param_groups": [grp]}

    def load_state_dict(self, sd):
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
    def __init__(self, model, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, max_grad_norm=None,
                 skip_nonfinite=False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(model, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov),
                         max_grad_norm, skip_nonfinite)
        self.momentum_buffer = torch.zeros_like(self.flat) if momentum != 0 else None
        if self.guard is not None:
            self.guard.table()                                         # one row: SGD has no bias correction

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = closure() if closure is not None else None
        self._check_views()
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
        n = len(self._index)
        state = {}
        if self.momentum_buffer is not None and self.steps > 0 and (self.guard is None or self.guard.head().applied > 0):
            b = self._state_views(self.momentum_buffer)
            state = {i: {"momentum_buffer": b[i].clone()} for i in range(n)}
        grp = {k: v_ for k, v_ in self.param_groups[0].items() if k != "params"}
        grp["params"] = list(range(n))
        return {"state": state, "param_groups": [grp]}

    def load_state_dict(self, sd):
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
