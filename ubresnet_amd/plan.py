"""Launch plans: one recorded C++ tape per (network, input shape, dtype, mode) instead of ~560 Python-issued launches.

The reference has no scheduler (each layer is a torch.nn call, models/ub_uresnet.py:88-147; autograd replays them).
Round 1 of this package scheduled the kernels from Python; that costs 10.6 ms of host time per 13.7 ms train step.
Here the FIRST pass of a shape runs the ordinary Python schedule (ubresnet_amd/engine.py) while the C library records
every launch with its resolved arguments (ubr_tape_*, include/ubresnet_hip.h); later passes replay the tape with one
C call.  What makes that legal:

  * every buffer the pass touches is owned by the plan and stays at its address (``Engine._new`` pins allocations made
    while recording; with 288 GB of HBM the ~1 GB/image of a bf16 train step is cheap to keep);
  * the three ops whose operands belong to the caller -- the input image (stem expansion), the fresh log-probability
    tensor (conv11 + LogSoftmax) and the incoming loss gradient (LogSoftmax backward) -- stay off the tape and are issued
    from Python around the replay, so inputs are read in place and outputs are new tensors on every call;
  * the fork/join structure of the two-stream backward and the hand-over points of the data-parallel reducer are tape
    nodes (events), not Python calls.

A plan is used only when it is safe: same parameter/buffer storage as at record time, no forward pass of the same plan
still waiting for its backward, no gradient accumulation into existing ``.grad`` tensors, no launch profiler, no stream
capture.  Everything else takes the ordinary schedule, which stays the reference for the bitwise-equality tests.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import torch

from . import _lib as L
from . import ops
from .engine import wgrad_stream_enabled

ENABLED = os.environ.get("UBR_PLAN", "1") != "0"
MAX_PLANS = 4
TIMED = None      # a list: replays time every launch and append (op, kernel, shape, bytes, flops, seconds) per operator call (bench.py)


class Tape:
    def __init__(self):
        self.h = L.lib().ubr_tape_create()
        if not self.h:
            raise RuntimeError("ubresnet_amd: ubr_tape_create failed")

    def __del__(self):
        try:
            if self.h:
                L.lib().ubr_tape_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @staticmethod
    def _arr(streams):
        return (C.c_void_p * len(streams))(*[int(s) for s in streams])

    def begin(self, streams):
        L.check(L.lib().ubr_tape_begin(self.h, len(streams), self._arr(streams)), "tape_begin")

    def end(self):
        L.check(L.lib().ubr_tape_end(self.h), "tape_end")

    def pause(self):
        L.check(L.lib().ubr_tape_pause(self.h, 1), "tape_pause")

    def resume(self):
        L.check(L.lib().ubr_tape_pause(self.h, 0), "tape_resume")

    def fork(self, a, b):
        L.check(L.lib().ubr_tape_fork(self.h, a, b), "tape_fork")

    def mark(self, slot) -> int:
        m = L.lib().ubr_tape_mark(self.h, slot)
        if m < 0:
            L.check(m, "tape_mark")
        return m

    def replay(self, streams):
        L.check(L.lib().ubr_tape_replay(self.h, len(streams), self._arr(streams)), "tape_replay")

    def size(self) -> int:
        return L.lib().ubr_tape_size(self.h)

    def set_label(self, label: int):
        L.check(L.lib().ubr_tape_set_label(self.h, label), "tape_set_label")

    def replay_timed(self, streams):
        """-> ([ms per node], [label per node]); label -2 = fork / mark node, -1 = launch outside any labelled operator"""
        n = self.size()
        ms, lab = (C.c_float * n)(), (C.c_int32 * n)()
        L.check(L.lib().ubr_tape_replay_timed(self.h, len(streams), self._arr(streams), ms, lab, n), "tape_replay_timed")
        return list(ms), list(lab)


class TapeMark:
    """a point of a replayed stream another stream can wait for (the data-parallel reducer's exchange stream)"""
    __slots__ = ("tape", "idx")

    def __init__(self, tape, idx):
        self.tape, self.idx = tape, idx

    def wait_on(self, stream):
        L.check(L.lib().ubr_tape_wait_mark(self.tape.h, self.idx, stream.cuda_stream), "tape_wait_mark")


class Recording:
    """state of one tape while it records"""

    def __init__(self, nstreams):
        self.tape = Tape()
        self.nstreams = nstreams
        self.keep = []           # every tensor allocated during the pass
        self.stages = []         # backward: (lo, hi, mark on the compute stream, mark on the side stream or None)
        self.pre = None          # callable(s) issued from Python before a replay
        self.post = None         # ... and after it
        self.labels = []         # per labelled operator call: (op, kernel symbol, shape signature, algorithmic bytes, flops)

    def label_begin(self) -> int:
        self.labels.append(None)
        self.tape.set_label(len(self.labels) - 1)
        return len(self.labels) - 1

    def label_end(self, idx: int, meta):
        self.labels[idx] = meta
        self.tape.set_label(-1)

    def operator_names(self):
        """name of every labelled operator call of the pass, in issue order (None: a call that recorded nothing)"""
        return [None if meta is None else meta[0] for meta in self.labels]

    def launches_per_operator(self, streams):
        """[launches on the tape] per labelled operator call, index = position in operator_names().  Replays the tape once
        (the tape's nodes carry the labels; ubr_tape_replay_timed is the C ABI's way to read them back)."""
        _, labs = self.tape.replay_timed(streams)
        out = [0] * len(self.labels)
        for l in labs:
            if l >= 0:
                out[l] += 1
        return out

    def replay(self, streams):
        """ordinary replay, or -- while `TIMED` collects -- a replay with timing events around every launch"""
        if TIMED is None:
            self.tape.replay(streams)
            return
        ms, lab = self.tape.replay_timed(streams)
        per = {}
        for t, l in zip(ms, lab):
            if l >= -1:
                per[l] = per.get(l, 0.0) + t * 1e-3
        for l, sec in per.items():
            meta = self.labels[l] if l >= 0 and self.labels[l] is not None else ("other", "launches outside the timed operators (finalize kernels, memsets)", "", 0, 0.0)
            TIMED.append(meta + (sec,))


class PlannedPass:
    def __init__(self, key, sig):
        self.key, self.sig = key, sig
        self.fwd = None          # Recording
        self.bwd = None
        self.sv = None
        self.flat = self.views = None
        self.in_flight = False
        self.live = None         # weakref to the autograd node's token of the pass in flight (autograd_fn._NetFn)
        self.uses = 0


def _signature(model):
    """device addresses of every parameter and buffer: a plan bakes them in, so a replaced storage or a replaced Parameter
    must retire it.  The module list is walked once (the executor assumes a fixed module tree anyway: its gradient layout is
    built from it); per call only the modules' own parameter / buffer dicts are read -- model.parameters() + model.buffers()
    re-walk the tree through three generator layers and cost ~0.35 ms per call, twice per step."""
    mods = model.__dict__.get("_ubr_modules")
    if mods is None:
        mods = [m for m in model.modules() if m._parameters or m._buffers]
        model.__dict__["_ubr_modules"] = mods
    sig = []
    for m in mods:
        for t in m._parameters.values():
            if t is not None:
                sig.append(t.data_ptr())
        for t in m._buffers.values():
            if t is not None:
                sig.append(t.data_ptr())
        if hasattr(m, "momentum") and hasattr(m, "eps"):
            # host scalars a tape bakes in at record time (Engine._finish_bn): changing them must retire the plan too
            sig.append((m.momentum, m.eps, getattr(m, "track_running_stats", None)))
    return tuple(sig)


def _streams(eng, dev):
    main = L.stream_ptr()
    if eng.side is not None and wgrad_stream_enabled():
        return [main, eng.side.cuda_stream]
    return [main]


@contextlib.contextmanager
def recording(eng, streams):
    """record the eager pass run inside the block onto a new tape: the engine pins its buffers to the Recording, the
    operators label their launches on it"""
    rec = Recording(len(streams))
    eng._rec = rec
    rec.tape.begin(streams)
    ops._rec_sink = rec
    try:
        yield rec
    finally:
        ops._rec_sink = None
        eng._rec = None
        rec.tape.end()


def usable(eng, x) -> bool:
    return (ENABLED and eng.kind in ("uresnet", "aspp") and x.is_cuda and (ops._prof is None or TIMED is not None)
            and not torch.cuda.is_current_stream_capturing())


def forward(eng, x, training, dt, save):
    """-> (out, sv) like Engine.forward, through a plan when one applies"""
    if not usable(eng, x):
        return eng.forward_eager(x, training, dt, save)
    dev = x.device
    if wgrad_stream_enabled():
        eng._ensure_side(dev)
    # (the frozen pattern of the BatchNorm sites, not just the flag: a tape bakes in which launches each site got)
    key = (tuple(x.shape), dt, bool(training), eng.frozen_pattern(training), bool(save), dev.index)
    sig = _signature(eng.model)
    plan = eng._planned.get(key)
    if plan is not None and plan.sig != sig:
        del eng._planned[key]            # parameter or buffer storage was replaced: the baked addresses are stale
        plan = None
    if plan is not None and plan.in_flight and plan.live is not None and plan.live() is None:
        # the pass in flight was dropped without a backward (its autograd node is gone: e.g. a forward with gradients enabled
        # whose loss was never back-propagated, as the reference's validate() does, train_ubresnet2018_wlarcv2.py:428)
        plan.in_flight = False
    if plan is not None and plan.in_flight:
        return eng.forward_eager(x, training, dt, save)      # a second forward before the first one's backward
    streams = _streams(eng, dev)
    if plan is None:
        while len(eng._planned) >= MAX_PLANS:                # oldest plan that is not waiting for its backward
            victims = [k for k, p in eng._planned.items() if not p.in_flight]
            if not victims:
                return eng.forward_eager(x, training, dt, save)
            del eng._planned[min(victims, key=lambda k: eng._planned[k].uses)]
        plan = PlannedPass(key, sig)
        with recording(eng, streams) as rec:
            out, sv = eng.forward_eager(x, training, dt, save)
        plan.fwd, plan.sv = rec, sv
        eng._planned[key] = plan
    else:
        x = eng._check_input(x, eng.model.conv1.in_channels)
        plan.fwd.pre(x)
        plan.fwd.replay(streams)
        out = plan.fwd.post()
        eng._bwd_packed = None           # (an eager backward after a replayed forward repacks its own weight images)
        sv = plan.sv
        if sv is not None:
            sv.x, sv.out = x, out.detach()
    plan.uses += 1
    if save:
        plan.in_flight = True
        plan.live = None
        sv.plan = plan
    return out, sv


def recorded_forward(eng, x, dt):
    """the Recording of the engine's no-grad forward plan for this input shape and dtype (None: not recorded), and the
    streams to replay it on -- for tests and probes that count launches"""
    for key, p in eng._planned.items():
        if key[0] == tuple(x.shape) and key[1] == dt and not key[4] and p.fwd is not None:
            return p.fwd, _streams(eng, x.device)[:p.fwd.nstreams]
    return None, None


def backward(eng, sv, g_out, grad_ready, allow_plan=True):
    plan = getattr(sv, "plan", None)
    if plan is None or plan.sv is not sv:
        return eng.backward_eager(sv, g_out, grad_ready)
    dev = g_out.device
    try:
        if not allow_plan or not usable(eng, g_out) or plan.sig != _signature(eng.model):
            return eng.backward_eager(sv, g_out, grad_ready)
        streams = _streams(eng, dev)
        if plan.bwd is None:
            if len(streams) != plan.fwd.nstreams:
                return eng.backward_eager(sv, g_out, grad_ready)
            with recording(eng, streams) as rec:
                flat, views = eng.backward_eager(sv, g_out, grad_ready)
            plan.bwd, plan.flat, plan.views = rec, flat, views
            return flat, views
        if not g_out.is_contiguous():
            g_out = g_out.contiguous()
        plan.bwd.pre(g_out, sv.out)
        plan.bwd.replay(streams)
        if grad_ready is not None:
            for lo, hi, m0, m1 in plan.bwd.stages:
                marks = (TapeMark(plan.bwd.tape, m0),) + ((TapeMark(plan.bwd.tape, m1),) if m1 is not None else ())
                grad_ready(plan.flat, lo, hi, wait_events=marks, ordered=False)
        return plan.flat, plan.views
    finally:
        plan.in_flight = False
