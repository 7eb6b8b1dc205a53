"""StatsGuard: the BatchNorm running statistics survive a skipped step.

    opt = FlatAdam(model, lr=1e-5, max_grad_norm=1.0, skip_nonfinite=True)
    sg  = StatsGuard(model, optimizer=opt, check_nonfinite=True)
    loss.backward(); reducer.finish(); opt.step(); sg.resolve(); ema.update()

A guarded optimizer keeps a bad batch out of the parameters and the moments, ``ParamEMA`` out of the average -- but the forward
pass of that batch has already written ``running_mean`` / ``running_var`` / ``num_batches_tracked`` of every BatchNorm site, and
one NaN pixel leaves NaN in the stem's statistics: a model that is useless in ``eval()``.  A ``StatsGuard`` keeps a SHADOW of all
these buffers in one flat device buffer and, after each optimizer step, does one of two things, decided on the device:

  commit   shadow <- live: the step stands
  restore  live <- shadow: the statistics go back to what they were before the forward pass (with gradient accumulation: the
           passes) of this step

The rule: restore when the optimizer's guard skipped the step (its ``apply`` flag, read on the device as ``ParamEMA.update`` reads
it), or, with ``check_nonfinite=True``, when a live running_mean / running_var holds an infinity or a NaN; commit otherwise.

``resolve()`` is four launches of libubresnet_stats.so on the current stream (``ubs_scan``, ``ubs_note``, ``ubs_decide``,
``ubs_resolve``; two with ``check_nonfinite=False``), reads nothing back, allocates nothing and passes no argument that depends on
what happened, so it can be captured in a graph next to ``opt.step()`` and ``ema.update()``.

There is no ``state_dict``: at every step boundary the shadow equals the live buffers, which the model's own ``state_dict``
carries.  After anything outside a train step wrote the statistics -- ``model.load_state_dict(...)``,
``reducer.average_bn_stats()``, ``ema.copy_to_model()`` -- call ``resync()``, or the next restore brings the old ones back.

Data parallel.  The statistics, hence the scan's verdict, are per rank; the optimizer's flag is identical on all ranks.  A restore
that only the scan caused leaves the optimizer step of that batch applied (an unguarded optimizer has no way to withhold it).
``resolve()`` while a ``ParamEMA`` has its average swapped into the model (inside ``ema.applied()``) is a usage error and raises.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _ema as E
from . import _lib as L
from . import _stats as S
from .optim import FlatAdam, FlatSGD

__all__ = ["StatsGuard", "stat_rows", "stat_table"]


def _owners(model):
    """[(state_dict name, BatchNorm module, buffer name)] in ``state_dict`` order"""
    return [((prefix + "." if prefix else "") + bname, mod, bname) for prefix, mod in model.named_modules()
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm) for bname, b in mod._buffers.items() if b is not None]


def stat_rows(model):
    """every buffer of the model's BatchNorm modules -> [(state_dict name, tensor, kind, count of 4-byte units)] in
    ``state_dict`` order: a floating-point buffer must be fp32 and is a KIND_F32 row of numel units, an int64 buffer
    (``num_batches_tracked``) a KIND_RAW row of 2 units per element"""
    rows = []
    for name, mod, bname in _owners(model):
        b = mod._buffers[bname]
        if b.is_floating_point():
            if b.dtype != torch.float32:
                raise RuntimeError("ubresnet_amd.bnguard: buffer %s must be float32, got %s" % (name, b.dtype))
            rows.append((name, b, S.KIND_F32, b.numel()))
        elif b.dtype == torch.int64:
            rows.append((name, b, S.KIND_RAW, 2 * b.numel()))
        else:
            raise RuntimeError("ubresnet_amd.bnguard: buffer %s must be float32 or int64, got %s" % (name, b.dtype))
    return rows


def stat_table(rows, shadow_base):
    """the table of ``stat_rows`` rows whose shadows lie back to back from address `shadow_base` -> (numpy array of dtype
    _stats.SEG, offsets in 4-byte units, total units)"""
    offs, at = [], 0
    for _, _, _, count in rows:
        offs.append(at)
        at += count
    t = S.seg_table([shadow_base + 4 * o for o in offs], [b.data_ptr() for _, b, _, _ in rows], [c for _, _, _, c in rows],
                    [k for _, _, k, _ in rows])
    return t, offs, at


def _units(b):
    """a buffer as a flat run of 4-byte units (a view: same storage)"""
    return b.detach().reshape(-1).view(torch.int32)


class StatsGuard(object):
    """a shadow of the model's BatchNorm buffers, committed or restored after each optimizer step; see the module docstring"""

    def __init__(self, model, optimizer=None, check_nonfinite=True):
        if optimizer is not None and not isinstance(optimizer, (FlatAdam, FlatSGD)):
            raise TypeError("StatsGuard needs a ubresnet_amd.optim.FlatAdam or FlatSGD (or None), got %s" % type(optimizer).__name__)
        if optimizer is None and not check_nonfinite:
            raise ValueError("StatsGuard(optimizer=None, check_nonfinite=False) could never restore: there is neither an "
                             "optimizer's flag nor a scan to decide by")
        self.model, self.opt, self.check_nonfinite = model, optimizer, bool(check_nonfinite)
        self._rows = stat_rows(model)
        self._owners = [(mod, bname) for _, mod, bname in _owners(model)]
        if not self._rows:
            raise ValueError("StatsGuard: the model has no BatchNorm buffers")
        dev = self._rows[0][1].device
        for name, b, _, _ in self._rows:
            if b.device != dev or not b.is_contiguous():
                raise RuntimeError("ubresnet_amd.bnguard: buffer %s must be contiguous on %s" % (name, dev))
        self.names = [name for name, _, _, _ in self._rows]
        nseg = len(self._rows)
        self.shadow = torch.zeros(sum(c for _, _, _, c in self._rows), dtype=torch.int32, device=dev)
        self.bad = torch.zeros(nseg, dtype=torch.int32, device=dev)
        self.seen = torch.zeros(nseg, dtype=torch.int32, device=dev)
        self.ctl = torch.zeros(S.CTL_BYTES, dtype=torch.uint8, device=dev)
        self._row = self.ctl.view(torch.int32)[:2]
        self._table = torch.zeros((nseg, 4), dtype=torch.int64, device=dev)
        self._upload_table()
        S.ctl_init(self.ctl.data_ptr(), L.stream_ptr())
        self.resync()

    # ---- helpers ----
    def _upload_table(self):
        t, self._offs, _ = stat_table(self._rows, self.shadow.data_ptr())
        self._table.copy_(torch.from_numpy(t.view(np.int64).reshape(-1, 4).copy()))
        self._table_of = [b.data_ptr() for _, b, _, _ in self._rows]

    @torch.no_grad()
    def _copy_in(self, i):
        _, b, _, count = self._rows[i]
        self.shadow[self._offs[i]:self._offs[i] + count].copy_(_units(b))

    def _check_table(self):
        """the table holds the addresses of the live buffers: if a module's buffer is another tensor or has another storage than
        at the last upload (``.to()``, an assigning ``load_state_dict``, an assignment) it is built and uploaded again and that
        buffer is copied into its shadow -- the one case in which ``resolve()`` allocates"""
        moved = []
        for i, ((mod, bname), ptr) in enumerate(zip(self._owners, self._table_of)):
            b = mod._buffers[bname]
            if b.data_ptr() != ptr:
                name, old, kind, count = self._rows[i]
                if b.dtype != old.dtype or b.numel() != old.numel() or b.device != old.device or not b.is_contiguous():
                    raise RuntimeError("ubresnet_amd.bnguard: buffer %s changed its type, size or device" % name)
                self._rows[i] = (name, b, kind, count)
                moved.append(i)
        if moved:
            self._upload_table()
            for i in moved:
                self._copy_in(i)

    def _not_swapped(self, what):
        if self.model.__dict__.get("_ube_swapped", 0):
            raise RuntimeError("StatsGuard.%s while a ParamEMA has its averaged values swapped into the model (inside applied()): "
                               "the live statistics are the average's, not the training run's" % what)

    def _sites(self, counts):
        return [n for n, c in zip(self.names, counts) if c != 0]

    # ---- the step ----
    @torch.no_grad()
    def resolve(self):
        """after ``optimizer.step()``, on the current stream: scan, decide, commit or restore.  No allocation, no read-back"""
        self._not_swapped("resolve()")
        self._check_table()
        stream, nseg = L.stream_ptr(), len(self._rows)
        table, bad, ctl = self._table.data_ptr(), self.bad.data_ptr(), self.ctl.data_ptr()
        if self.check_nonfinite:
            S.scan(table, nseg, bad, stream)
            S.note(self.seen.data_ptr(), bad, nseg, stream)
        guard = None if self.opt is None else self.opt.guard
        flag = None if guard is None else guard.ctl.data_ptr() + E.APPLY_OFFSET
        S.decide(ctl, bad, nseg, flag, self.check_nonfinite, stream)
        S.resolve(table, nseg, ctl, stream)

    @torch.no_grad()
    def resync(self):
        """shadow <- live now, unconditionally: after anything outside a train step wrote the statistics.  Reads the scan back
        once (syncs) and raises a ValueError naming the sites if a live statistic is non-finite: a shadow taken from poisoned
        statistics would restore poison forever"""
        self._not_swapped("resync()")
        self._check_table()
        S.scan(self._table.data_ptr(), len(self._rows), self.bad.data_ptr(), L.stream_ptr())
        sites = self._sites(self.bad.cpu().tolist())
        if sites:
            raise ValueError("StatsGuard: the running statistics are already non-finite at %s" % ", ".join(sites))
        for i in range(len(self._rows)):
            self._copy_in(i)
        self.seen.zero_()

    # ---- what the device knows ----
    def row(self):
        """device int32 view [keep, bad_rows] of the last decision: copy it into a log buffer on the stream"""
        return self._row

    def head(self):
        """the control block's fields as they are now (syncs)"""
        return S.read_ctl(self.ctl.cpu().numpy().tobytes())

    def read(self):
        """-> dict of kept, restored, restored_for_stats, bad_rows (at the last decision), bad_sites (names of the buffers that
        held a non-finite value at any decision since construction or the last ``resync()``) and bad_sites_last (at the last
        decision) (syncs)"""
        h = self.head()
        return dict(kept=int(h.kept), restored=int(h.restored), restored_for_stats=int(h.restored_for_stats), bad_rows=int(h.bad_rows),
                    bad_sites=self._sites(self.seen.cpu().tolist()), bad_sites_last=self._sites(self.bad.cpu().tolist()))
