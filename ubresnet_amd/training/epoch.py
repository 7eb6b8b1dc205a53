"""The reference's epoch loops over a batch stager: ``train`` (training/train_ubresnet2018_wlarcv2.py:298-397), ``validate``
(:399-471, repaired: as checked in it reads undefined names) and ``AverageMeter`` (:482-497).

    with BatchStager(loader, 16, 512, 512, tag="train") as stager:
        for epoch in range(start, epochs):
            loss, acc = train(stager, model, criterion, optimizer, nbatches, iiter=epoch)

The meters are the reference's -- the average over the epoch of per-batch values, a batch's accuracies as
``metrics.accuracy`` defines them -- but the loop does not stop the host at every step as ``loss.data.item()`` and
``accuracy()`` do there (:353-355): each batch's loss and C x C confusion matrix go into a row of device buffers allocated
once per epoch, and the rows are read back at every ``print_freq``-th batch and at the end.  No TensorBoard writer.

``track_shower=True`` keeps one more meter, the fifth figure of the LArCV1 drivers' ``accuracy()``
(training/train_ubresnet2018_wlarcv1.py:584: classes 1 and 2 together), appends it to the log lines and to what is returned:
``train`` -> (loss, acc[1], track/shower), ``validate`` -> (total, track/shower).

With a guarded optimizer (``FlatAdam(..., max_grad_norm=..., skip_nonfinite=True)``: ``optimizer.guard`` is set) ``train`` keeps
one more device row per batch -- the gradient norm and whether the step was applied, copied from ``optimizer.guard.row()`` on
the stream -- drains it with the others, and its log lines gain ``GradNorm %.3e (%.3e)  Skipped %d`` (last norm, average of the
finite norms, steps skipped so far this epoch).  What it returns does not change.  The step comes after ``reducer.finish()``, so
under data parallelism every rank takes the norm of the same reduced bytes and decides alike.

With ``ema=ParamEMA(optimizer, ...)`` (ubresnet_amd/ema.py) ``train`` calls ``ema.update()`` right after ``optimizer.step()`` and its
log lines gain ``EMA %d/%d`` (updates applied / withheld so far), read where the other rows are drained, never per step;
``validate`` runs its whole loop inside ``ema.applied()``: the model is evaluated with the averaged weights and has its own back
afterwards.  With ``ema=None`` (the default) both loops are what they were.

With ``accumulate=K`` (K > 1) ``train`` takes one optimizer step per K batches: a ``GradAccumulator(model, every=K)``
(ubresnet_amd/accum.py) sums the micro-batches' flat gradients on the device and leaves their mean in the flat gradient buffer of
the K-th, where the optimizer reads it; ``optimizer.step()``, ``ema.update()`` and the guard row happen on that batch only, and
the ``zero_grad()`` before every backward keeps each one a plain, replayed pass.  ``nbatches`` must be a multiple of K.  Loss and
confusion rows, hence the meters and what is returned, stay per batch; ``GradNorm`` / ``Skipped`` count optimizer steps.  With
``accumulate=1`` (the default) the loop is what it was.

With ``stats_guard=StatsGuard(model, optimizer=optimizer)`` (ubresnet_amd/bnguard.py) ``train`` calls ``stats_guard.resolve()``
right after ``optimizer.step()`` and before ``ema.update()`` -- the average then sees the restored statistics -- on the batches
that take an optimizer step only: with ``accumulate=K`` a bad micro-batch rolls the BatchNorm running statistics back over the
whole cycle of K.  It keeps one more device row per step, copied from ``stats_guard.row()`` on the stream and drained with the
others, and the log lines gain ``BNRestored %d`` (restores so far this epoch).  With ``stats_guard=None`` (the default) the loop is
what it was.  ``validate`` does not take it: eval mode writes no statistics.
"""
from __future__ import annotations

import contextlib
import math
import time

import torch

from ubresnet_amd import metrics, ops

__all__ = ["AverageMeter", "train", "validate"]


class AverageMeter(object):
    """Computes and stores the average and current value"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


class _EpochRecord(object):
    """per-batch loss and confusion matrix in device rows; drain() moves the rows not yet read into the meters, in order"""

    def __init__(self, nbatches, nclasses, track_shower=False):
        self.nbatches, self.nclasses = int(nbatches), int(nclasses)
        self.track_shower = AverageMeter() if track_shower else None            # the fifth meter, apart from acc_list
        self.loss = self.cm = self.guard = None
        self.guard_rows = []                                                    # the rows of self.guard that were written, ascending
        self.read = 0
        self.gradnorm, self.skipped = AverageMeter(), 0                         # guarded optimizers only
        self.ema, self.ema_counts = None, (0, 0)                                # train(..., ema=...) only
        self.stats, self.stats_rows, self.bn_restored = None, [], 0             # train(..., stats_guard=...) only
        self.losses = AverageMeter()
        self.acc_list = [AverageMeter() for _ in range(self.nclasses + 1)]      # last accuracy is for total

    def put(self, i, loss, pred, label):
        C = pred.shape[1]
        if C != self.nclasses:
            raise ValueError("epoch: the model scores %d classes, nclasses=%d" % (C, self.nclasses))
        if self.loss is None:
            self.loss = torch.empty(self.nbatches, dtype=torch.float32, device=pred.device)
            self.cm = torch.empty((self.nbatches, C * C), dtype=torch.int64, device=pred.device)
            ops.zero_(self.cm)
        pred, label = pred.detach(), label.detach()
        if pred.dtype != torch.float32 or label.dtype != torch.int64:
            raise RuntimeError("epoch: expected float32 scores and int64 labels")
        self.loss[i:i + 1].copy_(loss.detach().reshape(1))
        ops.confusion(pred.contiguous(), label.contiguous(), self.cm[i])

    def put_guard(self, i, guard):
        """row i <- (norm, scale, apply) of the guarded step just issued; a device-to-device copy on the stream"""
        if self.guard is None:
            self.guard = torch.zeros((self.nbatches, 3), dtype=torch.float32, device=guard.ctl.device)
        self.guard[i].copy_(guard.row())
        self.guard_rows.append(i)

    def put_stats(self, i, stats_guard):
        """row i <- (keep, bad_rows) of the decision just issued; a device-to-device copy on the stream"""
        if self.stats is None:
            self.stats = torch.zeros((self.nbatches, 2), dtype=torch.int32, device=stats_guard.ctl.device)
        self.stats[i].copy_(stats_guard.row())
        self.stats_rows.append(i)

    def tail(self):
        """what track_shower and a guarded optimizer add to a log line"""
        ts = self.track_shower
        s = "" if ts is None else "\tAcc[trk/shr] %.3f (%.3f)" % (ts.val, ts.avg)
        if self.guard is not None:
            s += "\tGradNorm %.3e (%.3e)  Skipped %d" % (self.gradnorm.val, self.gradnorm.avg, self.skipped)
        if self.ema is not None:
            s += "\tEMA %d/%d" % self.ema_counts
        if self.stats is not None:
            s += "\tBNRestored %d" % self.bn_restored
        return s

    def drain(self, upto):
        if self.loss is None or upto <= self.read:
            return
        C = self.nclasses
        loss = self.loss[self.read:upto].cpu()                                   # the host waits here, and only here
        cm = self.cm[self.read:upto].cpu()
        if self.guard is not None:
            rows = self.guard[self.read:upto].cpu().tolist()
            # (with train(..., accumulate=K) only every K-th row is written: a row without a step is not a skipped step)
            for norm, _, applied in (rows[j - self.read] for j in self.guard_rows if self.read <= j < upto):
                if math.isfinite(norm):
                    self.gradnorm.update(norm)
                else:
                    self.gradnorm.val = norm                                     # shown as the last value, kept out of the average
                self.skipped += int(applied == 0.0)
        if self.ema is not None:
            self.ema_counts = self.ema.counts()
        if self.stats is not None:
            rows = self.stats[self.read:upto].cpu().tolist()
            self.bn_restored += sum(int(rows[j - self.read][0] == 0) for j in self.stats_rows if self.read <= j < upto)
        for j in range(upto - self.read):
            acc_values = metrics.accuracy_from_confusion(cm[j].view(C, C), track_shower=self.track_shower is not None)
            self.losses.update(loss[j].item())
            for iacc, acc in enumerate(self.acc_list):
                acc.update(acc_values[iacc])
            if self.track_shower is not None:
                self.track_shower.update(acc_values[C + 1])
        self.read = upto


def _flush(criterion):
    flush = getattr(criterion, "flush", None)
    if flush is not None:
        flush()             # PixelWiseNLLLoss reports a bad label one call late: raise for the last batches too


def train(stager, model, criterion, optimizer, nbatches, iiter=0, nclasses=3, print_freq=10, reducer=None, log=print,
          track_shower=False, accumulate=1, stats_guard=None, ema=None):
    """one epoch of `nbatches` train steps fed by `stager.next()`; -> (losses.avg, acc_list[1].avg) as the reference (:396),
    with `track_shower` -> (losses.avg, acc_list[1].avg, track/shower avg); `ema`: a ParamEMA updated after every step;
    `accumulate`: batches per optimizer step (their gradients are averaged on the device; `nbatches` must be a multiple);
    `stats_guard`: a StatsGuard resolved after every optimizer step, before the `ema` update"""
    if int(accumulate) != accumulate or int(accumulate) < 1:
        raise ValueError("accumulate must be an integer >= 1, got %r" % (accumulate,))
    accumulate = int(accumulate)
    if nbatches % accumulate != 0:
        raise ValueError("nbatches=%d is not a multiple of accumulate=%d: the last optimizer step would be left open" % (nbatches, accumulate))
    acc = None
    if accumulate > 1:
        from ubresnet_amd.accum import GradAccumulator
        acc = GradAccumulator(model, every=accumulate)
    batch_time, data_time = AverageMeter(), AverageMeter()
    rec = _EpochRecord(nbatches, nclasses, track_shower)
    rec.ema = ema

    # switch to train mode
    model.train()

    for i in range(0, nbatches):
        batchstart = time.time()
        adc_t, label_t, weight_t = stager.next()
        data_time.update(time.time() - batchstart)

        # compute output
        pred_t = model.forward(adc_t)
        loss = criterion.forward(pred_t, label_t, weight_t)

        # compute gradient and do the optimizer step
        optimizer.zero_grad()
        loss.backward()
        if reducer is not None:
            reducer.finish()
        stepped = acc is None or acc.add()                    # accumulate=K: True on every K-th batch, the mean is in place
        if stepped:
            optimizer.step()
            if stats_guard is not None:
                stats_guard.resolve()
            if ema is not None:
                ema.update()

        rec.put(i, loss, pred_t, label_t)
        if stepped and getattr(optimizer, "guard", None) is not None:
            rec.put_guard(i, optimizer.guard)
        if stepped and stats_guard is not None:
            rec.put_stats(i, stats_guard)
        batch_time.update(time.time() - batchstart)           # host time: the device runs behind it between two read-backs

        if i % print_freq == 0:
            rec.drain(i + 1)
            log("Train Iter: [%d][%d/%d]  Batch %.3f (%.3f)  Data %.3f (%.3f)\t || \tLoss %.3f (%.3f)\tAcc[total] %.3f (%.3f)" % (
                iiter, i, nbatches, batch_time.val, batch_time.avg, data_time.val, data_time.avg,
                rec.losses.val, rec.losses.avg, rec.acc_list[-1].val, rec.acc_list[1].avg) + rec.tail())

    rec.drain(nbatches)
    _flush(criterion)
    log("Train Iter [%d] Ave: Batch %.3f  Data %.3f ||  Loss %.3f Acc[Total] %.3f" % (
        iiter, batch_time.avg, data_time.avg, rec.losses.avg, rec.acc_list[-1].avg) + rec.tail())
    if track_shower:
        return rec.losses.avg, rec.acc_list[1].avg, rec.track_shower.avg
    return rec.losses.avg, rec.acc_list[1].avg


def validate(stager, model, criterion, nbatches, iiter=0, nclasses=3, print_freq=10, log=print, track_shower=False,
             calibration=None, ema=None):
    """`nbatches` batches of `stager.next()` through the model in eval mode, without gradients (the folded inference schedule);
    -> float(acc_list[-1].avg), the average total accuracy in percent (:471), with `track_shower` -> (that, track/shower avg);
    `ema`: a ParamEMA whose averaged weights the model computes with for the length of the loop;
    `calibration`: a calibration.TemperatureFit that takes every batch's (pred, label, adc) -- one launch pair per batch on the
    current stream, nothing read back; the caller reads it after the loop.  The return value and the log lines do not change"""
    batch_time, load_data = AverageMeter(), AverageMeter()
    rec = _EpochRecord(nbatches, nclasses, track_shower)

    # switch to evaluate mode
    model.eval()

    with torch.no_grad(), (ema.applied() if ema is not None else contextlib.nullcontext()):
        for i in range(0, nbatches):
            batchstart = time.time()
            adc_t, label_t, weight_t = stager.next()
            load_data.update(time.time() - batchstart)

            # compute output
            pred_t = model.forward(adc_t)
            loss_t = criterion.forward(pred_t, label_t, weight_t)
            if calibration is not None:
                calibration.add(pred_t, label_t, adc_t)

            rec.put(i, loss_t, pred_t, label_t)
            batch_time.update(time.time() - batchstart)

            if i % print_freq == 0:
                rec.drain(i + 1)
                log("Valid: [%d/%d]\tTime %.3f (%.3f)\tLoss %.3f (%.3f)\tAcc[Total] %.3f (%.3f)" % (
                    i, nbatches, batch_time.val, batch_time.avg, rec.losses.val, rec.losses.avg,
                    rec.acc_list[-1].val, rec.acc_list[-1].avg) + rec.tail())

    rec.drain(nbatches)
    _flush(criterion)
    log("Valid Iter %d sum: Batch %.3f\tData %.3f || Loss %.3f\tAcc[Total] %.3f" % (
        iiter, batch_time.avg, load_data.avg, rec.losses.avg, rec.acc_list[-1].avg))
    log("Test:Result* Acc[Total] %.3f\tLoss %.3f" % (rec.acc_list[-1].avg, rec.losses.avg) + rec.tail())
    if track_shower:
        return float(rec.acc_list[-1].avg), float(rec.track_shower.avg)
    return float(rec.acc_list[-1].avg)
