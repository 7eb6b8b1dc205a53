"""Threaded staging of loader batches: producer threads fill pinned slots, the device prepares the batch.

The reference's loader runs two filler threads over two batch buffers (training/ubresnet_train.cfg:1-29,
training/larcv1_interface.py:36-66) and ``prep_data`` (training/train_ubresnet2018_wlarcv2.py:576-615) then converts the
labels on the host, inside the step.  ``BatchStager`` keeps the host's share of a batch to one loader call and one memcpy
per array, both off the training thread:

    loader = SyntheticLArCVDataset(512, 512, tag="train"); loader.start(16)
    with BatchStager(loader, 16, 512, 512, tag="train") as stager:
        adc, label, weight = stager.next()          # [B,P,H,W] float32, [B,H,W] int64, [B,H,W] float32 on the device

* ``threads`` producers each take a free slot, then -- under one lock, because a loader is not thread-safe and batch order
  must not depend on timing -- call ``loader[0]`` and take the batch's sequence number.  Outside the lock they copy the flat
  float32 arrays as they are into the slot, ``[image | label wire | weight]`` in one packed (pinned) buffer.  Nothing is
  converted on the host.
* The thread that calls ``next()`` makes every GPU call: for the batch after the one it returns it issues, on a copy stream,
  ONE host-to-device copy of the packed slot, ``ubd_prep_batch`` (libubresnet_data.so: float labels -> int64, the optional
  ADC threshold, all-ones weights when the wire carries none) and an event.  A producer waits for that event before it
  refills the slot; that is the only GPU call a producer makes.
* Batches arrive in sequence order.  The returned tensors are fresh device memory per batch (``adc`` and ``weight`` are views
  of the packed device copy) and stay valid for as long as the caller holds them.
* No wait is unbounded: ``next()`` raises ``RuntimeError("Batch Loader timed out")`` (the reference's wording,
  larcv1_interface.py) after ``timeout`` seconds; an exception in a producer is re-raised by the ``next()`` whose batch it
  hit; ``close()`` stops and joins the (daemon) threads.

``augment=Augment(...)`` (ubresnet_amd/augment.py) pads, flips and crops every image of a training batch on the device, with
its label and weight: behind the same one copy the consumer launches ``uba_augment_batch`` (libubresnet_aug.so) INSTEAD of
``ubd_prep_batch`` -- it does the label conversion and the threshold as well -- with ``augment.params(seq, B)``, `seq` the
batch's sequence number.  Still one copy, one launch and one event per batch; the three tensors are fresh allocations and the
packed device copy is dropped behind the launch (it was allocated and used on the copy stream only).  What a batch looks like
depends on ``(augment.seed, seq)`` alone, so neither thread timing nor ``skip(n)`` changes it.  A validation stager takes no
``augment``.

``weights=PixelWeights(...)`` (ubresnet_amd/pixel_weights.py) makes the weight image on the device from the labels the network
will see (converted, thresholded, cropped and flipped, the pad label included): behind ``ubd_prep_batch`` or
``uba_augment_batch`` and before the event the consumer launches ``ubw_pixel_weights`` (libubresnet_weight.so) on the copy
stream.  ``weights.when == "missing"`` does so only for a batch whose wire has no ``weight_<tag>`` entry (one that gets all ones
without it), ``"always"`` for every batch; a wire weight that is replaced is not copied to the device.  ``stager.counts`` is
then the ``[B,16]`` int64 device tensor of per-image class counts of the batch ``next()`` returned last (None where its weights
came off the wire).  ``weights=None`` changes nothing.

``detector=DetectorEffects(...)`` (ubresnet_amd/detector.py) puts dead wires, a gain per plane and noise into the prepared
batch, in place: the producer that fills a slot also writes ``detector.table(seq, B, P, W)`` into a small pinned array of the
slot; the consumer copies it to the slot's device table (one more small non-blocking copy on the copy stream, no allocation) and launches ``ubx_apply``
(libubresnet_det.so) behind ``ubd_prep_batch`` / ``uba_augment_batch`` and BEFORE ``ubw_pixel_weights``, so that the weights
balance the labels as they finally are.  Table and noise depend on ``(detector.seed, seq)`` alone.  ``detector=None`` changes
nothing.

``device=None`` runs the host half alone (``pin=False`` then needs no GPU at all): ``next()`` returns a ``HostBatch`` of numpy
views of the slot, which stay valid until the following ``next()``, ``skip()`` or ``close()`` releases the slot.  Nothing is
augmented there: ``stager.augment.params(batch.seq, B)`` gives the caller the batch's parameters.
"""
from __future__ import annotations

import collections
import threading
import time

import numpy as np

__all__ = ["BatchStager", "HostBatch"]

HostBatch = collections.namedtuple("HostBatch", ["seq", "image", "label_wire", "weight"])


class _Slot(object):
    __slots__ = ("index", "tensor", "array", "event", "has_weight", "table_tensor", "table", "table_dev")

    def __init__(self, index, nfloats, pin, ntable=0):
        self.index = index
        self.tensor = None
        if pin:
            import torch
            self.tensor = torch.empty(nfloats, dtype=torch.float32).pin_memory()
            self.array = self.tensor.numpy()
        else:
            self.array = np.empty(nfloats, dtype=np.float32)
        self.table_tensor = self.table = None          # the detector's table of the batch in this slot (int32 / its uint32 view)
        self.table_dev = None                          # its device copy: written and read on the copy stream only
        if ntable:
            import torch
            self.table_tensor = torch.empty(ntable, dtype=torch.int32)
            if pin:
                self.table_tensor = self.table_tensor.pin_memory()
            self.table = self.table_tensor.numpy().view(np.uint32)
        self.event = None              # recorded behind the last host-to-device copy that read this slot
        self.has_weight = True


class BatchStager(object):
    def __init__(self, loader, batchsize, height, width, planes=1, tag="train", device="cuda", threads=2, slots=None,
                 label_offset=0, adc_threshold=None, timeout=60.0, pin=True, augment=None, weights=None, detector=None):
        if threads < 1:
            raise ValueError("BatchStager: threads must be >= 1")
        self.loader, self.tag = loader, tag
        self.shape = (int(batchsize), int(planes), int(height), int(width))
        b, p, h, w = self.shape
        self.npix = b * h * w
        self.label_offset = int(label_offset)
        self.adc_threshold = None if adc_threshold is None else float(adc_threshold)
        self.timeout = float(timeout)
        self.augment = augment
        self.weights = weights
        self.detector = detector
        self.counts = None
        if detector is not None and device is None:
            raise ValueError("BatchStager: detector effects are made on the device; device=None (the host half alone) takes none")
        if weights is not None and device is None:
            raise ValueError("BatchStager: weights are made on the device; device=None (the host half alone) takes none")
        nslots = int(slots) if slots is not None else int(threads) + 1
        if nslots < 1:
            raise ValueError("BatchStager: slots must be >= 1")
        self.device = None
        if device is not None:
            import torch
            from . import _data
            self._torch, self._data = torch, _data
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise RuntimeError("BatchStager: the device stage needs a ROCm device (got %s); device=None runs the host half alone" % (self.device,))
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            _data.lib()                                    # a missing library is an error now, not at the first batch
            if augment is not None:
                from . import _aug
                self._aug = _aug
                _aug.lib()
                if b > _aug.MAX_BATCH:
                    raise ValueError("BatchStager: augment takes at most %d images per batch (got %d)" % (_aug.MAX_BATCH, b))
            if weights is not None:
                from . import _weight
                self._weight = _weight
                _weight.lib()
            if detector is not None:
                from . import _det
                _det.lib()
            self.stream = torch.cuda.Stream(device=self.device)
        ntable = b * p * detector.row_words(w) if detector is not None else 0
        self._slots = [_Slot(i, (p + 2) * self.npix, pin, ntable) for i in range(nslots)]
        if ntable:
            for slot in self._slots:
                slot.table_dev = self._torch.empty(ntable, dtype=self._torch.int32, device=self.device)
        self._free = collections.deque(self._slots)
        self._ready = {}                                   # sequence number -> filled slot, or the exception that batch hit
        self._cond = threading.Condition()                 # guards _free, _ready, _stop, the stage times
        self._loader_lock = threading.Lock()               # guards the loader and _seq
        self._seq = 0                                      # next sequence number a producer takes
        self._want = 0                                     # next sequence number the consumer takes
        self._stop = False                                 # close(): every producer ends where it stands
        self._halt = False                                 # a batch failed: no producer begins another one
        self._closed = False
        self._held = None                                  # host mode: the slot whose views the caller holds
        self._inflight = None                              # device mode: (tensors, event, counts) of the staged batch, or an exception
        self._times = {"loader": [0.0, 0], "fill": [0.0, 0], "wait_slot": [0.0, 0]}
        self._nthreads = int(threads)
        self._threads = []

    # ---- producers -------------------------------------------------------------------------------------------------------
    def _start(self):
        if not self._threads:
            for i in range(self._nthreads):
                t = threading.Thread(target=self._produce, name="BatchStager-%d" % i, daemon=True)
                self._threads.append(t)
                t.start()

    def _note(self, what, dt):
        with self._cond:
            acc = self._times[what]
            acc[0] += dt
            acc[1] += 1

    def _produce(self):
        while True:
            t0 = time.perf_counter()
            with self._cond:
                while not self._free and not (self._stop or self._halt):
                    self._cond.wait(0.1)
                if self._stop or self._halt:
                    return
                slot = self._free.popleft()
            self._note("wait_slot", time.perf_counter() - t0)
            seq = None
            try:
                with self._loader_lock:
                    if self._stop or self._halt:
                        return
                    seq = self._seq
                    self._seq += 1
                    t0 = time.perf_counter()
                    try:
                        data = self.loader[0]
                    except BaseException:
                        self._halt = True                  # still under the lock: no producer calls the loader after this
                        raise
                    self._note("loader", time.perf_counter() - t0)
                t0 = time.perf_counter()
                if not self._wait_copied(slot):
                    return
                self._fill(slot, data)
                if slot.table is not None:
                    slot.table[:] = self.detector.table(seq, *self.shape[:2], self.shape[3]).reshape(-1)
                self._note("fill", time.perf_counter() - t0)
                result = slot
            except BaseException as e:                     # delivered to the next() that asks for this batch
                if seq is None:
                    return
                result = e
            with self._cond:
                self._ready[seq] = result
                if not isinstance(result, _Slot):
                    self._halt = True                      # batches already under way are still delivered, no new one is begun
                self._cond.notify_all()
            if not isinstance(result, _Slot):
                return

    def _wait_copied(self, slot):
        """the host-to-device copy that last read this slot is done (the one GPU call of a producer); False: stopped"""
        ev, slot.event = slot.event, None
        if ev is None:
            return True
        deadline = time.monotonic() + self.timeout
        while not ev.query():
            if self._stop:
                return False
            if time.monotonic() > deadline:
                raise RuntimeError("Batch Loader timed out")
            time.sleep(0.0002)
        return True

    def _fill(self, slot, data):
        b, p, h, w = self.shape
        n = self.npix
        parts = [("source_%s" % self.tag, 0, p * n), ("label_%s" % self.tag, p * n, n)]
        key = "weight_%s" % self.tag
        slot.has_weight = key in data
        if slot.has_weight:
            parts.append((key, (p + 1) * n, n))
        for name, lo, cnt in parts:
            a = data[name]
            if a.dtype != np.float32 or a.size != cnt:
                raise ValueError("BatchStager: %s is %s[%d], expected float32[%d]" % (name, a.dtype, a.size, cnt))
            np.copyto(slot.array[lo:lo + cnt], a.reshape(-1))

    # ---- consumer --------------------------------------------------------------------------------------------------------
    def _take(self):
        """-> the filled slot of the next batch in sequence order; raises what that batch hit, or the timeout"""
        if self._closed:
            raise RuntimeError("BatchStager is closed")
        self._start()
        seq = self._want
        deadline = time.monotonic() + self.timeout
        with self._cond:
            while seq not in self._ready:
                left = deadline - time.monotonic()
                if left <= 0:
                    break
                self._cond.wait(min(left, 0.1))
            got = self._ready.pop(seq, None)
        if got is None:
            self.close()
            raise RuntimeError("Batch Loader timed out")
        if not isinstance(got, _Slot):
            self.close()
            raise got
        self._want = seq + 1
        return got

    def _release(self, slot):
        with self._cond:
            self._free.append(slot)
            self._cond.notify_all()

    def _issue(self):
        """stage the next batch in sequence order on the copy stream; an exception becomes the staged batch"""
        torch = self._torch
        b, p, h, w = self.shape
        n = self.npix
        try:
            slot = self._take()
        except BaseException as e:
            self._inflight = e
            return
        if self.augment is not None:
            self._issue_augmented(slot, self._want - 1)
            return
        with torch.cuda.stream(self.stream):
            packed = torch.empty((p + 2) * n, dtype=torch.float32, device=self.device)
            label = torch.empty((b, h, w), dtype=torch.int64, device=self.device)
            make = self._makes_weights(slot)
            m = (p + 2) * n if slot.has_weight and not make else (p + 1) * n
            packed[:m].copy_(slot.tensor[:m] if slot.tensor is not None else torch.from_numpy(slot.array[:m]),
                             non_blocking=slot.tensor is not None)
            base = packed.data_ptr()
            self._data.prep_batch(base + 4 * p * n, label.data_ptr(), n, self.label_offset, image=base, planes=p, hw=h * w,
                                  threshold=self.adc_threshold,
                                  weight_fill=None if slot.has_weight or make else base + 4 * (p + 1) * n,
                                  stream=self.stream.cuda_stream)
            if self.detector is not None:
                self._launch_detector(slot, self._want - 1, base, label.data_ptr(), base + 4 * (p + 1) * n)
            counts = self._launch_weights(label, base + 4 * (p + 1) * n) if make else None
            ev = torch.cuda.Event()
            ev.record(self.stream)
        slot.event = ev
        self._release(slot)
        self._inflight = ((packed[:p * n].view(b, p, h, w), label, packed[(p + 1) * n:].view(b, h, w)), ev, counts)

    def _issue_augmented(self, slot, seq):
        """_issue with an Augment: the same copy, then uba_augment_batch out of the packed copy into three fresh tensors"""
        torch = self._torch
        b, p, h, w = self.shape
        n = self.npix
        aug = self.augment
        with torch.cuda.stream(self.stream):
            packed = torch.empty((p + 2) * n, dtype=torch.float32, device=self.device)
            adc = torch.empty((b, p, h, w), dtype=torch.float32, device=self.device)
            label = torch.empty((b, h, w), dtype=torch.int64, device=self.device)
            weight = torch.empty((b, h, w), dtype=torch.float32, device=self.device)
            make = self._makes_weights(slot)
            m = (p + 2) * n if slot.has_weight and not make else (p + 1) * n
            packed[:m].copy_(slot.tensor[:m] if slot.tensor is not None else torch.from_numpy(slot.array[:m]),
                             non_blocking=slot.tensor is not None)
            base = packed.data_ptr()
            self._aug.augment_batch(base, base + 4 * p * n, base + 4 * (p + 1) * n if slot.has_weight and not make else None,
                                    adc.data_ptr(), label.data_ptr(), weight.data_ptr(), self.shape, aug.pad,
                                    aug.params(seq, b), label_offset=self.label_offset, threshold=self.adc_threshold,
                                    pad_label=aug.pad_label, pad_weight=aug.pad_weight, stream=self.stream.cuda_stream)
            if self.detector is not None:
                self._launch_detector(slot, seq, adc.data_ptr(), label.data_ptr(), weight.data_ptr())
            counts = self._launch_weights(label, weight.data_ptr()) if make else None
            ev = torch.cuda.Event()
            ev.record(self.stream)
        del packed                                          # allocated and used on the copy stream only: its reuse is ordered
        slot.event = ev
        self._release(slot)
        self._inflight = ((adc, label, weight), ev, counts)

    def _makes_weights(self, slot):
        return self.weights is not None and (self.weights.when == "always" or not slot.has_weight)

    def _launch_detector(self, slot, seq, image_ptr, label_ptr, weight_ptr):
        """the slot's table to its device copy and ubx_apply, both on the copy stream (the caller has made it current).  The
        device copy belongs to the slot and is written and read on the copy stream only, so the copy for the slot's next batch
        is ordered behind this launch."""
        slot.table_dev.copy_(slot.table_tensor, non_blocking=slot.table_tensor.is_pinned())
        self.detector.launch(image_ptr, label_ptr, weight_ptr, self.shape, slot.table_dev.data_ptr(), seq, stream=self.stream.cuda_stream)

    def _launch_weights(self, label, weight_ptr):
        """ubw_pixel_weights on the copy stream (the caller has made it current): `label` -> the weights at `weight_ptr`;
        -> the counts tensor"""
        counts = self._torch.empty((self.shape[0], self._weight.MAX_CLASSES), dtype=self._torch.int64, device=self.device)
        self.weights.launch(label.data_ptr(), weight_ptr, counts.data_ptr(), tuple(label.shape), self.stream.cuda_stream)
        return counts

    def _staged(self):
        """take the staged batch; what it hit while it was staged is raised by the call it belongs to"""
        staged, self._inflight = self._inflight, None
        if isinstance(staged, BaseException):
            self.close()
            raise staged
        return staged

    def next(self):
        if isinstance(self._inflight, BaseException):
            self._staged()
        if self._closed:
            raise RuntimeError("BatchStager is closed")
        if self.device is None:
            if self._held is not None:
                self._release(self._held)
                self._held = None
            seq = self._want
            slot = self._held = self._take()
            b, p, h, w = self.shape
            n = self.npix
            a = slot.array
            return HostBatch(seq, a[:p * n].reshape(b, p, h, w), a[p * n:(p + 1) * n].reshape(b, h, w),
                             a[(p + 1) * n:].reshape(b, h, w) if slot.has_weight else None)
        if self._inflight is None:
            self._issue()
        dev, ev, counts = self._staged()
        cur = self._torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        for t in dev:
            t.record_stream(cur)
        if counts is not None:
            counts.record_stream(cur)
        self.counts = counts
        self._issue()
        return dev

    def skip(self, nbatches):
        """advance the loader by `nbatches` batches without staging them on the device (resume from a checkpoint)"""
        nbatches = int(nbatches)
        if self._closed:
            raise RuntimeError("BatchStager is closed")
        if nbatches > 0 and self._inflight is not None:     # the staged batch is the first one skipped
            self._staged()
            nbatches -= 1
        if not self._threads:                               # nothing fetched yet: the loader alone moves, no slot is filled
            with self._loader_lock:
                for _ in range(nbatches):
                    self.loader[0]
                    self._seq += 1
                self._want = self._seq
            return
        if self._held is not None:
            self._release(self._held)
            self._held = None
        for _ in range(nbatches):
            self._release(self._take())

    def stage_times(self):
        """mean host milliseconds per batch of the producers' stages: {"loader", "fill", "wait_slot"} -> (mean ms, count)"""
        with self._cond:
            return {k: (1e3 * s / c if c else 0.0, c) for k, (s, c) in self._times.items()}

    def close(self):
        """stop and join the producers; idempotent.  A producer stuck inside the loader is left behind (it is a daemon)."""
        self._closed = True
        with self._cond:
            self._stop = True
            self._cond.notify_all()
        deadline = time.monotonic() + 1.0
        me = threading.current_thread()
        for t in self._threads:
            if t is not me:
                t.join(max(0.0, deadline - time.monotonic()))
        self._held = None
        self._inflight = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
