"""Training crops from whole labelled events, on the device (include/ubresnet_crop.h).

Deployment takes a whole 3 x 1008 x 3456 view; training took crops of the network's size from a loader, and cutting them out of
an event was left to the host.  ``EventCropper`` does it on the device: a summed-area table of the view's counting pixels per
cell (``ubn_occupancy``), seeded crop positions drawn against it (``ubn_choose``) and the gather of image, label and weight
straight into the training batch (``ubn_gather``) -- three calls, four launches, no host round trip.

    cropper = EventCropper(crop=(512, 512), per_event=16, min_lit=2000, tries=8, seed=base_seed + rank)
    batch = cropper(image, label, weight=None, number=event_number)     # CropBatch(adc, label, weight, table, status)
    cropper.read()                                                      # the table's rows on the host: the one synchronisation

* A pixel COUNTS iff its ADC is above ``adc_threshold`` (strict; NaN does not) and, with ``classes={...}``, its label is one of
  them.  ``min_lit`` is the number of counting pixels a crop must hold: up to ``tries`` seeded positions are drawn per crop, the
  first that holds enough is taken, otherwise the best of them.  ``min_lit=0`` takes the first draw: uniform sampling.
* Positions are multiples of the cell ``g``, the largest power of two in 4..64 that divides the crop's sides and the view's
  slack (16 for 1008 x 3456 with 512 x 512 or 512 x 832); no such cell is a ValueError.  Two crops of an event may coincide.
* ``stacked=True`` is the ASPP layout: the planes are the channels of every crop and the label is one [rows, cols] image.
  Otherwise a crop is one plane, drawn from ``planes`` (default: all).
* The table -- plane, row0, col0, lit, try, accepted, flip_rows, flip_cols per crop -- is a pure function of ``(seed, number)``
  and the view.  ``table=`` gathers a caller's own rows instead (fixed validation crops; any in-range offsets); a row that
  points outside the view gives a crop of zeros and is counted in ``status``.

``EventCropStager(events, cropper)`` has ``BatchStager``'s consumer contract (``next()`` -> fresh device ``(adc, label, weight)``; a
context manager) and is what ``training.epoch.train`` / ``validate`` take: it walks ``LabelledEvent``s on the host or the device
and issues every batch one ahead on a copy stream -- uploads, the scatter of a ``SparseEvent``, the three crop calls per event
with ``number`` the running event count, then ``detector`` and ``weights`` in ``BatchStager``'s order, and an event the compute
stream waits on.  A cropper given to a stager runs on the stager's copy stream: give it to nothing else.  The overlap with the
step needs events in PINNED host memory (or on the device): a pageable tensor, and the lists of a pageable ``SparseEvent``, are
uploaded synchronously on the thread that calls ``next()``.  The batches are the same either way.
"""
from __future__ import annotations

import itertools
from typing import NamedTuple, Optional

import torch

from . import _crop as NL
from . import _lib as L
from .sparse import SparseEvent

__all__ = ["EventCropper", "CropBatch", "LabelledEvent", "EventCropStager"]

_KINDS = {torch.uint8: NL.LABEL_U8, torch.int64: NL.LABEL_I64, torch.float32: NL.LABEL_F32}


class CropBatch(NamedTuple):
    """`adc` float32 [K,C,H,W] (C = 1, or the planes of a stacked view), `label` int64 [K,H,W], `weight` float32 [K,H,W],
    `table` int32 [K,8] and `status` int64 [1] (invalid table rows met so far), all on the device"""
    adc: torch.Tensor
    label: torch.Tensor
    weight: torch.Tensor
    table: torch.Tensor
    status: torch.Tensor


class LabelledEvent(NamedTuple):
    """one event of a training set: `image` and `label` as EventCropper takes them (dense tensors on the host or the device, or
    SparseEvents), `weight` a dense float32 tensor of label's shape or None"""
    image: object
    label: object
    weight: Optional[torch.Tensor] = None


def _int(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError("EventCropper: %s must be an int in %d..%d (got %r)" % (name, lo, hi, v))
    return v


def choose_cell(rows, cols, H, W, cell=None):
    """the cell of a rows x cols view and an H x W crop: `cell` if it is legal for them, the largest legal one for None"""
    if H > rows or W > cols:
        raise ValueError("EventCropper: a %d x %d crop does not fit a %d x %d view" % (H, W, rows, cols))
    if cell is None:
        g = NL.largest_cell(rows, cols, H, W)
        if not g:
            raise ValueError("EventCropper: no cell (a power of two in %d..%d) divides the crop %d x %d and the slack %d x %d of a "
                             "%d x %d view" % (NL.MIN_CELL, NL.MAX_CELL, H, W, rows - H, cols - W, rows, cols))
        return g
    if H % cell or W % cell or (rows - H) % cell or (cols - W) % cell:
        raise ValueError("EventCropper: cell=%d does not divide the crop %d x %d and the slack %d x %d" % (cell, H, W, rows - H, cols - W))
    return cell


class EventCropper(object):
    def __init__(self, crop=(512, 512), per_event=16, min_lit=0, tries=8, classes=None, planes=None, stacked=False, adc_threshold=10.0,
                 flip_rows=False, flip_cols=False, label_offset=0, seed=0, cell=None):
        try:
            H, W = crop
        except (TypeError, ValueError):
            raise ValueError("EventCropper: crop must be a (height, width) pair (got %r)" % (crop,))
        self.crop = (_int("crop height", H, 1, NL.MAX_PIXELS), _int("crop width", W, 1, NL.MAX_PIXELS))
        self.per_event = _int("per_event", per_event, 1, NL.MAX_CROPS)
        self.min_lit = _int("min_lit", min_lit, 0, NL.MAX_PIXELS)
        self.tries = _int("tries", tries, 1, NL.MAX_TRIES)
        self.stacked = bool(stacked)
        self.class_mask = None
        if classes is not None:
            classes = sorted(set(classes))
            if not classes:
                raise ValueError("EventCropper: classes must name at least one class (None: every label counts)")
            self.class_mask = 0
            for c in classes:
                self.class_mask |= 1 << _int("a class", c, 0, 31)
        self.classes = classes
        if planes is not None:
            planes = list(planes)
            if self.stacked:
                raise ValueError("EventCropper: a stacked view has one count plane; planes must be None")
            if not planes or len(set(planes)) != len(planes):
                raise ValueError("EventCropper: planes must be a non-empty list of distinct planes (got %r)" % (planes,))
            for p in planes:
                _int("a plane", p, 0, NL.MAX_PLANES - 1)
        self.planes = planes
        self.adc_threshold = float(adc_threshold)
        self.flip_rows, self.flip_cols = bool(flip_rows), bool(flip_cols)
        self.label_offset = _int("label_offset", label_offset, -2 ** 31, 2 ** 31 - 1)
        self.seed = _int("seed", seed, 0, 2 ** 64 - 1)
        if cell is not None and (isinstance(cell, bool) or not isinstance(cell, int) or cell not in (4, 8, 16, 32, 64)):
            raise ValueError("EventCropper: cell must be None or a power of two in %d..%d (got %r)" % (NL.MIN_CELL, NL.MAX_CELL, cell))
        self.cell = cell
        self.sat = None                  # the device table of sums of the last call that drew its own crops
        self.table = None                # the device crop table of the last call
        self.status = None               # int64 [1] on the device: invalid table rows (and refused sparse entries) so far
        self._views = {}                 # what: the dense buffer a SparseEvent is scattered into

    # ---- arguments -------------------------------------------------------------------------------------------------------
    def geometry(self, planes, rows, cols):
        """(count planes Q, cell g) for a view; the errors of a view this cropper cannot take"""
        H, W = self.crop
        if planes < 1 or planes > NL.MAX_PLANES or planes * rows * cols > NL.MAX_PIXELS:
            raise ValueError("EventCropper: a view of %d x %d x %d is not 1..%d planes below 2^31 pixels" % (planes, rows, cols, NL.MAX_PLANES))
        g = choose_cell(rows, cols, H, W, self.cell)
        if cols // g > NL.MAX_CELL_COLS:
            raise ValueError("EventCropper: %d cells per row are more than %d" % (cols // g, NL.MAX_CELL_COLS))
        if self.planes is not None and max(self.planes) >= planes:
            raise ValueError("EventCropper: planes=%r names a plane the view of %d does not have" % (self.planes, planes))
        return (1 if self.stacked else planes), g

    @staticmethod
    def _dense(t, what, dtypes):
        if not isinstance(t, torch.Tensor):
            raise TypeError("EventCropper: %s must be a torch tensor or a SparseEvent (got %s)" % (what, type(t).__name__))
        if t.dtype not in dtypes:
            raise TypeError("EventCropper: %s must be %s (got %s)" % (what, " / ".join(str(d).replace("torch.", "") for d in dtypes), t.dtype))
        if t.dim() == 4 and t.shape[1] == 1:
            t = t[:, 0]
        return t

    def _scattered(self, ev, what, device):
        key = (what, ev.planes, ev.rows, ev.cols)
        buf = self._views.get(key)
        if buf is None or buf.device != device:
            buf = self._views[key] = torch.empty((ev.planes, 1, ev.rows, ev.cols), dtype=torch.float32, device=device)
        return ev.to_view(device, out=buf, status=self.status)[:, 0]

    def _check_out(self, out, K, C, device):
        H, W = self.crop
        try:
            adc, label, weight = out
        except (TypeError, ValueError):
            raise ValueError("EventCropper: out must be an (adc, label, weight) triple")
        for t, what, dt, shape in ((adc, "adc", torch.float32, (K, C, H, W)), (label, "label", torch.int64, (K, H, W)),
                                   (weight, "weight", torch.float32, (K, H, W))):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("EventCropper: out %s must be a contiguous %s tensor of %s" % (what, str(dt).replace("torch.", ""), shape))
            L.require_cuda(t, "out " + what)
            if t.device != device:
                raise ValueError("EventCropper: out %s lives on %s, the view on %s" % (what, t.device, device))
        return adc, label, weight

    # ---- the call --------------------------------------------------------------------------------------------------------
    def __call__(self, image, label, weight=None, number=0, out=None, table=None, _table_out=None):
        """`image`: float32 [P,rows,cols] or [P,1,rows,cols] on the device, or a SparseEvent; `label`: uint8 / int64 / float32 of
        [P,rows,cols] (stacked: [rows,cols]) on the device, or a SparseEvent whose values are the labels (unlisted pixels: 0);
        `weight`: float32 of label's shape or None (all ones); `number`: the event's number, 0..2^32-1; `out`: an (adc, label,
        weight) triple to write, e.g. slices of a batch; `table`: int32 [K,8] rows to gather instead of drawing per_event crops.
        Everything is issued on the current stream of the image's device."""
        H, W = self.crop
        number = _int("number", number, 0, 2 ** 32 - 1)
        sparse_image = isinstance(image, SparseEvent)
        if sparse_image:
            P, rows, cols = image.planes, image.rows, image.cols
            device = image.index.device if image.index.is_cuda else torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        else:
            image = self._dense(image, "image", (torch.float32,))
            if image.dim() != 3:
                raise ValueError("EventCropper: image must be [planes,rows,cols] or [planes,1,rows,cols] (got %s)" % (tuple(image.shape),))
            P, rows, cols = (int(s) for s in image.shape)
            device = image.device
        Q, g = self.geometry(P, rows, cols)
        lshape = (rows, cols) if self.stacked else (P, rows, cols)
        if isinstance(label, SparseEvent):
            if (label.planes, label.rows, label.cols) != ((1,) + lshape if self.stacked else lshape):
                raise ValueError("EventCropper: the label list is for %d x %d x %d, the view wants %s" % (label.planes, label.rows, label.cols, lshape))
        else:
            label = self._dense(label, "label", (torch.uint8, torch.int64, torch.float32))
            if tuple(label.shape) != lshape:
                raise ValueError("EventCropper: label must be %s for this view%s (got %s)" % (lshape, " (stacked)" if self.stacked else "", tuple(label.shape)))
        if weight is not None:
            weight = self._dense(weight, "weight", (torch.float32,))
            if tuple(weight.shape) != lshape:
                raise ValueError("EventCropper: weight must be %s, the label's shape (got %s)" % (lshape, tuple(weight.shape)))
        if table is not None:
            if not isinstance(table, torch.Tensor) or table.dtype != torch.int32:
                raise TypeError("EventCropper: table must be an int32 tensor")
            if table.dim() != 2 or table.shape[1] != NL.TABLE_FIELDS or not 1 <= table.shape[0] <= NL.MAX_CROPS:
                raise ValueError("EventCropper: table must be [K,%d] with K in 1..%d (got %s)" % (NL.TABLE_FIELDS, NL.MAX_CROPS, tuple(table.shape)))
        K = self.per_event if table is None else int(table.shape[0])
        C = P if self.stacked else 1
        if device is None or device.type != "cuda":
            raise RuntimeError("ubresnet_amd: EventCropper needs a ROCm device (got %s); the HIP path has no CPU fallback" % (device,))
        for t, what in ((label, "label"), (weight, "weight")):
            if isinstance(t, torch.Tensor):
                L.require_cuda(t, what)
                if t.device != device:
                    raise ValueError("EventCropper: %s lives on %s, the image on %s" % (what, t.device, device))
        if out is not None:
            out = self._check_out(out, K, C, device)
        with torch.cuda.device(device):
            if self.status is None or self.status.device != device:
                self.status = torch.zeros(1, dtype=torch.int64, device=device)
            image = self._scattered(image, "image", device) if sparse_image else image.contiguous()
            label = self._scattered(label, "label", device) if isinstance(label, SparseEvent) else label.contiguous()
            if self.stacked and label.dim() == 3:
                label = label[0]
            weight = None if weight is None else weight.contiguous()
            adc, lab, wgt = out if out is not None else (torch.empty((K, C, H, W), dtype=torch.float32, device=device),
                                                         torch.empty((K, H, W), dtype=torch.int64, device=device),
                                                         torch.empty((K, H, W), dtype=torch.float32, device=device))
            kind, st = _KINDS[label.dtype], L.stream_ptr()
            if table is None:
                shape = NL.sat_shape(Q, rows, cols, g)
                if self.sat is None or tuple(self.sat.shape) != shape or self.sat.device != device:
                    self.sat = torch.empty(shape, dtype=torch.int32, device=device)
                table = _table_out if _table_out is not None else torch.empty((K, NL.TABLE_FIELDS), dtype=torch.int32, device=device)
                masked = self.class_mask is not None
                NL.occupancy(image.data_ptr(), label.data_ptr() if masked else None, kind if masked else NL.LABEL_NONE, self.label_offset,
                             self.class_mask or 0, self.stacked, self.adc_threshold, P, rows, cols, g, self.sat.data_ptr(), st)
                NL.choose(self.sat.data_ptr(), Q, rows, cols, H, W, g, self.planes, K, self.tries, self.min_lit, self.seed, number,
                          self.flip_rows, self.flip_cols, table.data_ptr(), st)
            else:
                table = table.to(device, non_blocking=True).contiguous()
                if _table_out is not None:
                    _table_out.copy_(table)
                    table = _table_out
            NL.gather(image.data_ptr(), label.data_ptr(), kind, self.label_offset, None if weight is None else weight.data_ptr(), self.stacked,
                      P, rows, cols, H, W, table.data_ptr(), K, adc.data_ptr(), lab.data_ptr(), wgt.data_ptr(), self.status.data_ptr(), st)
        self.table = table
        return CropBatch(adc, lab, wgt, table, self.status)

    def read(self):
        """the rows of the last call's table on the host, int32 [K,8]: the one synchronisation"""
        if self.table is None:
            raise RuntimeError("EventCropper.read: no call yet")
        return self.table.cpu()


class EventCropStager(object):
    def __init__(self, events, cropper, events_per_batch=1, device="cuda", weights=None, detector=None):
        if not isinstance(cropper, EventCropper):
            raise TypeError("EventCropStager: cropper must be an EventCropper")
        if isinstance(events_per_batch, bool) or not isinstance(events_per_batch, int) or events_per_batch < 1:
            raise ValueError("EventCropStager: events_per_batch must be an int >= 1 (got %r)" % (events_per_batch,))
        if events_per_batch * cropper.per_event > NL.MAX_CROPS:
            raise ValueError("EventCropStager: %d x %d crops per batch are more than %d" % (events_per_batch, cropper.per_event, NL.MAX_CROPS))
        self.cropper, self.events_per_batch = cropper, events_per_batch
        self.batchsize = events_per_batch * cropper.per_event
        self.weights, self.detector = weights, detector
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ubresnet_amd: EventCropStager needs a ROCm device (got %s); the HIP path has no CPU fallback" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        NL.lib()                                           # a missing library is an error now, not at the first batch
        if weights is not None:
            from . import _weight
            self._weight = _weight
            _weight.lib()
        if detector is not None:
            from . import _det
            _det.lib()
        self._events = itertools.cycle(events) if hasattr(events, "__len__") else iter(events)
        self.stream = torch.cuda.Stream(device=self.device)
        self.seq = 0                                       # batches issued
        self.count = 0                                     # events issued: the `number` of the next one
        self.tables = None                                 # int32 [B,8] on the device: the rows of the batch next() returned last
        self.counts = None                                 # int64 [B,16] class counts where the weights of that batch were made here
        self._inflight = None
        self._closed = False
        self._det_slots = None                             # the detector's pinned tables, made at the first batch

    def _up(self, t):
        if isinstance(t, SparseEvent) or t is None:
            return t                                        # a SparseEvent is uploaded by its own to_view
        return t.to(self.device, non_blocking=True)

    def _detector_table(self, B, C, W):
        """the detector's table of batch `seq` on the device (the copy stream is current).  Two slots, as BatchStager keeps one per
        slot: a pinned host array, its device copy and the event behind the copy.  The host array is rewritten only after the
        copy that last read it is done; the device copy is written and read on the copy stream only."""
        n = B * C * self.detector.row_words(W)
        if self._det_slots is None or self._det_slots[0][0].numel() != n:
            self._det_slots = [[torch.empty(n, dtype=torch.int32).pin_memory(), torch.empty(n, dtype=torch.int32, device=self.device), None]
                               for _ in range(2)]
        slot = self._det_slots[self.seq & 1]
        host, dev, copied = slot
        if copied is not None:
            copied.synchronize()
        host.numpy().view("uint32")[:] = self.detector.table(self.seq, B, C, W).reshape(-1)
        dev.copy_(host, non_blocking=True)
        slot[2] = torch.cuda.Event()
        slot[2].record(self.stream)
        return dev

    def _issue(self):
        """stage the next batch on the copy stream; an exception becomes the staged batch"""
        try:
            events = [next(self._events) for _ in range(self.events_per_batch)]
        except BaseException as e:
            self._inflight = e
            return
        cr, K, B = self.cropper, self.cropper.per_event, self.batchsize
        H, W = cr.crop
        try:
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                first = events[0].image
                C = (first.planes if isinstance(first, SparseEvent) else int(first.shape[0])) if cr.stacked else 1
                adc = torch.empty((B, C, H, W), dtype=torch.float32, device=self.device)
                label = torch.empty((B, H, W), dtype=torch.int64, device=self.device)
                weight = torch.empty((B, H, W), dtype=torch.float32, device=self.device)
                tables = torch.empty((B, NL.TABLE_FIELDS), dtype=torch.int32, device=self.device)
                for e, ev in enumerate(events):
                    s = slice(e * K, (e + 1) * K)
                    cr(self._up(ev.image), self._up(ev.label), self._up(ev.weight), number=(self.count + e) & 0xFFFFFFFF,
                       out=(adc[s], label[s], weight[s]), _table_out=tables[s])
                if self.detector is not None:
                    t = self._detector_table(B, C, W)
                    self.detector.launch(adc.data_ptr(), label.data_ptr(), weight.data_ptr(), (B, C, H, W), t.data_ptr(), self.seq,
                                         stream=self.stream.cuda_stream)
                counts = None
                if self.weights is not None:
                    make = [self.weights.when == "always" or ev.weight is None for ev in events]
                    if any(make):
                        counts = torch.zeros((B, self._weight.MAX_CLASSES), dtype=torch.int64, device=self.device)
                        for e, m in enumerate(make):
                            if m:
                                s = slice(e * K, (e + 1) * K)
                                self.weights.launch(label[s].data_ptr(), weight[s].data_ptr(), counts[s].data_ptr(), (K, H, W),
                                                    self.stream.cuda_stream)
                done = torch.cuda.Event()
                done.record(self.stream)
        except BaseException as e:
            self._inflight = e
            return
        self.seq += 1
        self.count += len(events)
        self._inflight = ((adc, label, weight), done, counts, tables)

    def next(self):
        if self._closed:
            raise RuntimeError("EventCropStager is closed")
        if self._inflight is None:
            self._issue()
        staged, self._inflight = self._inflight, None
        if isinstance(staged, BaseException):
            self.close()
            raise staged
        dev, done, counts, tables = staged
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(done)
        for t in dev + (tables,) + ((counts,) if counts is not None else ()):
            t.record_stream(cur)
        self.counts, self.tables = counts, tables
        self._issue()
        return dev

    def close(self):
        self._closed = True
        self._inflight = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
