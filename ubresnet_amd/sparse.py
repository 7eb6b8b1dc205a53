"""Sparse event I/O around whole-view inference: the event enters as a sorted list of (pixel index, ADC) pairs and the result
leaves as the list of its lit pixels (include/ubresnet_sparse.h).  A wire-plane event is one or two per cent lit; LArCV-style
files hold it as such a list, and the downstream chain reads the lit pixels of the result as a list as well.

  * ``SparseEvent(index, value, planes, rows, cols)``: the input list, on the host or on the device; ``to_view`` copies it to the
    device if need be and scatters it into the dense [planes,1,rows,cols] view the network's tiles are cropped from
    (ubz_scatter_view).  ``WholeViewSegmenter.__call__`` takes one in place of the dense view.
  * ``compact(products, view, ...)`` -> ``PixelList``: index, label and confidence of the lit pixels of ``deploy.Products`` in
    ascending pixel-index order, and their number, all on the device (ubz_compact: three launches, no atomics).
    ``WholeViewSegmenter(..., output="pixels")`` returns one.
  * ``PixelList.read()`` is the one host synchronisation: the count, then that many entries.  ``PixelList.to_products()``
    expands the list back into dense Products (ubz_expand).

A pixel index is the int32 offset (plane * rows + row) * cols + col.  The three kernels only move data: every result is exact.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib as L
from . import _sparse as ZL


def _check_image(planes, rows, cols):
    for name, v in (("planes", planes), ("rows", rows), ("cols", cols)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError("sparse: %s must be a positive int (got %r)" % (name, v))
    if planes * rows * cols > ZL.MAX_PIXELS:
        raise ValueError("sparse: %d x %d x %d pixels do not fit an int32 pixel index" % (planes, rows, cols))


def _status_word(device):
    return torch.zeros(1, dtype=torch.int64, device=device)


class SparseEvent:
    """One event as a list: `index` int32 [n] pixel indices in strictly ascending order, `value` float32 [n], both on the host
    (pinned or not) or both on one device, for a [planes][rows][cols] image.  Nothing is read here: validate() checks the list
    on the host, and the device counts the entries that break the rule into the status word (they are not written)."""

    def __init__(self, index: torch.Tensor, value: torch.Tensor, planes: int, rows: int, cols: int):
        _check_image(planes, rows, cols)
        if not isinstance(index, torch.Tensor) or not isinstance(value, torch.Tensor):
            raise TypeError("SparseEvent: index and value must be torch tensors")
        if index.dtype != torch.int32 or value.dtype != torch.float32:
            raise TypeError("SparseEvent: index must be int32 and value float32 (got %s, %s)" % (index.dtype, value.dtype))
        if index.dim() != 1 or value.dim() != 1 or index.shape != value.shape:
            raise ValueError("SparseEvent: index and value must be 1-D of one length (got %s, %s)" % (tuple(index.shape), tuple(value.shape)))
        if index.device != value.device:
            raise ValueError("SparseEvent: index and value must live on one device (got %s, %s)" % (index.device, value.device))
        self.index, self.value = index.contiguous(), value.contiguous()
        self.planes, self.rows, self.cols = planes, rows, cols
        self.status = None                                  # the device word of the last to_view that was given none

    @property
    def n(self) -> int:
        return self.index.numel()

    @staticmethod
    def from_dense(view: torch.Tensor, threshold: Optional[float] = None) -> "SparseEvent":
        """host helper for tests and tools: the list of a dense float32 view [planes,1,rows,cols] or [planes,rows,cols].
        threshold=None keeps every element whose bits are not those of +0.0 (so to_view gives the view back bit for bit);
        otherwise the elements > threshold."""
        if not isinstance(view, torch.Tensor) or view.dtype != torch.float32:
            raise TypeError("SparseEvent.from_dense: expected a float32 tensor")
        if view.dim() == 4 and view.shape[1] == 1:
            view = view[:, 0]
        if view.dim() != 3:
            raise ValueError("SparseEvent.from_dense: expected [planes,1,rows,cols] or [planes,rows,cols] (got %s)" % (tuple(view.shape),))
        planes, rows, cols = (int(s) for s in view.shape)
        _check_image(planes, rows, cols)
        flat = view.detach().cpu().contiguous().reshape(-1)
        keep = flat.view(torch.int32) != 0 if threshold is None else flat > float(threshold)
        index = torch.nonzero(keep).reshape(-1).to(torch.int32)
        return SparseEvent(index, flat[keep].clone(), planes, rows, cols)

    def validate(self) -> "SparseEvent":
        """on the host (a device list is copied, which synchronises): every index in range and above its predecessor"""
        idx = self.index.cpu().to(torch.int64)
        if idx.numel():
            if int(idx.min()) < 0 or int(idx.max()) >= self.planes * self.rows * self.cols:
                raise ValueError("SparseEvent: a pixel index lies outside 0..%d" % (self.planes * self.rows * self.cols - 1))
            if idx.numel() > 1 and not bool((idx[1:] > idx[:-1]).all()):
                raise ValueError("SparseEvent: the pixel indices are not strictly ascending")
        return self

    def to_view(self, device, out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the dense float32 view [planes,1,rows,cols] on `device`: a non-blocking copy of index and value if they are on the
        host, then ubz_scatter_view on the current stream.  `out` is written on every element; `status` (int64 [1] on the
        device, its bits a uint64) has the number of refused entries added -- a new zero word, kept as self.status, if None."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ubresnet_amd: SparseEvent.to_view needs a ROCm device (got %s); the HIP path has no CPU fallback" % device)
        shape = (self.planes, 1, self.rows, self.cols)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=device)
        elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous()):
            raise RuntimeError("SparseEvent.to_view: out must be a contiguous float32 %s on the device" % (shape,))
        if status is None:
            status = self.status = _status_word(out.device)
        elif not (status.is_cuda and status.dtype == torch.int64 and status.numel() == 1):
            raise RuntimeError("SparseEvent.to_view: status must be one int64 word on the device")
        index, value = self.index, self.value
        if not index.is_cuda:
            index, value = index.to(out.device, non_blocking=True), value.to(out.device, non_blocking=True)
        elif index.device != out.device:
            raise RuntimeError("SparseEvent.to_view: the list lives on %s, the view on %s" % (index.device, out.device))
        with torch.cuda.device(out.device):
            ZL.scatter_view(index.data_ptr(), value.data_ptr(), self.n, None, out.data_ptr(), self.planes, self.rows, self.cols,
                            status.data_ptr(), L.stream_ptr())
        return out


class PixelList(NamedTuple):
    """the lit pixels of event products in ascending pixel-index order, on the device: `index` int32 / `label` uint8 /
    `confidence` float16 of [capacity], of which the first min(count, capacity) are defined; `count` int64 [1], the number of lit
    pixels (above capacity: the list overflowed); `counts` the per-plane class counts of the Products."""
    index: torch.Tensor
    label: torch.Tensor
    confidence: torch.Tensor
    count: torch.Tensor
    counts: Optional[torch.Tensor]
    planes: int
    rows: int
    cols: int
    fill_label: int

    @property
    def capacity(self) -> int:
        return self.index.numel()

    def read(self):
        """the one host synchronisation: (index, label, confidence) of the lit pixels on the host -- the count is copied, then
        that many entries and no more.  OverflowError if there were more lit pixels than capacity."""
        total = int(self.count.item())
        if total > self.capacity:
            raise OverflowError("PixelList: %d lit pixels, capacity %d" % (total, self.capacity))
        return self.index[:total].cpu(), self.label[:total].cpu(), self.confidence[:total].cpu()

    def to_products(self, status: Optional[torch.Tensor] = None):
        """deploy.Products again (ubz_expand on the current stream): fill_label / +0 where no entry names the pixel.  Shapes
        [planes,rows,cols], or [rows,cols] where `counts` is that of a stacked model ([classes])."""
        from .deploy import Products
        dev = self.index.device
        label = torch.empty((self.planes, self.rows, self.cols), dtype=torch.uint8, device=dev)
        conf = torch.empty((self.planes, self.rows, self.cols), dtype=torch.float16, device=dev)
        if status is None:
            status = _status_word(dev)
        with torch.cuda.device(dev):
            ZL.expand(self.index.data_ptr(), self.label.data_ptr(), self.confidence.data_ptr(), self.capacity, self.count.data_ptr(),
                      self.fill_label, label.data_ptr(), conf.data_ptr(), self.planes, self.rows, self.cols, status.data_ptr(),
                      L.stream_ptr())
        if self.counts is not None and self.counts.dim() == 1 and self.planes == 1:
            return Products(label[0], conf[0], self.counts)
        return Products(label, conf, self.counts)


class Compactor:
    """the buffers of ubz_compact for one image size and capacity -- the three output arrays, the count and the scratch --
    allocated once; every call overwrites them (WholeViewSegmenter keeps one between its calls)"""

    def __init__(self, planes: int, rows: int, cols: int, capacity: Optional[int], device):
        _check_image(planes, rows, cols)
        if capacity is None:
            capacity = planes * rows * cols
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError("sparse: capacity must be None or an int >= 1 (got %r)" % (capacity,))
        self.planes, self.rows, self.cols, self.capacity = planes, rows, cols, capacity
        self.scratch_bytes = ZL.compact_scratch_bytes(planes, rows, cols)
        self.device = torch.device(device)
        self.index = torch.empty(capacity, dtype=torch.int32, device=self.device)
        self.label = torch.empty(capacity, dtype=torch.uint8, device=self.device)
        self.confidence = torch.empty(capacity, dtype=torch.float16, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.scratch = torch.empty(self.scratch_bytes // 4, dtype=torch.int32, device=self.device)

    def __call__(self, label, confidence, counts, view, vplanes, adc_threshold, fill_label) -> PixelList:
        use_adc = view is not None and adc_threshold is not None
        ZL.compact(label.data_ptr(), confidence.data_ptr(), view.data_ptr() if use_adc else None, vplanes,
                   float(adc_threshold) if use_adc else 0.0, self.planes, self.rows, self.cols, self.capacity, self.index.data_ptr(),
                   self.label.data_ptr(), self.confidence.data_ptr(), self.count.data_ptr(), self.scratch.data_ptr(),
                   self.scratch_bytes, L.stream_ptr())
        return PixelList(self.index, self.label, self.confidence, self.count, counts, self.planes, self.rows, self.cols, fill_label)


def compact(products, view: Optional[torch.Tensor], adc_threshold: Optional[float] = 10.0, capacity: Optional[int] = None,
            vplanes: int = 1, fill_label: int = 255) -> PixelList:
    """the lit pixels of `products` (deploy.Products: label uint8 and confidence float16 of [P,rows,cols], or [rows,cols]) as a
    PixelList, on the current stream.  `view` is the float32 ADC of the lit test, P * vplanes planes of rows x cols (a pixel is lit
    iff any of its vplanes values is > adc_threshold; NaN is not lit); view=None or adc_threshold=None: every pixel is lit.
    capacity=None: P * rows * cols entries, which cannot overflow.  `fill_label` is what to_products() gives the other pixels."""
    label, conf = products.label, products.confidence
    for t, what in ((label, "label"), (conf, "confidence")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("sparse.compact: products.%s must be a torch tensor" % what)
    if label.dtype != torch.uint8 or conf.dtype != torch.float16:
        raise TypeError("sparse.compact: label must be uint8 and confidence float16 (got %s, %s)" % (label.dtype, conf.dtype))
    if label.dim() not in (2, 3) or label.shape != conf.shape:
        raise ValueError("sparse.compact: label and confidence must both be [P,rows,cols] or [rows,cols] (got %s, %s)"
                         % (tuple(label.shape), tuple(conf.shape)))
    P, rows, cols = (1,) * (3 - label.dim()) + tuple(int(s) for s in label.shape)
    _check_image(P, rows, cols)
    if isinstance(vplanes, bool) or not isinstance(vplanes, int) or not 1 <= vplanes <= ZL.MAX_VPLANES:
        raise ValueError("sparse.compact: vplanes must be an int in 1..%d (got %r)" % (ZL.MAX_VPLANES, vplanes))
    if isinstance(fill_label, bool) or not isinstance(fill_label, int) or not 0 <= fill_label <= 255:
        raise ValueError("sparse.compact: fill_label must be an int in 0..255 (got %r)" % (fill_label,))
    if view is not None:
        if not isinstance(view, torch.Tensor) or view.dtype != torch.float32:
            raise TypeError("sparse.compact: view must be a float32 tensor or None")
        if view.numel() != P * vplanes * rows * cols or tuple(view.shape[-2:]) != (rows, cols):
            raise ValueError("sparse.compact: view %s is not %d x %d planes of %d x %d" % (tuple(view.shape), P, vplanes, rows, cols))
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1):
        raise ValueError("sparse: capacity must be None or an int >= 1 (got %r)" % (capacity,))
    L.require_cuda(label, "products.label")
    L.require_cuda(conf, "products.confidence")
    if view is not None:
        L.require_cuda(view, "view")
        view = view.contiguous()
    with torch.cuda.device(label.device):
        return Compactor(P, rows, cols, capacity, label.device)(label.contiguous(), conf.contiguous(), products.counts, view, vplanes,
                                                                adc_threshold, fill_label)
