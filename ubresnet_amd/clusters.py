"""Connected components of event products on the device (include/ubresnet_cluster.h): the lit pixels of a class map grouped into
clusters, each cluster numbered and summarised -- pixels, bounding box, summed confidence, pixels per class -- without the event
leaving the device.  The first thing a LArTPC chain does with an SSNet map is to cluster it and to ask each cluster how much of it
is track and how much is shower.

    cl = clusters.EventClusterer(planes=3, rows=1008, cols=3456, num_classes=4, connectivity=8, by_class=False,
                                 fill_label=255, capacity=65536, device="cuda:0")
    found = cl(products)                 # or cl(label, confidence), or cl(pixel_list); nothing is read back
    tab = found.read(min_pixels=1)       # the one sync: the count, then that many rows; OverflowError if count > capacity
    tab.plane, tab.pixels, tab.bbox, tab.class_counts, tab.fractions(), tab.mean_confidence()
    k = clusters.of_pixels(found, pixel_list)   # int32 cluster number per listed pixel, on the device (ubi_gather_ids)

Two lit pixels are adjacent if they lie in the same plane and touch (8-connected: also diagonally) and, with by_class, carry the
same label.  A cluster's root is its smallest pixel index, the clusters are numbered in ascending root order, and every column of
the table is an integer sum, minimum or maximum: the result is the same bits on every run.  Buffers are kept between calls; a
call overwrites the result of the one before, as a PixelList does.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _cluster as IL
from . import _lib as L


def _int(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        raise ValueError("clusters: %s must be an int %s (got %r)" % (name, ">= %d" % lo if hi is None else "in %d..%d" % (lo, hi), v))
    return v


class ClusterTable:
    """the rows of the cluster table on the host (int64 [n, 8 + C]), `total` clusters of which these passed min_pixels"""

    def __init__(self, rows: torch.Tensor, num_classes: int, image, total: int):
        self.rows, self.num_classes, self.image, self.total = rows, num_classes, tuple(image), total

    def __len__(self):
        return self.rows.shape[0]

    @property
    def root(self):
        return self.rows[:, 0]

    @property
    def plane(self):
        return self.rows[:, 0] // (self.image[1] * self.image[2])

    @property
    def pixels(self):
        return self.rows[:, 1]

    @property
    def bbox(self):
        """[n, 4]: row_min, row_max, col_min, col_max, inclusive"""
        return self.rows[:, 2:6]

    @property
    def nonfinite(self):
        return self.rows[:, 7]

    @property
    def class_counts(self):
        return self.rows[:, IL.TABLE_FIXED:]

    def fractions(self):
        """[n, C] float64: the share of every class among the cluster's pixels"""
        return self.class_counts.double() / self.pixels.double().unsqueeze(1)

    def mean_confidence(self):
        """[n] float64: the mean of the finite, non-negative confidences; NaN where the cluster has none"""
        finite = (self.pixels - self.nonfinite).double()
        return self.rows[:, 6].double() / float(1 << 24) / finite.masked_fill(finite == 0, float("nan"))


class Clusters(NamedTuple):
    """the clusters of one event, on the device: `ids` / `root` int32 like the label (-1 where the pixel is not lit), `table`
    int64 [capacity, 8 + C], `count` int64 [1] (the total, also above capacity), `status` int64 [1] (foreign labels met so far)"""
    ids: torch.Tensor
    root: torch.Tensor
    table: torch.Tensor
    count: torch.Tensor
    status: torch.Tensor

    @property
    def capacity(self) -> int:
        return self.table.shape[0]

    def read(self, min_pixels: int = 1) -> ClusterTable:
        """the one host synchronisation: the count is copied, then that many rows and no more.  OverflowError if there were more
        clusters than capacity.  Rows of fewer than min_pixels pixels are dropped on the host."""
        _int("min_pixels", min_pixels, 0)
        total = int(self.count.item())
        if total > self.capacity:
            raise OverflowError("Clusters: %d clusters, capacity %d" % (total, self.capacity))
        rows = self.table[:total].cpu()
        if min_pixels > 1:
            rows = rows[rows[:, 1] >= min_pixels]
        image = (1,) * (3 - self.ids.dim()) + tuple(int(s) for s in self.ids.shape)
        return ClusterTable(rows, self.table.shape[1] - IL.TABLE_FIXED, image, total)


class EventClusterer:
    """the buffers of ubi_label and ubi_tabulate for one image size -- root, ids, table, count, status, scratch -- allocated once;
    every call overwrites them (status is added to).  Stacked models (label [rows, cols]) count as one plane: planes=1."""

    def __init__(self, planes: int = 3, rows: int = 1008, cols: int = 3456, num_classes: int = 4, connectivity: int = 8,
                 by_class: bool = False, fill_label: int = 255, capacity: int = 65536, device="cuda:0"):
        _int("planes", planes, 1), _int("rows", rows, 1), _int("cols", cols, 1)
        if planes * rows * cols > IL.MAX_PIXELS:
            raise ValueError("clusters: %d x %d x %d pixels do not fit an int32 pixel index" % (planes, rows, cols))
        _int("num_classes", num_classes, 1, IL.MAX_CLASSES), _int("fill_label", fill_label, 0, 255), _int("capacity", capacity, 1)
        if connectivity not in (4, 8) or isinstance(connectivity, bool):
            raise ValueError("clusters: connectivity must be 4 or 8 (got %r)" % (connectivity,))
        if not isinstance(by_class, bool):
            raise ValueError("clusters: by_class must be a bool (got %r)" % (by_class,))
        self.planes, self.rows, self.cols, self.num_classes = planes, rows, cols, num_classes
        self.connectivity, self.by_class, self.fill_label, self.capacity = connectivity, by_class, fill_label, capacity
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ubresnet_amd: EventClusterer needs a ROCm device (got %s); the HIP path has no CPU fallback" % self.device)
        self.scratch_bytes = IL.scratch_bytes(planes, rows, cols)
        shape = (planes, rows, cols)
        self.root = torch.empty(shape, dtype=torch.int32, device=self.device)
        self.ids = torch.empty(shape, dtype=torch.int32, device=self.device)
        self.table = torch.zeros((capacity, IL.TABLE_FIXED + num_classes), dtype=torch.int64, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.scratch = torch.empty(self.scratch_bytes // 4, dtype=torch.int32, device=self.device)
        self.label = None                                           # the class map of the last call (shapes.ClusterMoments reads it)

    def _views(self, label, confidence):
        if confidence is None:
            if hasattr(label, "to_products"):                       # a sparse.PixelList: expanded on the device
                label = label.to_products()
            label, confidence = label.label, label.confidence
        for t, what in ((label, "label"), (confidence, "confidence")):
            if not isinstance(t, torch.Tensor):
                raise TypeError("EventClusterer: %s must be a torch tensor" % what)
        if label.dtype != torch.uint8 or confidence.dtype != torch.float16:
            raise TypeError("EventClusterer: label must be uint8 and confidence float16 (got %s, %s)" % (label.dtype, confidence.dtype))
        want = (self.planes, self.rows, self.cols)
        got = (1,) * (3 - label.dim()) + tuple(int(s) for s in label.shape) if label.dim() in (2, 3) else tuple(label.shape)
        if got != want or label.shape != confidence.shape:
            raise ValueError("EventClusterer: expected label and confidence of %s (or [rows, cols] for one plane), got %s and %s"
                             % (want, tuple(label.shape), tuple(confidence.shape)))
        L.require_cuda(label, "label")
        L.require_cuda(confidence, "confidence")
        if label.device != self.device or confidence.device != self.device:
            raise RuntimeError("EventClusterer: the products live on %s, the buffers on %s" % (label.device, self.device))
        return label.contiguous(), confidence.contiguous()

    def __call__(self, label, confidence: Optional[torch.Tensor] = None) -> Clusters:
        """label a deploy.Products, a sparse.PixelList or the uint8 label map (then `confidence` is the float16 map); launches on
        the current stream of the clusterer's device"""
        label, confidence = self._views(label, confidence)
        self.label = label
        with torch.cuda.device(self.device):
            st = L.stream_ptr()
            IL.label(label.data_ptr(), self.num_classes, self.fill_label, self.connectivity, self.by_class, self.root.data_ptr(),
                     self.status.data_ptr(), self.planes, self.rows, self.cols, st)
            IL.tabulate(label.data_ptr(), confidence.data_ptr(), self.root.data_ptr(), self.num_classes, self.fill_label,
                        self.ids.data_ptr(), self.table.data_ptr(), self.capacity, self.count.data_ptr(), self.scratch.data_ptr(),
                        self.planes, self.rows, self.cols, st)
        if label.dim() == 2:
            return Clusters(self.ids[0], self.root[0], self.table, self.count, self.status)
        return Clusters(self.ids, self.root, self.table, self.count, self.status)


def of_pixels(found: Clusters, pixel_list, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the cluster number of every entry of a sparse.PixelList, int32 [capacity of the list] on the device (ubi_gather_ids on the
    current stream): the first min(count, capacity) entries are written, the rest are left as they were"""
    ids, index = found.ids, pixel_list.index
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 1:
        raise TypeError("clusters.of_pixels: the list's index must be a 1-D int32 tensor")
    if ids.numel() != pixel_list.planes * pixel_list.rows * pixel_list.cols:
        raise ValueError("clusters.of_pixels: the list is of a %d x %d x %d image, the clusters of %d pixels"
                         % (pixel_list.planes, pixel_list.rows, pixel_list.cols, ids.numel()))
    L.require_cuda(ids, "ids")
    L.require_cuda(index, "pixel_list.index")
    if index.device != ids.device:
        raise RuntimeError("clusters.of_pixels: the list lives on %s, the clusters on %s" % (index.device, ids.device))
    if out is None:
        out = torch.full((index.numel(),), -1, dtype=torch.int32, device=ids.device)
    elif not (out.is_cuda and out.dtype == torch.int32 and out.shape == index.shape and out.is_contiguous() and out.device == ids.device):
        raise RuntimeError("clusters.of_pixels: out must be a contiguous int32 tensor of the list's capacity on the device")
    with torch.cuda.device(ids.device):
        IL.gather_ids(ids.data_ptr(), index.data_ptr(), pixel_list.count.data_ptr(), index.numel(), out.data_ptr(), ids.numel(),
                      L.stream_ptr())
    return out
