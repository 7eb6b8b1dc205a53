"""Two clusterings of an event matched on the device (include/ubresnet_overlap.h): the contingency table of two id maps over the
same pixels -- one row per pair (a, b) of cluster numbers with its first pixel, pixel count and charge -- without a map or the view
leaving the device.  Which true cluster a reconstructed cluster is, how pure and how complete; how the clusters of by_class=True
nest inside those of by_class=False; how 4- and 8-connected clusterings differ; how stable the clusters are between two inference
settings: all are read off this table.

    co = overlap.ClusterOverlap(planes=3, rows=1008, cols=3456, capacity=131072, adc_scale=16)    # buffers allocated once
    ov = co(found_a, found_b, view)          # clusters.Clusters or int32 id maps; view: the float32 ADC, a SparseEvent, or None
    tab = ov.read()                          # the one sync: status and count, then that many rows
    tab.purity(), tab.efficiency(), tab.matched(0.5, 0.5), tab.unmatched_a(), tab.unmatched_b(), tab.ari()

A value >= 0 of a map is a cluster number, any negative value "none"; a pixel takes part if either side is >= 0, and the pair
(a, -1) holds the pixels of a that no cluster of b covers.  Rows are numbered by their first pixel and every column is an integer,
so the table is the same bytes on every run.  The truth side of a labelled event: truth_products() makes the label map an
EventClusterer clusters.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib as L
from . import _overlap as HL
from .clusters import _int
from .shapes import _scale

NONE = -1


class Match(NamedTuple):
    """per cluster of one side, in ascending cluster number: `cluster` int64 [m], `value` float64 [m] (the largest overlap with a
    cluster of the other side over the cluster's own size; NaN where that size is 0) and `best` int64 [m] (that cluster of the
    other side, -1 where none overlaps)"""
    cluster: torch.Tensor
    value: torch.Tensor
    best: torch.Tensor


class OverlapTable:
    """the rows of the pair table on the host (int64 [n, 6]: a, b, first, pixels, weighted, Q), in ascending order of `first`.  All
    arithmetic is in Python integers with one division at the end; weighted=True counts charge (Q) where weighted=False counts
    pixels."""

    def __init__(self, rows: torch.Tensor, adc_scale: int = 1):
        if rows.dim() != 2 or rows.shape[1] != HL.COLUMNS or rows.dtype != torch.int64:
            raise ValueError("OverlapTable: expected int64 rows of %d columns, got %s %s" % (HL.COLUMNS, rows.dtype, tuple(rows.shape)))
        self.rows, self.adc_scale = rows, adc_scale
        self._list = None

    def __len__(self):
        return self.rows.shape[0]

    @property
    def a(self):
        return self.rows[:, 0]

    @property
    def b(self):
        return self.rows[:, 1]

    @property
    def first(self):
        return self.rows[:, 2]

    @property
    def pixels(self):
        return self.rows[:, 3]

    @property
    def weighted(self):
        return self.rows[:, 4]

    @property
    def charge(self):
        """[n] float64: the summed ADC of the pair, Q / adc_scale"""
        return self.rows[:, 5].double() / self.adc_scale

    def _pairs(self, weighted):
        """[(a, b, first, n)] as Python integers, n the pixel count or Q"""
        if self._list is None:
            self._list = self.rows.tolist()
        col = 5 if weighted else 3
        return [(r[0], r[1], r[2], r[col]) for r in self._list]

    def _sizes(self, side, weighted):
        out = {}
        for p in self._pairs(weighted):
            if p[side] >= 0:
                out[p[side]] = out.get(p[side], 0) + p[3]
        return dict(sorted(out.items()))

    def sizes_a(self, weighted: bool = False):
        """{cluster of a: its pixels (its Q, weighted) summed over its pairs, the pair with none included}"""
        return self._sizes(0, weighted)

    def sizes_b(self, weighted: bool = False):
        return self._sizes(1, weighted)

    def _match(self, side, weighted) -> Match:
        sizes = self._sizes(side, weighted)
        best = {k: (0, -1, NONE) for k in sizes}                      # (overlap, -first, other): the larger overlap, then the smaller first
        for p in self._pairs(weighted):
            mine, other = p[side], p[1 - side]
            if mine < 0 or other < 0:
                continue
            cand = (p[3], -p[2], other)
            if best[mine][2] == NONE or cand[:2] > best[mine][:2]:
                best[mine] = cand
        keys = list(sizes)
        value = [best[k][0] / sizes[k] if sizes[k] else float("nan") for k in keys]
        return Match(torch.tensor(keys, dtype=torch.int64), torch.tensor(value, dtype=torch.float64),
                     torch.tensor([best[k][2] for k in keys], dtype=torch.int64))

    def purity(self, weighted: bool = False) -> Match:
        """per cluster of a: the largest n_ab over b >= 0 divided by n_a, and that b (`best`); ties go to the smaller first"""
        return self._match(0, weighted)

    def efficiency(self, weighted: bool = False) -> Match:
        """per cluster of b: the largest n_ab over a >= 0 divided by n_b, and that a (`best`)"""
        return self._match(1, weighted)

    def matched(self, min_purity: float = 0.0, min_efficiency: float = 0.0, weighted: bool = False):
        """[(a, b, purity of a, efficiency of b)], in ascending a: the pairs that are each other's best match and pass both
        thresholds"""
        pur, eff = self.purity(weighted), self.efficiency(weighted)
        of_b = {k: (v, a) for k, v, a in zip(eff.cluster.tolist(), eff.value.tolist(), eff.best.tolist())}
        out = []
        for a, p, b in zip(pur.cluster.tolist(), pur.value.tolist(), pur.best.tolist()):
            if b >= 0 and of_b[b][1] == a and p >= min_purity and of_b[b][0] >= min_efficiency:
                out.append((a, b, p, of_b[b][0]))
        return out

    def unmatched_a(self, min_purity: float = 0.0, min_efficiency: float = 0.0, weighted: bool = False):
        """the clusters of a in no pair of matched(), ascending"""
        got = {m[0] for m in self.matched(min_purity, min_efficiency, weighted)}
        return [k for k in self.sizes_a() if k not in got]

    def unmatched_b(self, min_purity: float = 0.0, min_efficiency: float = 0.0, weighted: bool = False):
        got = {m[1] for m in self.matched(min_purity, min_efficiency, weighted)}
        return [k for k in self.sizes_b() if k not in got]

    def ari(self) -> float:
        """the adjusted Rand index of the two clusterings over the pixels where both sides are >= 0.  The three binomial sums are
        Python integers.  NaN below two such pixels; 1.0 where the denominator is zero (both sides one cluster, or all singletons)."""
        both = [p for p in self._pairs(False) if p[0] >= 0 and p[1] >= 0]
        n = sum(p[3] for p in both)
        if n < 2:
            return float("nan")
        na, nb = {}, {}
        for a, b, _, c in both:
            na[a] = na.get(a, 0) + c
            nb[b] = nb.get(b, 0) + c
        pairs = lambda m: m * (m - 1) // 2
        s_ab, s_a, s_b, s_n = sum(pairs(p[3]) for p in both), sum(pairs(v) for v in na.values()), sum(pairs(v) for v in nb.values()), pairs(n)
        num, den = 2 * (s_ab * s_n - s_a * s_b), (s_a + s_b) * s_n - 2 * s_a * s_b
        return 1.0 if den == 0 else num / den


class Overlap(NamedTuple):
    """the pair table of one call, on the device: `table` int64 [capacity, 6], `count` int64 [1] (the total, also above capacity),
    `status` int64 [2] ([0]: pixels whose pair found no slot, so far)"""
    table: torch.Tensor
    count: torch.Tensor
    status: torch.Tensor
    adc_scale: int = 1
    slots: int = 0

    @property
    def capacity(self) -> int:
        return self.table.shape[0]

    def read(self) -> OverlapTable:
        """the one host synchronisation: status and count are copied, then that many rows and no more.  OverflowError if there
        were more pairs than capacity, or if pixels found no slot."""
        dropped, total = int(self.status[0].item()), int(self.count.item())
        if dropped != 0:
            raise OverflowError("Overlap: %d pixels found no slot among slots=%d (status[0]); the table is not valid: raise slots"
                                % (dropped, self.slots))
        if total > self.capacity:
            raise OverflowError("Overlap: %d pairs, capacity %d (slots=%d): raise capacity, and slots with it"
                                % (total, self.capacity, self.slots))
        return OverlapTable(self.table[:total].cpu(), self.adc_scale)


class ClusterOverlap:
    """the buffers of ubh_overlap for one image size -- table, count, status, scratch -- allocated once; every call overwrites
    table and count (status is added to).  slots=None takes ubh_default_slots(capacity): a load of at most 0.5."""

    def __init__(self, planes: int = 3, rows: int = 1008, cols: int = 3456, capacity: int = 131072, slots: Optional[int] = None,
                 adc_scale: int = 16, device="cuda:0"):
        _int("planes", planes, 1), _int("rows", rows, 1), _int("cols", cols, 1), _int("capacity", capacity, 1)
        if planes * rows * cols > HL.MAX_PIXELS:
            raise ValueError("overlap: %d x %d x %d pixels do not fit an int32 pixel index" % (planes, rows, cols))
        self.adc_scale = _scale(adc_scale)
        if slots is None:
            slots = HL.default_slots(capacity)
        _int("slots", slots, HL.MIN_SLOTS, HL.MAX_SLOTS)
        if slots & (slots - 1):
            raise ValueError("overlap: slots must be a power of two (got %d)" % slots)
        self.planes, self.rows, self.cols, self.capacity, self.slots = planes, rows, cols, capacity, slots
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ubresnet_amd: ClusterOverlap needs a ROCm device (got %s); the HIP path has no CPU fallback" % self.device)
        self.scratch_bytes = HL.scratch_bytes(planes, rows, cols, slots)
        self.table = torch.zeros((capacity, HL.COLUMNS), dtype=torch.int64, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.status = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.scratch = torch.empty(self.scratch_bytes // 8, dtype=torch.int64, device=self.device)
        self._dense = None                                            # the view a SparseEvent is scattered into, kept between calls

    def _ids(self, t, what):
        if hasattr(t, "ids") and hasattr(t, "table"):                 # a clusters.Clusters
            t = t.ids
        if not isinstance(t, torch.Tensor):
            raise TypeError("ClusterOverlap: %s must be a clusters.Clusters or a torch tensor" % what)
        if t.dtype != torch.int32:
            raise TypeError("ClusterOverlap: %s must be int32 (got %s)" % (what, t.dtype))
        want = (self.planes, self.rows, self.cols)
        shape = tuple(int(s) for s in t.shape)
        if shape != want and not (self.planes == 1 and shape == want[1:]):
            raise ValueError("ClusterOverlap: expected %s of %s or, for one plane, [rows, cols]; got %s" % (what, want, shape))
        L.require_cuda(t, what)
        if t.device != self.device:
            raise RuntimeError("ClusterOverlap: %s lives on %s, the buffers on %s" % (what, t.device, self.device))
        t = t.contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()

    def _view(self, view):
        want = (self.planes, self.rows, self.cols)
        if hasattr(view, "to_view"):                                  # a sparse.SparseEvent
            if (view.planes, view.rows, view.cols) != want:
                raise ValueError("ClusterOverlap: the sparse event is of a %d x %d x %d image, the maps of %s"
                                 % (view.planes, view.rows, view.cols, want))
            if self._dense is None:
                self._dense = torch.empty((self.planes, 1, self.rows, self.cols), dtype=torch.float32, device=self.device)
            return view.to_view(self.device, out=self._dense)
        if not isinstance(view, torch.Tensor):
            raise TypeError("ClusterOverlap: view must be a torch tensor, a sparse.SparseEvent or None")
        if view.dtype != torch.float32:
            raise TypeError("ClusterOverlap: view must be float32 (got %s)" % view.dtype)
        shape = tuple(int(s) for s in view.shape)
        if shape not in (want, (self.planes, 1, self.rows, self.cols)) and not (self.planes == 1 and shape == want[1:]):
            raise ValueError("ClusterOverlap: expected a view of %s, [%d, 1, %d, %d] or, for one plane, [rows, cols]; got %s"
                             % (want, self.planes, self.rows, self.cols, shape))
        L.require_cuda(view, "view")
        if view.device != self.device:
            raise RuntimeError("ClusterOverlap: the view lives on %s, the buffers on %s" % (view.device, self.device))
        view = view.contiguous()
        return view if view.data_ptr() % 16 == 0 else view.clone()

    def __call__(self, a, b, view=None) -> Overlap:
        """a, b: each a clusters.Clusters or an int32 id map of the image on the device; view: the float32 ADC -- [P,1,rows,cols],
        [P,rows,cols] or [rows,cols] -- or a sparse.SparseEvent, which is scattered into a buffer kept between calls, or None
        (then `weighted` and `Q` are 0).  Launches on the current stream of the buffers' device; nothing is read back."""
        ia, ib = self._ids(a, "a"), self._ids(b, "b")
        v = None if view is None else self._view(view)
        with torch.cuda.device(self.device):
            HL.overlap(ia.data_ptr(), ib.data_ptr(), None if v is None else v.data_ptr(), float(self.adc_scale), self.table.data_ptr(),
                       self.capacity, self.count.data_ptr(), self.status.data_ptr(), self.scratch.data_ptr(), self.slots, self.planes,
                       self.rows, self.cols, L.stream_ptr())
        return Overlap(self.table, self.count, self.status, self.adc_scale, self.slots)


def truth_products(truth: torch.Tensor, view: torch.Tensor, adc_threshold: float = 10.0, fill_label: int = 255, ignore_index: int = -100):
    """the truth side of a labelled event as an EventClusterer takes it: (label uint8 like truth -- fill_label where the ADC is at
    or below the threshold or the truth is ignore_index --, confidence float16 of ones).  Plain torch ops on the tensors' device:
    not a hot path.  truth: an integer class map [P, rows, cols]; view: the float32 ADC, [P, rows, cols] or [P, 1, rows, cols]."""
    if not isinstance(truth, torch.Tensor) or truth.is_floating_point() or truth.dtype == torch.bool:
        raise TypeError("truth_products: truth must be an integer tensor")
    if not isinstance(view, torch.Tensor) or view.dtype != torch.float32:
        raise TypeError("truth_products: view must be a float32 tensor")
    _int("fill_label", fill_label, 0, 255)
    if view.dim() == truth.dim() + 1 and view.shape[1] == 1:
        view = view[:, 0]
    if view.shape != truth.shape:
        raise ValueError("truth_products: truth is %s, the view %s" % (tuple(truth.shape), tuple(view.shape)))
    wide = truth.to(torch.int64)
    dark = ~(view > adc_threshold) | (wide == ignore_index) | (wide < 0) | (wide > 255)       # NaN is dark
    label = torch.where(dark, torch.full_like(wide, fill_label), wide).to(torch.uint8)
    return label.contiguous(), torch.ones(label.shape, dtype=torch.float16, device=label.device)
