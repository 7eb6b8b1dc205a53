"""Clusters matched across wire planes by their time profiles, on the device (include/ubresnet_match.h).  The planes of a LArTPC
event share one axis, the time, which is the image row: two clusters of different planes belong together when they deposit charge
in the same time ticks.  For every cluster of at least min_pixels pixels the charge per time bin is summed, and for every pair of
them from two planes the shared bins, the overlap of the two profiles and each side's charge inside the shared bins -- without
`ids` or the view leaving the device.

    cl = clusters.EventClusterer(planes=3, rows=1008, cols=3456, num_classes=4, device="cuda:0")
    pm = planes.PlaneMatcher(cl, slots=512, min_pixels=20, time_bin=1, row_shift=(0, 0, 0), adc_scale=16)   # buffers allocated once
    found = cl(products)
    m = pm(found, view)                      # view: the float32 ADC on the device, or a sparse.SparseEvent
    tab = m.read()                           # the one sync: ncand and status, then that many candidates and their pairs
    tab.matched(0.5), tab.triples(0.5), tab.best(0, 2), tab.containment(), tab.charge_iou(), tab.time_iou()
    m.profiles()                             # [n, T] for a metric of one's own

A candidate is numbered by its position among the clusters that pass min_pixels, in ascending cluster number, so the candidates of
a plane are contiguous.  Every column is an integer, so the tables are the same bytes on every run.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib as L
from . import _match as UL
from .clusters import Clusters, _int
from .shapes import _scale

METRICS = ("containment", "charge_iou", "time_iou")


class PlaneTable:
    """the candidates (int64 [n, 6]: cluster, plane, Q, bins, t_min, t_max) and their pair table (int64 [n, n, 4]: both, I, Qi_in,
    Qj_in; entry (i, j) is defined for i < j) on the host.  All arithmetic is in Python integers with one division at the end.
    `dropped`: the pixels row_shift pushed out of the image so far (status[1])."""

    def __init__(self, candidates: torch.Tensor, pair_table: torch.Tensor, adc_scale: int = 1, time_bin: int = 1, dropped: int = 0):
        n = candidates.shape[0]
        if candidates.dim() != 2 or candidates.shape[1] != UL.CAND_COLUMNS or candidates.dtype != torch.int64:
            raise ValueError("PlaneTable: expected int64 candidates of %d columns, got %s %s"
                             % (UL.CAND_COLUMNS, candidates.dtype, tuple(candidates.shape)))
        if tuple(pair_table.shape) != (n, n, UL.PAIR_COLUMNS) or pair_table.dtype != torch.int64:
            raise ValueError("PlaneTable: expected an int64 pair table of %s, got %s %s"
                             % ((n, n, UL.PAIR_COLUMNS), pair_table.dtype, tuple(pair_table.shape)))
        self.candidates, self.pair_table, self.adc_scale, self.time_bin, self.dropped = candidates, pair_table, adc_scale, time_bin, dropped
        self._cand = candidates.tolist()
        self._rows = None

    def __len__(self):
        return self.candidates.shape[0]

    @property
    def cluster(self):
        return self.candidates[:, 0]

    @property
    def plane(self):
        return self.candidates[:, 1]

    def charge(self):
        """[n] float64: the summed ADC of every candidate, Q / adc_scale"""
        return self.candidates[:, 2].double() / self.adc_scale

    @property
    def bins(self):
        return self.candidates[:, 3]

    def span(self):
        """[n, 2] int64: the first and the last occupied time bin (T and -1 for a candidate without a pixel inside the image)"""
        return self.candidates[:, 4:6]

    def _pair_rows(self):
        """{(i, j): (both, I, Qi_in, Qj_in)} over i < j with both > 0, in ascending (i, j)"""
        if self._rows is None:
            n = len(self)
            upper = torch.triu(torch.ones((n, n), dtype=torch.bool), diagonal=1) & (self.pair_table[:, :, 0] > 0)
            ij = upper.nonzero().tolist()
            vals = self.pair_table[upper].tolist()
            self._rows = {(i, j): tuple(v) for (i, j), v in zip(ij, vals)}
        return self._rows

    def pairs(self):
        """[(i, j)], i < j: the pairs of candidates from two planes that share a time bin"""
        return list(self._pair_rows())

    def containment(self):
        """{(i, j): I / min(Qi, Qj)}: how much of the smaller profile lies under the larger; NaN where the smaller charge is 0"""
        c = self._cand
        return {p: (r[1] / min(c[p[0]][2], c[p[1]][2]) if min(c[p[0]][2], c[p[1]][2]) else float("nan")) for p, r in self._pair_rows().items()}

    def charge_iou(self):
        """{(i, j): I / (Qi + Qj - I)}; NaN where both charges are 0"""
        c = self._cand
        out = {}
        for p, r in self._pair_rows().items():
            union = c[p[0]][2] + c[p[1]][2] - r[1]
            out[p] = r[1] / union if union else float("nan")
        return out

    def time_iou(self):
        """{(i, j): both / (bins_i + bins_j - both)}: the overlap of the occupied bins alone, which no gain enters"""
        c = self._cand
        return {p: r[0] / (c[p[0]][3] + c[p[1]][3] - r[0]) for p, r in self._pair_rows().items()}

    def _metric(self, by):
        if by not in METRICS:
            raise ValueError("PlaneTable: by must be one of %s (got %r)" % (METRICS, by))
        return getattr(self, by)()

    def best(self, plane_a: int, plane_b: int, by: str = "containment"):
        """{i: (j, value)} for every candidate i of plane_a: its best partner j in plane_b and the metric's value there; (-1, NaN)
        where no candidate of plane_b shares a bin with it or every value is NaN.  Ties go to the smaller candidate number."""
        if plane_a == plane_b:
            raise ValueError("PlaneTable: best() is between two different planes (got %r twice)" % (plane_a,))
        c = self._cand
        out = {i: (-1, float("nan")) for i in range(len(c)) if c[i][1] == plane_a}
        for (i, j), v in self._metric(by).items():                      # ascending (i, j): the first of equal values stays
            for mine, other in ((i, j), (j, i)):
                if c[mine][1] == plane_a and c[other][1] == plane_b and v == v:
                    held = out[mine]
                    if held[0] < 0 or v > held[1] or (v == held[1] and other < held[0]):
                        out[mine] = (other, v)
        return out

    def matched(self, threshold: float = 0.5, by: str = "containment"):
        """[(i, j, value)], i < j, ascending: the pairs that are each other's best partner between their two planes and whose value
        is at least the threshold"""
        planes = sorted({r[1] for r in self._cand})
        out = []
        for a in planes:
            for b in planes:
                if a >= b:
                    continue
                ab, ba = self.best(a, b, by), self.best(b, a, by)
                for i, (j, v) in ab.items():
                    if j >= 0 and ba[j][0] == i and v >= threshold:
                        out.append((min(i, j), max(i, j), v))
        return sorted(out)

    def triples(self, threshold: float = 0.5, by: str = "containment"):
        """[(i, j, k)], i < j < k of three different planes, ascending: all three pairs are in matched(threshold, by)"""
        got = {(i, j) for i, j, _ in self.matched(threshold, by)}
        partners = {}
        for i, j in got:
            partners.setdefault(i, []).append(j)
        return sorted((i, j, k) for i, js in partners.items() for j in js for k in partners.get(j, ()) if (i, k) in got)


class Matches(NamedTuple):
    """the result of one call, on the device: `profile` int32 [slots, T] (the bits of uint32 sums), `candidates` int64 [slots, 6],
    `pairs` int64 [slots, slots, 4], `ncand` int64 [1] (the total, also above slots), `status` int64 [2] ([0]: candidates past
    slots, [1]: pixels dropped by row_shift, both so far)"""
    profile: torch.Tensor
    candidates: torch.Tensor
    pairs: torch.Tensor
    ncand: torch.Tensor
    status: torch.Tensor
    adc_scale: int = 1
    time_bin: int = 1

    @property
    def slots(self) -> int:
        return self.candidates.shape[0]

    def _count(self):
        """the one host synchronisation: (ncand, status[0], status[1]); OverflowError if there were more candidates than slots"""
        total, over, dropped = torch.cat([self.ncand, self.status]).tolist()
        if total > self.slots:
            raise OverflowError("Matches: %d candidates, slots=%d: raise slots or min_pixels" % (total, self.slots))
        return total, over, dropped

    def read(self) -> PlaneTable:
        """one sync for ncand and status, then [:n] of the candidate table and [:n, :n] of the pair table and no more"""
        n, _, dropped = self._count()
        return PlaneTable(self.candidates[:n].cpu(), self.pairs[:n, :n].cpu(), self.adc_scale, self.time_bin, dropped)

    def profiles(self) -> torch.Tensor:
        """int64 [n, T] on the host: the time profile of every candidate, in weight units (ADC times adc_scale)"""
        n, _, _ = self._count()
        return self.profile[:n].cpu().to(torch.int64) & 0xFFFFFFFF


class PlaneMatcher:
    """the buffers of ubu_match for the image of one EventClusterer -- profile, candidates, pairs, ncand, status, scratch --
    allocated once; every call overwrites them (status is added to).  row_shift=None is no shift in any plane."""

    def __init__(self, clusterer, slots: int = 512, min_pixels: int = 20, time_bin: int = 1, row_shift=None, adc_scale: int = 16):
        self.adc_scale = _scale(adc_scale)
        self.clusterer = clusterer
        self.planes, self.rows, self.cols = clusterer.planes, clusterer.rows, clusterer.cols
        self.num_classes, self.capacity, self.device = clusterer.num_classes, clusterer.capacity, torch.device(clusterer.device)
        if not UL.MIN_PLANES <= self.planes <= UL.MAX_PLANES:
            raise ValueError("planes: matching needs %d..%d planes (the clusterer has %d)" % (UL.MIN_PLANES, UL.MAX_PLANES, self.planes))
        if self.rows > UL.MAX_ROWS or self.cols > UL.MAX_COLS or self.rows * self.cols > UL.MAX_PLANE_PIXELS:
            raise ValueError("planes: a %d x %d plane is outside the limits: rows <= %d, cols <= %d, rows * cols <= 2^22"
                             % (self.rows, self.cols, UL.MAX_ROWS, UL.MAX_COLS))
        _int("slots", slots, UL.MIN_SLOTS, UL.MAX_SLOTS), _int("min_pixels", min_pixels, 1), _int("time_bin", time_bin, 1, UL.MAX_TIME_BIN)
        if slots % UL.TILE:
            raise ValueError("planes: slots must be a multiple of %d (got %d)" % (UL.TILE, slots))
        if time_bin & (time_bin - 1):
            raise ValueError("planes: time_bin must be a power of two (got %d)" % time_bin)
        if time_bin * self.cols > UL.MAX_BIN_PIXELS:
            raise ValueError("planes: time_bin * cols = %d is above %d: a 32-bit bin could overflow" % (time_bin * self.cols, UL.MAX_BIN_PIXELS))
        row_shift = (0,) * self.planes if row_shift is None else tuple(row_shift)
        if len(row_shift) != self.planes:
            raise ValueError("planes: row_shift must have one entry per plane (%d), got %r" % (self.planes, row_shift))
        for s in row_shift:
            _int("row_shift", s, -UL.MAX_SHIFT, UL.MAX_SHIFT)
        self.slots, self.min_pixels, self.time_bin, self.row_shift = slots, min_pixels, time_bin, row_shift
        self.T = UL.time_bins(self.rows, time_bin)
        self.scratch_bytes = UL.scratch_bytes(self.planes, self.rows, self.cols, time_bin, slots, self.capacity)
        self.profile = torch.zeros((slots, self.T), dtype=torch.int32, device=self.device)
        self.candidates = torch.zeros((slots, UL.CAND_COLUMNS), dtype=torch.int64, device=self.device)
        self.pairs = torch.zeros((slots, slots, UL.PAIR_COLUMNS), dtype=torch.int64, device=self.device)
        self.ncand = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.status = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.scratch = torch.empty(self.scratch_bytes // 8, dtype=torch.int64, device=self.device)
        self._dense = None                                            # the view a SparseEvent is scattered into, kept between calls

    def _view(self, view):
        want = (self.planes, self.rows, self.cols)
        if hasattr(view, "to_view"):                                  # a sparse.SparseEvent
            if (view.planes, view.rows, view.cols) != want:
                raise ValueError("PlaneMatcher: the sparse event is of a %d x %d x %d image, the clusters of %s"
                                 % (view.planes, view.rows, view.cols, want))
            if self._dense is None:
                self._dense = torch.empty((self.planes, 1, self.rows, self.cols), dtype=torch.float32, device=self.device)
            return view.to_view(self.device, out=self._dense)
        if not isinstance(view, torch.Tensor):
            raise TypeError("PlaneMatcher: view must be a torch tensor or a sparse.SparseEvent")
        if view.dtype != torch.float32:
            raise TypeError("PlaneMatcher: view must be float32 (got %s)" % view.dtype)
        shape = tuple(int(s) for s in view.shape)
        if shape not in (want, (self.planes, 1, self.rows, self.cols)):
            raise ValueError("PlaneMatcher: expected a view of %s or [%d, 1, %d, %d]; got %s" % (want, self.planes, self.rows, self.cols, shape))
        L.require_cuda(view, "view")
        if view.device != self.device:
            raise RuntimeError("PlaneMatcher: the view lives on %s, the buffers on %s" % (view.device, self.device))
        view = view.contiguous()
        return view if view.data_ptr() % 16 == 0 else view.clone()

    def __call__(self, found: Clusters, view) -> Matches:
        """found: the Clusters the clusterer returned last; view: the float32 ADC the event was segmented from -- [P,1,rows,cols]
        or [P,rows,cols] on the device, or a sparse.SparseEvent, which is scattered into a buffer kept between calls.  Launches on
        the current stream of the clusterer's device; nothing is read back."""
        cl = self.clusterer
        if not isinstance(found, Clusters):
            raise TypeError("PlaneMatcher: found must be the Clusters of the clusterer")
        if found.table.data_ptr() != cl.table.data_ptr() or found.count.data_ptr() != cl.count.data_ptr() or \
                found.ids.data_ptr() != cl.ids.data_ptr():
            raise ValueError("PlaneMatcher: these Clusters are not the buffers of the clusterer this matcher was sized from")
        view = self._view(view)
        with torch.cuda.device(self.device):
            UL.match(cl.ids.data_ptr(), cl.table.data_ptr(), UL.CLUSTER_FIXED + self.num_classes, cl.count.data_ptr(), self.capacity,
                     view.data_ptr(), float(self.adc_scale), self.planes, self.rows, self.cols, self.min_pixels, self.time_bin,
                     self.row_shift, self.slots, self.profile.data_ptr(), self.candidates.data_ptr(), self.pairs.data_ptr(),
                     self.ncand.data_ptr(), self.status.data_ptr(), self.scratch.data_ptr(), L.stream_ptr())
        return Matches(self.profile, self.candidates, self.pairs, self.ncand, self.status, self.adc_scale, self.time_bin)
