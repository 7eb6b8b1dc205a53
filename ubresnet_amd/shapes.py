"""Per-cluster charge and shape on the device (include/ubresnet_moment.h): for every cluster an EventClusterer found, the ADC sum,
the ADC sum per class and the first and second moments of the charge, from which centroid, principal axis, length, width and
linearity follow -- without `ids` or the view leaving the device.  The pixel count of a cluster is no energy proxy (a shower's halo
is many faint pixels, a Bragg peak few bright ones); the charge is.

    cl = clusters.EventClusterer(planes=3, rows=1008, cols=3456, num_classes=4, device="cuda:0")
    cm = shapes.ClusterMoments(cl, adc_scale=16)       # capacity x (9 + C) int64, allocated once
    found = cl(products)
    mom = cm(found, view)                              # view: the float32 ADC on the device, or a sparse.SparseEvent
    tab = mom.read(min_pixels=1)                       # the one sync: the count, then that many rows of both tables
    tab.charge(), tab.class_charge(), tab.charge_fractions(), tab.centroid(), tab.extent(), tab.axis(), tab.linearity()
    tab.clusters.pixels, tab.clusters.bbox             # the ClusterTable of the same rows

The weight of a pixel is its ADC times adc_scale (a power of two in 1..256) rounded to the nearest integer, ties to even, and
clamped to 0..65535; every column of the table is an integer sum, so the table is the same bits on every run.  NaN and negative
ADC count into `odd`, clamped values into `clipped`.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import _lib as L
from . import _moment as ML
from .clusters import Clusters, ClusterTable, _int


class ShapeTable:
    """the rows of the charge table on the host (int64 [n, 9 + C]) beside the ClusterTable of the same clusters (`clusters`)"""

    def __init__(self, rows: torch.Tensor, clusters: ClusterTable, adc_scale: int):
        if rows.shape[0] != len(clusters) or rows.shape[1] != ML.TABLE_FIXED + clusters.num_classes:
            raise ValueError("ShapeTable: %s rows do not belong to a cluster table of %d rows and %d classes"
                             % (tuple(rows.shape), len(clusters), clusters.num_classes))
        self.rows, self.clusters, self.adc_scale = rows, clusters, adc_scale
        self._cov = None

    def __len__(self):
        return self.rows.shape[0]

    @property
    def weighted(self):
        return self.rows[:, 0]

    @property
    def clipped(self):
        return self.rows[:, 1]

    @property
    def odd(self):
        return self.rows[:, 2]

    def charge(self):
        """[n] float64: the summed ADC, Q / adc_scale"""
        return self.rows[:, 3].double() / self.adc_scale

    def class_charge(self):
        """[n, C] float64: the summed ADC of the pixels of every class"""
        return self.rows[:, ML.TABLE_FIXED:].double() / self.adc_scale

    def charge_fractions(self):
        """[n, C] float64: the share of every class in the cluster's charge; NaN where the cluster has none"""
        q = self.rows[:, 3].double()
        return self.rows[:, ML.TABLE_FIXED:].double() / q.masked_fill(q == 0, float("nan")).unsqueeze(1)

    def centroid(self):
        """[n, 2] float64: the charge-weighted mean row and column; NaN where the cluster has no charge"""
        q = self.rows[:, 3].double()
        return self.rows[:, 4:6].double() / q.masked_fill(q == 0, float("nan")).unsqueeze(1)

    def covariance(self):
        """[n, 2, 2] float64: the central second moments of the charge.  (Q Qrr - Qr^2) / Q^2 and its like are formed in Python
        integers -- the products reach 2^100 -- and rounded once: float64 products of the raw sums cancel for a thin cluster far
        from the origin.  NaN where the cluster has no charge."""
        if self._cov is None:
            nan = float("nan")
            out = []
            for Q, Qr, Qc, Qrr, Qrc, Qcc in self.rows[:, 3:9].tolist():
                if Q == 0:
                    out.append((nan, nan, nan, nan))
                    continue
                d = Q * Q
                rc = (Q * Qrc - Qr * Qc) / d
                out.append(((Q * Qrr - Qr * Qr) / d, rc, rc, (Q * Qcc - Qc * Qc) / d))
            self._cov = torch.tensor(out, dtype=torch.float64).reshape(len(out), 2, 2)
        return self._cov

    def _eigen(self):
        s = self.covariance()
        srr, src, scc = s[:, 0, 0], s[:, 0, 1], s[:, 1, 1]
        half, diff = (srr + scc) / 2, (srr - scc) / 2
        root = torch.hypot(diff, src)
        major, minor = half + root, (half - root).clamp_min(0.0)      # NaN stays NaN
        return srr, src, scc, major, minor

    def extent(self):
        """[n, 2] float64: the square roots of the eigenvalues of the covariance, major then minor (the minor clamped at 0); a
        uniform line of length L has a major extent of L / (2 sqrt 3)"""
        _, _, _, major, minor = self._eigen()
        return torch.stack([major.sqrt(), minor.sqrt()], dim=1)

    def axis(self):
        """[n, 2] float64: the unit eigenvector (d_row, d_col) of the major eigenvalue, with d_col > 0, or d_col == 0 and
        d_row > 0; (0, 1) for an isotropic cluster; NaN where the cluster has no charge"""
        srr, src, scc, major, _ = self._eigen()
        a_r, a_c = major - scc, src                                    # from the second row of (S - major) v = 0
        b_r, b_c = src, major - srr                                    # from the first; take the longer of the two
        use_b = (major - srr).abs() > (major - scc).abs()
        dr, dc = torch.where(use_b, b_r, a_r), torch.where(use_b, b_c, a_c)
        flat = src == 0                                                # the axes of the image are the eigenvectors
        dr = torch.where(flat, (srr > scc).double(), dr)
        dc = torch.where(flat, (srr <= scc).double(), dc)
        n = torch.hypot(dr, dc)
        dr, dc = dr / n, dc / n
        flip = (dc < 0) | ((dc == 0) & (dr < 0))
        dr, dc = torch.where(flip, -dr, dr), torch.where(flip, -dc, dc)
        out = torch.stack([dr, dc], dim=1)
        return out.masked_fill(torch.isnan(major).unsqueeze(1), float("nan"))

    def linearity(self):
        """[n] float64: 1 - minor / major eigenvalue: 1 for a line, 0 for an isotropic cluster; NaN where the major eigenvalue is 0
        (one pixel) or the cluster has no charge"""
        _, _, _, major, minor = self._eigen()
        return 1.0 - minor / major.masked_fill(major == 0, float("nan"))

    def length(self):
        """[n] float64: 2 sqrt(3) times the major extent -- exact for a uniform line"""
        return 2.0 * math.sqrt(3.0) * self.extent()[:, 0]

    def width(self):
        """[n] float64: 2 sqrt(3) times the minor extent"""
        return 2.0 * math.sqrt(3.0) * self.extent()[:, 1]


class Moments(NamedTuple):
    """the charge table of one event, on the device: `table` int64 [capacity, 9 + C] beside the `clusters` it belongs to"""
    table: torch.Tensor
    clusters: Clusters
    adc_scale: int

    def read(self, min_pixels: int = 1) -> ShapeTable:
        """the one host synchronisation: the count is copied, then that many rows of both tables and no more.  OverflowError if
        there were more clusters than capacity.  Clusters of fewer than min_pixels pixels are dropped from both tables alike."""
        _int("min_pixels", min_pixels, 0)
        found = self.clusters
        total = int(found.count.item())
        if total > found.capacity:
            raise OverflowError("Clusters: %d clusters, capacity %d" % (total, found.capacity))
        rows, mine = found.table[:total].cpu(), self.table[:total].cpu()
        if min_pixels > 1:
            keep = rows[:, 1] >= min_pixels
            rows, mine = rows[keep], mine[keep]
        image = (1,) * (3 - found.ids.dim()) + tuple(int(s) for s in found.ids.shape)
        from . import _cluster as IL
        return ShapeTable(mine, ClusterTable(rows, found.table.shape[1] - IL.TABLE_FIXED, image, total), self.adc_scale)


def _scale(adc_scale):
    if isinstance(adc_scale, bool) or not isinstance(adc_scale, int) or adc_scale not in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        raise ValueError("shapes: adc_scale must be a power of two in 1..%d (got %r)" % (ML.MAX_SCALE, adc_scale))
    return adc_scale


class ClusterMoments:
    """the charge table of ubm_moments for the buffers of one EventClusterer, allocated once; every call overwrites it.  The
    clusterer's image must be inside the overflow limits: rows, cols <= 4096 and rows * cols <= 2^22."""

    def __init__(self, clusterer, adc_scale: int = 16):
        self.adc_scale = _scale(adc_scale)
        self.clusterer = clusterer
        self.planes, self.rows, self.cols = clusterer.planes, clusterer.rows, clusterer.cols
        self.num_classes, self.capacity, self.device = clusterer.num_classes, clusterer.capacity, torch.device(clusterer.device)
        if self.rows > ML.MAX_ROWS or self.cols > ML.MAX_COLS or self.rows * self.cols > ML.MAX_PLANE_PIXELS:
            raise ValueError("shapes: a %d x %d plane is outside the overflow limits: rows <= %d, cols <= %d, rows * cols <= 2^22"
                             % (self.rows, self.cols, ML.MAX_ROWS, ML.MAX_COLS))
        self.table = torch.zeros((self.capacity, ML.TABLE_FIXED + self.num_classes), dtype=torch.int64, device=self.device)
        self._dense = None                                            # the view a SparseEvent is scattered into, kept between calls

    def _view(self, view):
        want = (self.planes, self.rows, self.cols)
        if hasattr(view, "to_view"):                                  # a sparse.SparseEvent
            if (view.planes, view.rows, view.cols) != want:
                raise ValueError("ClusterMoments: the sparse event is of a %d x %d x %d image, the clusters of %s"
                                 % (view.planes, view.rows, view.cols, want))
            if self._dense is None:
                self._dense = torch.empty((self.planes, 1, self.rows, self.cols), dtype=torch.float32, device=self.device)
            return view.to_view(self.device, out=self._dense)
        if not isinstance(view, torch.Tensor):
            raise TypeError("ClusterMoments: view must be a torch tensor or a sparse.SparseEvent")
        if view.dtype != torch.float32:
            raise TypeError("ClusterMoments: view must be float32 (got %s)" % view.dtype)
        shape = tuple(int(s) for s in view.shape)
        if shape not in (want, (self.planes, 1, self.rows, self.cols)) and not (self.planes == 1 and shape == want[1:]):
            raise ValueError("ClusterMoments: expected a view of %s, [%d, 1, %d, %d] or, for one plane, [rows, cols]; got %s"
                             % (want, self.planes, self.rows, self.cols, shape))
        L.require_cuda(view, "view")
        if view.device != self.device:
            raise RuntimeError("ClusterMoments: the view lives on %s, the buffers on %s" % (view.device, self.device))
        view = view.contiguous()
        return view if view.data_ptr() % 16 == 0 else view.clone()

    def __call__(self, found: Clusters, view) -> Moments:
        """found: the Clusters the clusterer returned last; view: the float32 ADC the event was segmented from -- [P,1,rows,cols],
        [P,rows,cols] or [rows,cols] on the device, or a sparse.SparseEvent, which is scattered into a buffer kept between calls.
        The class map is the one the clusterer was last called with (EventClusterer.label).  Launches on the current stream of
        the clusterer's device."""
        cl = self.clusterer
        if not isinstance(found, Clusters):
            raise TypeError("ClusterMoments: found must be the Clusters of the clusterer")
        if found.table.data_ptr() != cl.table.data_ptr() or found.count.data_ptr() != cl.count.data_ptr() or \
                found.ids.data_ptr() != cl.ids.data_ptr():
            raise ValueError("ClusterMoments: these Clusters are not the buffers of the clusterer this table was sized from")
        label = cl.label
        if not isinstance(label, torch.Tensor) or label.dtype != torch.uint8 or label.numel() != self.planes * self.rows * self.cols:
            raise RuntimeError("ClusterMoments: the clusterer holds no class map of %d x %d x %d: call it first"
                               % (self.planes, self.rows, self.cols))
        view = self._view(view)
        L.require_cuda(label, "label")
        label = label.contiguous()
        if label.data_ptr() % 4:
            label = label.clone()
        with torch.cuda.device(self.device):
            ML.moments(cl.ids.data_ptr(), label.data_ptr(), view.data_ptr(), self.num_classes, float(self.adc_scale),
                       self.table.data_ptr(), self.capacity, cl.count.data_ptr(), self.planes, self.rows, self.cols, L.stream_ptr())
        return Moments(self.table, found, self.adc_scale)
