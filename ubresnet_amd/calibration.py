"""Temperature calibration on the device: fit one temperature per wire plane on the lit, labelled pixels, and apply it to the
scores of every forward of whole-view inference.

``EventScorer`` measures how far the confidence in ``deploy.Products`` is from the accuracy it promises; this module corrects it
by temperature scaling: the scores l of a pixel become ``log_softmax(l / T)``, with one scalar T per group (wire plane) that
minimises the negative log-likelihood (NLL) of a held-out labelled set.  With beta = 1 / T,

    NLL(beta) = lse_c(beta l_c) - beta l_t,    g = dNLL/dbeta = E_p[l] - l_t,    h = d2NLL/dbeta2 = Var_p[l] >= 0,

so the NLL is convex in beta and its minimum is the root of g.

    fit = TemperatureFit(num_classes=4, groups=3)
    for view, truth in events:                       # a segmenter with tta, blend and temperature OFF
        fit.add(segmenter(view), truth, lit=view)    # one ubf_accumulate call on the current stream; nothing is read back
    cal = fit.read()                                 # the one host sync
    print(cal.temperatures, cal.at_edge)
    seg = WholeViewSegmenter(model, ..., temperature=cal)

``TemperatureFit.add`` sums NLL, g and h at a fixed grid of temperatures (33 log-spaced on [1/4, 4] unless given) into a device
table ``double [groups][K][3]`` (libubresnet_calib.so, include/ubresnet_calib.h: per-pixel terms in fp32, sums in fp64 in a fixed
order, no atomics).  ``Calibration`` finds, per group, the grid interval where g changes sign and takes the root of the cubic
Hermite interpolant of g there (h is its derivative) by bisection in float64.  It never extrapolates: a g of one sign over the
whole grid gives the end of the grid and ``at_edge``.  ``TemperatureScale`` carries the temperatures into deployment and into a
checkpoint.  There is no fallback: a missing library is a RuntimeError.
"""
from __future__ import annotations

import numpy as np

from . import _calib

__all__ = ["TemperatureFit", "TemperatureScale", "Calibration", "default_temps", "hermite_root", "solve_group"]

COUNTERS = ("counted", "ignored", "nonfinite")


def default_temps():
    """33 temperatures log-spaced on [1/4, 4] (T = 1 is the middle one)"""
    return [4.0 ** (i / 16.0 - 1.0) for i in range(33)]


def _betas32(temps):
    """the inverse temperatures as the device reads them: 1 / T rounded once to float32"""
    return np.array([1.0 / t for t in temps], dtype=np.float64).astype(np.float32)


def _positive_finite(name, values):
    try:
        out = [float(v) for v in values]
    except (TypeError, ValueError):
        raise ValueError("%s must be a float or a sequence of floats (got %r)" % (name, values))
    if not out:
        raise ValueError("%s is empty" % name)
    for v in out:
        if not (v > 0.0 and v < float("inf")):
            raise ValueError("%s must be positive and finite (got %r)" % (name, v))
    return out


def hermite_root(b0, b1, g0, g1, h0, h1):
    """the root in [b0, b1] of the cubic Hermite interpolant of g (values g0 <= 0 <= g1 at the ends, derivatives h0, h1), by
    bisection in float64 until the interval no longer shrinks.  Pure Python."""
    b0, b1, g0, g1, h0, h1 = (float(v) for v in (b0, b1, g0, g1, h0, h1))
    if g0 == 0.0:
        return b0
    if g1 == 0.0:
        return b1
    if not (g0 < 0.0 < g1 and b0 < b1):
        raise ValueError("hermite_root: g must change sign from below on an interval of positive length")
    w = b1 - b0

    def f(s):
        s2, s3 = s * s, s * s * s
        return ((2 * s3 - 3 * s2 + 1) * g0 + (s3 - 2 * s2 + s) * w * h0 + (-2 * s3 + 3 * s2) * g1 + (s3 - s2) * w * h1)

    lo, hi = 0.0, 1.0
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        v = f(mid)
        if v == 0.0:
            lo = hi = mid
            break
        if v < 0.0:
            lo = mid
        else:
            hi = mid
    return b0 + 0.5 * (lo + hi) * w


def solve_group(betas, g, h, counted):
    """-> (beta, at_edge, empty) of one group: `betas`, `g`, `h` float64 over the grid (any order), `counted` its pixels.
    No counted pixel: (1.0, False, True).  g == 0 at a grid point: that point.  Otherwise, in ascending beta, the first interval
    with g < 0 at its lower and g > 0 at its upper end, and hermite_root there; if there is none, the end of the grid the sign of
    g at the smallest beta points to (g > 0: the NLL rises with beta, the smallest beta; else the largest) with at_edge."""
    if int(counted) == 0:
        return 1.0, False, True
    order = sorted(range(len(betas)), key=lambda i: float(betas[i]))
    b = [float(betas[i]) for i in order]
    gs = [float(g[i]) for i in order]
    hs = [float(h[i]) for i in order]
    for bi, gi in zip(b, gs):
        if gi == 0.0:
            return bi, False, False
    for i in range(len(b) - 1):
        if gs[i] < 0.0 < gs[i + 1]:
            return hermite_root(b[i], b[i + 1], gs[i], gs[i + 1], hs[i], hs[i + 1]), False, False
    return (b[0] if gs[0] > 0.0 else b[-1]), True, False


class TemperatureScale(object):
    """One temperature per group (wire plane), positive and finite; a float is one group.  `apply_` rescales float32 scores
    [n, C, H, W] on the device in place: image i becomes log_softmax(scores[i] / T[groups[i]]) (ubf_apply)."""

    def __init__(self, temperature):
        if isinstance(temperature, TemperatureScale):
            temperature = temperature.temperatures
        if isinstance(temperature, (int, float, np.integer, np.floating)) and not isinstance(temperature, bool):
            temperature = [temperature]
        if isinstance(temperature, (str, bytes, bool)):
            raise ValueError("TemperatureScale: temperature must be a float or a sequence of floats (got %r)" % (temperature,))
        self.temperatures = _positive_finite("TemperatureScale: temperature", temperature)
        self._dev = {}

    def __len__(self):
        return len(self.temperatures)

    def __repr__(self):
        return "TemperatureScale(%r)" % (self.temperatures,)

    def state_dict(self):
        """tensors only, so that it travels inside the dict deploy.save_checkpoint writes and loads with weights_only"""
        import torch
        return {"temperature": torch.tensor(self.temperatures, dtype=torch.float64)}

    def load_state_dict(self, state):
        t = state["temperature"]
        self.temperatures = _positive_finite("TemperatureScale: temperature", t.tolist() if hasattr(t, "tolist") else t)
        self._dev = {}
        return self

    def group_list(self, n, groups=None):
        """the group of each of n images: `groups` as given (checked), or image i -> i when there are n temperatures, or all
        group 0 when there is one"""
        G = len(self.temperatures)
        if groups is None:
            if G == 1:
                return [0] * n
            if G == n:
                return list(range(n))
            raise ValueError("TemperatureScale: %d temperatures and %d images: say which group each image is" % (G, n))
        groups = [int(v) for v in groups]
        if len(groups) != n or any(not 0 <= v < G for v in groups):
            raise ValueError("TemperatureScale: groups must be %d indices in 0..%d (got %r)" % (n, G - 1, groups))
        return groups

    def betas_for(self, groups):
        """float32 numpy array: 1 / T of each listed group, rounded once"""
        return _betas32([self.temperatures[v] for v in groups])

    def device_betas(self, groups, device):
        """the same on the device; built once per (groups, device)"""
        import torch
        key = (tuple(groups), str(device))
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.betas_for(groups)).to(device)
        return self._dev[key]

    def apply_(self, scores, groups=None):
        import torch
        if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or scores.dim() not in (3, 4):
            raise ValueError("TemperatureScale.apply_: scores must be a float32 tensor [n, C, H, W] or [C, H, W]")
        if not scores.is_cuda:
            raise RuntimeError("TemperatureScale.apply_: scores must be on a CUDA device; there is no CPU fallback")
        if not scores.is_contiguous():
            raise ValueError("TemperatureScale.apply_: scores must be contiguous (the call works in place)")
        shape = scores.shape if scores.dim() == 4 else (1,) + tuple(scores.shape)
        betas = self.device_betas(self.group_list(shape[0], groups), scores.device)
        with torch.cuda.device(scores.device):
            _calib.apply(scores.data_ptr(), scores.data_ptr(), betas.data_ptr(), shape[0], shape[1], shape[2], shape[3],
                         torch.cuda.current_stream(scores.device).cuda_stream)
        return scores


def as_scale(temperature):
    """what `temperature=` of the deployment calls accepts -> TemperatureScale, or None for None"""
    if temperature is None:
        return None
    if isinstance(temperature, Calibration):
        return temperature.scale()
    return TemperatureScale(temperature)


class Calibration(object):
    """What TemperatureFit.read() returns, on the host.  `table` float64 [groups, K, 3]: the sums of NLL, g and h; `counters`
    uint64 [groups, 3]: counted, ignored, non-finite; `temps` the grid and `betas` float64 [K], the float32 inverse temperatures
    the device summed at.  `temperatures`, `at_edge`, `empty`: one entry per group (solve_group)."""

    def __init__(self, temps, table, counters):
        self.temps = [float(t) for t in temps]
        self.betas = _betas32(self.temps).astype(np.float64)
        self.table = np.ascontiguousarray(table, dtype=np.float64)
        self.counters = np.ascontiguousarray(counters, dtype=np.uint64)
        K = len(self.temps)
        if self.table.ndim != 3 or self.table.shape[1:] != (K, 3) or self.counters.shape != (self.table.shape[0], 3):
            raise ValueError("Calibration: expected table [groups, %d, 3] and counters [groups, 3], got %s and %s"
                             % (K, self.table.shape, self.counters.shape))
        self.groups = self.table.shape[0]
        solved = [solve_group(self.betas, self.table[g, :, 1], self.table[g, :, 2], self.counters[g, 0]) for g in range(self.groups)]
        self.inverse_temperatures = [s[0] for s in solved]
        self.temperatures = [1.0 / s[0] for s in solved]
        self.at_edge = [s[1] for s in solved]
        self.empty = [s[2] for s in solved]

    def _mean(self, group, word):
        n = int(self.counters[group, 0])
        return self.table[group, :, word] / n if n else np.full(len(self.temps), np.nan)

    def nll(self, group=0):
        """mean NLL per counted pixel over `temps`, float64 (nan without pixels)"""
        return self._mean(group, 0)

    def gradient(self, group=0):
        """mean dNLL/dbeta per counted pixel over `temps`"""
        return self._mean(group, 1)

    def curvature(self, group=0):
        """mean d2NLL/dbeta2 per counted pixel over `temps`"""
        return self._mean(group, 2)

    def temperature(self, group=0):
        return self.temperatures[group]

    def tallies(self, group=0):
        return dict((k, int(v)) for k, v in zip(COUNTERS, self.counters[group]))

    def scale(self):
        return TemperatureScale(self.temperatures)

    def __str__(self):
        lines = []
        for g in range(self.groups):
            t = self.tallies(g)
            lines.append("group %d: T = %.4f%s%s  (%d counted, %d ignored, %d non-finite)"
                         % (g, self.temperatures[g], " (at the edge of the grid)" if self.at_edge[g] else "",
                            " (no pixel: 1.0)" if self.empty[g] else "", t["counted"], t["ignored"], t["nonfinite"]))
        return "\n".join(lines)


class TemperatureFit(object):
    """A device table of NLL, gradient and curvature sums per group over a grid of temperatures; see the module docstring.
    Arguments are checked here, before anything touches the device; the table is allocated and zeroed by the first add()."""

    def __init__(self, num_classes, groups=1, temps=None, adc_threshold=10.0, device="cuda"):
        for name, v, lo, hi in (("num_classes", num_classes, 1, _calib.MAX_CLASSES), ("groups", groups, 1, _calib.MAX_GROUPS)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError("TemperatureFit: %s must be an int in %d..%d (got %r)" % (name, lo, hi, v))
        self.num_classes, self.groups = int(num_classes), int(groups)
        self.temps = _positive_finite("TemperatureFit: temps", default_temps() if temps is None else temps)
        if len(self.temps) > _calib.MAX_TEMPS:
            raise ValueError("TemperatureFit: %d temperatures are more than %d" % (len(self.temps), _calib.MAX_TEMPS))
        self.betas = _betas32(self.temps)
        if not (np.isfinite(self.betas).all() and (self.betas > 0).all()):
            raise ValueError("TemperatureFit: a temperature whose inverse is not a positive finite float32")
        if adc_threshold is not None and not float(adc_threshold) == float(adc_threshold):
            raise ValueError("TemperatureFit: adc_threshold is NaN")
        self.adc_threshold = None if adc_threshold is None else float(adc_threshold)
        self.device = device
        self._table = self._counters = self._betas = self._scratch = None
        self._groups = {}
        self.calls = 0

    def _shapes(self, scores, truth, lit):
        import torch
        for name, t in (("scores", scores), ("truth", truth)) + ((("lit", lit),) if lit is not None else ()):
            if not isinstance(t, torch.Tensor):
                raise ValueError("TemperatureFit.add: %s must be a tensor (got %s)" % (name, type(t).__name__))
        if scores.dtype != torch.float32:
            raise ValueError("TemperatureFit.add: scores must be float32 (got %s)" % scores.dtype)
        if truth.dtype not in (torch.uint8, torch.int64):
            raise ValueError("TemperatureFit.add: truth must be uint8 or int64 (got %s)" % truth.dtype)
        if scores.dim() == 3:                                  # the stacked form of WholeViewSegmenter: one [C, rows, cols] map
            scores = scores[None]
            truth = truth[None] if truth.dim() == 2 else truth
            if lit is not None and lit.dim() == 4 and lit.shape[1] == 1:
                lit = lit[:, 0]
            if lit is not None and lit.dim() == 3 and lit.shape[0] != 1:
                lit = lit.amax(0, keepdim=True)                # lit where any plane is
            elif lit is not None and lit.dim() == 2:
                lit = lit[None]
        if scores.dim() != 4 or scores.shape[1] != self.num_classes:
            raise ValueError("TemperatureFit.add: scores must be [N, %d, H, W] (got %s)" % (self.num_classes, tuple(scores.shape)))
        N, _, H, W = scores.shape
        if lit is not None and lit.dim() == 4 and lit.shape[1] == 1:
            lit = lit[:, 0]
        if tuple(truth.shape) != (N, H, W):
            raise ValueError("TemperatureFit.add: truth must be %s (got %s)" % ((N, H, W), tuple(truth.shape)))
        if lit is not None and (lit.dtype != torch.float32 or tuple(lit.shape) != (N, H, W)):
            raise ValueError("TemperatureFit.add: lit must be float32 %s or [N, 1, H, W] (got %s %s)" % ((N, H, W), lit.dtype, tuple(lit.shape)))
        if N > _calib.MAX_IMAGES:
            raise ValueError("TemperatureFit.add: %d images are more than %d" % (N, _calib.MAX_IMAGES))
        return scores, truth, lit

    def _group_list(self, N, groups):
        if groups is None:
            if self.groups == 1:
                return (0,) * N
            if self.groups == N:
                return tuple(range(N))
            raise ValueError("TemperatureFit.add: %d groups and %d images: say which group each image is" % (self.groups, N))
        groups = tuple(int(v) for v in groups)
        if len(groups) != N or any(not 0 <= v < self.groups for v in groups):
            raise ValueError("TemperatureFit.add: groups must be %d indices in 0..%d (got %r)" % (N, self.groups - 1, groups))
        return groups

    def add(self, scores, truth, lit=None, groups=None):
        """one ubf_accumulate call on the current stream, no read-back.  `scores` float32 [N, C, H, W] (a training batch, or what
        WholeViewSegmenter(output="scores") returns) or the stacked [C, rows, cols]; `truth` uint8 or int64 [N, H, W]; `lit` the
        ADC image, float32 [N, H, W] or [N, 1, H, W] (None, or adc_threshold None: every pixel counts); `groups` the group of
        each image (None: image n is group n when there are N groups, group 0 when there is one)."""
        import torch
        scores, truth, lit = self._shapes(scores, truth, lit)
        N, Cn, H, W = scores.shape
        glist = self._group_list(N, groups)
        if not scores.is_cuda:
            raise RuntimeError("TemperatureFit.add: scores must be on a CUDA device; there is no CPU fallback")
        dev = scores.device
        if truth.device != dev or (lit is not None and lit.device != dev):
            raise ValueError("TemperatureFit.add: scores, truth and lit must be on one device")
        if self._table is not None and self._table.device != dev:
            raise ValueError("TemperatureFit.add: the table is on %s, the scores on %s" % (self._table.device, dev))
        if self.adc_threshold is None:
            lit = None
        scores, truth = scores.contiguous(), truth.contiguous()
        lit = lit.contiguous() if lit is not None else None
        K = len(self.temps)
        with torch.cuda.device(dev):
            if self._table is None:
                self._table = torch.zeros((self.groups, K, 3), dtype=torch.float64, device=dev)
                self._counters = torch.zeros((self.groups, 3), dtype=torch.int64, device=dev)
                self._betas = torch.from_numpy(self.betas).to(dev)
            if glist not in self._groups:
                self._groups[glist] = torch.tensor(glist, dtype=torch.uint8).to(dev)
            need = _calib.scratch_bytes(N, H, W, K)
            if self._scratch is None or self._scratch.numel() * 8 < need:
                self._scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
            _calib.accumulate(scores.data_ptr(), truth.data_ptr(), _calib.TRUTH_U8 if truth.dtype == torch.uint8 else _calib.TRUTH_I64,
                              lit.data_ptr() if lit is not None else None, self.adc_threshold if lit is not None else 0.0,
                              self._groups[glist].data_ptr(), self._betas.data_ptr(), K, N, Cn, H, W, self.groups,
                              self._table.data_ptr(), self._counters.data_ptr(), self._scratch.data_ptr(), self._scratch.numel() * 8,
                              torch.cuda.current_stream(dev).cuda_stream)
        self.calls += 1

    def read(self) -> Calibration:
        """the sums added since the last reset(), on the host: the one synchronisation"""
        K = len(self.temps)
        if self._table is None:
            return Calibration(self.temps, np.zeros((self.groups, K, 3)), np.zeros((self.groups, 3), dtype=np.uint64))
        return Calibration(self.temps, self._table.cpu().numpy(), self._counters.cpu().numpy().view(np.uint64))

    def reset(self):
        """forget the sums: two memsets on the current stream"""
        if self._table is not None:
            self._table.zero_()
            self._counters.zero_()
        self.calls = 0
