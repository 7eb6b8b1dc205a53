"""Score event products against a labelled event, on the device: what ``caffe/analyze_accuracy.py`` of the reference set out to do
("Calculates basic accuracy metrics. To-do: expand to include designation of ambiguous label. This is if shower is on trunk of
cosmic muon.") and left a stub.

``metrics.confusion_matrix`` scores dense float32 crops over every pixel, and crops are 97-99 % background.  ``EventScorer`` reads
what deployment produces -- ``deploy.Products``: a class map and a float16 confidence where the wire is lit -- and a truth image,
and counts over the LIT pixels only, per plane, with one ``ubq_score_event`` launch per event (libubresnet_score.so,
include/ubresnet_score.h):

* a confusion matrix per stratum: *interface* pixels are those of a class ``>= interface_from`` with a different class
  ``>= interface_from`` inside the ``(2 radius + 1)^2`` window of the truth image (the contact rule of ``PixelWeights``; with
  ``interface_from=1`` the reference's "shower on the trunk of a muon"), *clear* pixels are the rest;
* a reliability table of the confidence: per bin the pixels, the correct ones and the sum of their confidence in units of 2^-24;
* four tallies: scored, ignored (lit with a truth or label that is no class), dark signal (truth >= 1 where the threshold hid the
  pixel from the network's score) and non-finite confidences.

    scorer = EventScorer(num_classes=4, planes=3, bins=10, radius=2, interface_from=1)
    for view, truth in events:
        scorer.add(segmenter(view), truth)      # one launch on the current stream; nothing is read back
    print(scorer.read())                        # the one host sync

Everything is integer arithmetic: a Score is reproducible bit for bit; tests/score_ref.py is the numpy statement of the rule.
There is no fallback: a missing library is a RuntimeError.
"""
from __future__ import annotations

import struct

import numpy as np

from . import _score

__all__ = ["EventScorer", "Score", "half_bits", "equal_width_edges"]

STRATA = ("clear", "interface")
TALLIES = ("scored", "ignored", "dark", "nonfinite")


def half_bits(x: float) -> int:
    """the IEEE half nearest to x (round to nearest even), as its bit pattern"""
    with np.errstate(over="ignore"):
        return int(np.float16(x).view(np.uint16))


def _half_value(bits: int) -> float:
    return struct.unpack("<e", struct.pack("<H", bits))[0]


def equal_width_edges(bins: int):
    """the inner edges of `bins` equal-width bins on [0, 1], rounded to half; two edges that round to one half are a ValueError"""
    edges = [half_bits(i / float(bins)) for i in range(1, bins)]
    if len(set(edges)) != len(edges):
        raise ValueError("EventScorer: %d equal-width bins have duplicate edges in half precision" % bins)
    return edges


def _int(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("EventScorer: %s must be an int (got %r)" % (name, v))
    if not lo <= v <= hi:
        raise ValueError("EventScorer: %s must be %d..%d (got %d)" % (name, lo, hi, v))
    return int(v)


def _edges(bins):
    if isinstance(bins, (int, np.integer)) and not isinstance(bins, bool):
        return equal_width_edges(_int("bins", bins, 1, _score.MAX_BINS))
    try:
        values = [float(v) for v in bins]
    except (TypeError, ValueError):
        raise ValueError("EventScorer: bins must be an int or a sequence of inner edges (got %r)" % (bins,))
    if len(values) + 1 > _score.MAX_BINS:
        raise ValueError("EventScorer: %d edges make more than %d bins" % (len(values), _score.MAX_BINS))
    edges = []
    for v in values:
        if not (v > 0.0 and v < float("inf")):
            raise ValueError("EventScorer: an edge must be positive and finite (got %r)" % v)
        h = half_bits(v)
        if not 0x0001 <= h <= 0x7BFF:
            raise ValueError("EventScorer: edge %r is not a positive finite half" % v)
        edges.append(h)
    if any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError("EventScorer: the edges must be strictly ascending in half precision (got %r)" % (values,))
    return edges


class Score(object):
    """What EventScorer.read() returns: the tables of `events` events on the host.  `tables` is uint64 [events, words] as the
    device wrote it; `total` the same summed over the events in Python ints (no wrap)."""

    def __init__(self, tables, planes, num_classes, edges):
        self.tables = np.ascontiguousarray(tables, dtype=np.uint64)
        self.events = self.tables.shape[0]
        self.planes, self.num_classes, self.edges = planes, num_classes, list(edges)
        self.bins = len(self.edges) + 1
        words = planes * (2 * num_classes * num_classes + 6 * self.bins + 4)
        if self.tables.ndim != 2 or self.tables.shape[1] != words:
            raise ValueError("Score: expected [events, %d] words, got %s" % (words, self.tables.shape))
        self.total = self.tables.astype(object).sum(axis=0) if self.events else np.zeros(words, dtype=object)

    def _parts(self, flat):
        P, Cn, B = self.planes, self.num_classes, self.bins
        t = np.asarray(flat).reshape(P, -1)
        cw = 2 * Cn * Cn
        return t[:, :cw].reshape(P, 2, Cn, Cn), t[:, cw:cw + 6 * B].reshape(P, 2, B, 3), t[:, cw + 6 * B:]

    def _select(self, part, stratum, plane):
        """sum `part` [P, 2, ...] over the planes and strata that are not named"""
        if stratum is not None:
            if stratum not in STRATA and stratum not in (0, 1):
                raise ValueError("Score: stratum must be None, 'clear' / 0 or 'interface' / 1 (got %r)" % (stratum,))
            s = STRATA.index(stratum) if stratum in STRATA else int(stratum)
            part = part[:, s:s + 1]
        if plane is not None:
            if not 0 <= plane < self.planes:
                raise ValueError("Score: plane must be None or 0..%d (got %r)" % (self.planes - 1, plane))
            part = part[plane:plane + 1]
        return part.sum(axis=(0, 1))

    def event(self, n):
        """(conf [P,2,C,C], rel [P,2,bins,3], tally [P,4]) of event n, uint64"""
        return self._parts(self.tables[n])

    def confusion(self, stratum=None, plane=None):
        """int64 [C, C] counts [truth, label] over the lit, scored pixels of every event"""
        import torch
        cm = self._select(self._parts(self.total)[0], stratum, plane)
        return torch.from_numpy(cm.astype(np.int64))

    def accuracy(self, track_shower=True, stratum=None, plane=None):
        """metrics.accuracy_from_confusion of confusion(): per-class recall in percent, the total, and the track/shower figure"""
        from . import metrics
        return metrics.accuracy_from_confusion(self.confusion(stratum, plane), track_shower=track_shower)

    def iou(self, stratum=None, plane=None):
        from . import metrics
        return metrics.iou(self.confusion(stratum, plane))

    def reliability(self, stratum=None, plane=None):
        """per confidence bin: dict of `low`, `high` (the bin's edges as floats; the last bin is open), `pixels`, `correct`,
        `confidence_sum` (Python ints, the last in units of 2^-24), `accuracy` and `mean_confidence` (float64, nan when empty)"""
        rel = self._select(self._parts(self.total)[1], stratum, plane)
        lows = [0.0] + [_half_value(e) for e in self.edges]
        highs = lows[1:] + [float("inf")]
        n = [int(v) for v in rel[:, 0]]
        c = [int(v) for v in rel[:, 1]]
        f = [int(v) for v in rel[:, 2]]
        nan = float("nan")
        return dict(low=lows, high=highs, pixels=n, correct=c, confidence_sum=f,
                    accuracy=np.array([ci / ni if ni else nan for ci, ni in zip(c, n)], dtype=np.float64),
                    mean_confidence=np.array([fi / (2.0 ** 24 * ni) if ni else nan for fi, ni in zip(f, n)], dtype=np.float64))

    def ece(self, stratum=None, plane=None):
        """expected calibration error: sum_b n_b / N * |correct_b / n_b - sum_b / (2^24 n_b)| in float64; nan without pixels"""
        r = self.reliability(stratum, plane)
        total = sum(r["pixels"])
        if total == 0:
            return float("nan")
        return float(sum(n / total * abs(c / n - f / (2.0 ** 24 * n))
                         for n, c, f in zip(r["pixels"], r["correct"], r["confidence_sum"]) if n))

    def tallies(self, plane=None):
        t = self._parts(self.total)[2]
        t = t[plane] if plane is not None else t.sum(axis=0)
        return dict((k, int(v)) for k, v in zip(TALLIES, t))

    def __str__(self):
        Cn = self.num_classes
        ts = Cn >= 3
        t = self.tallies()
        lines = ["%d event%s, %d plane%s: %d lit pixels scored, %d ignored, %d dark signal pixels, %d non-finite confidences"
                 % (self.events, "" if self.events == 1 else "s", self.planes, "" if self.planes == 1 else "s",
                    t["scored"], t["ignored"], t["dark"], t["nonfinite"])]
        head = "%-10s %10s " % ("stratum", "pixels") + " ".join("%8s" % ("Acc[%d]" % c) for c in range(Cn)) + " %8s" % "total"
        head += (" %8s" % "trk/shw" if ts else "") + " " + " ".join("%7s" % ("IoU[%d]" % c) for c in range(Cn)) + " %7s" % "ECE"
        lines.append(head)
        for name, s in (("lit", None), ("clear", 0), ("interface", 1)):
            acc = self.accuracy(track_shower=ts, stratum=s)
            row = "%-10s %10d " % (name, int(self.confusion(s).sum())) + " ".join("%8.3f" % a for a in acc)
            row += " " + " ".join("%7.4f" % v for v in self.iou(stratum=s)) + " %7.4f" % self.ece(stratum=s)
            lines.append(row)
        lines.append("confusion over the lit pixels [truth, label]:")
        for row in self.confusion().tolist():
            lines.append("  " + " ".join("%10d" % v for v in row))
        r = self.reliability()
        lines.append("%-19s %10s %9s %9s" % ("confidence bin", "pixels", "accuracy", "mean conf"))
        for lo, hi, n, a, m in zip(r["low"], r["high"], r["pixels"], r["accuracy"], r["mean_confidence"]):
            lines.append("[%7.4f, %7.4f)  %10d %9.4f %9.4f" % (lo, hi, n, a, m))
        return "\n".join(lines)


class EventScorer(object):
    """A device table of `capacity` events' scores; see the module docstring.  `bins`: an int for that many equal-width bins on
    [0, 1], or a sequence of floats, the inner edges.  Arguments are checked here, before anything touches the device; the
    table is allocated, and zeroed with one memset, by the first add()."""

    def __init__(self, num_classes=4, planes=3, bins=10, radius=2, interface_from=1, fill_label=255, capacity=64, device="cuda"):
        self.num_classes = _int("num_classes", num_classes, 1, _score.MAX_CLASSES)
        self.planes = _int("planes", planes, 1, 65535)
        self.edges = _edges(bins)
        self.bins = len(self.edges) + 1
        self.radius = _int("radius", radius, 0, _score.MAX_RADIUS)
        self.interface_from = _int("interface_from", interface_from, 0, self.num_classes)
        self.fill_label = _int("fill_label", fill_label, 0, 255)
        self.capacity = _int("capacity", capacity, 1, 1 << 20)
        self.words = self.planes * (2 * self.num_classes ** 2 + 6 * self.bins + 4)
        if self.words >= 1 << 31:
            raise ValueError("EventScorer: a table of %d words does not fit an int" % self.words)
        self.device = device
        self._edges_c = _score.edges_array(self.edges)
        self._table = None
        self.events = 0

    def _check(self, products, truth):
        import torch
        try:
            label, confidence = products[0], products[1]
        except (TypeError, IndexError):
            raise ValueError("EventScorer.add: products must be deploy.Products or (label, confidence)")
        for name, t in (("label", label), ("confidence", confidence), ("truth", truth)):
            if not isinstance(t, torch.Tensor):
                raise ValueError("EventScorer.add: %s must be a tensor (got %s)" % (name, type(t).__name__))
        if label.dtype != torch.uint8 or confidence.dtype != torch.float16:
            raise ValueError("EventScorer.add: label must be uint8 and confidence float16 (got %s, %s)" % (label.dtype, confidence.dtype))
        if truth.dtype not in (torch.uint8, torch.int64):
            raise ValueError("EventScorer.add: truth must be uint8 or int64 (got %s)" % truth.dtype)
        if self.planes == 1 and label.dim() == 2:             # the products of a stacked model: one [rows, cols] map per event
            label, confidence = label[None], confidence[None]
            truth = truth[None] if truth.dim() == 2 else truth
        if label.dim() != 3 or label.shape[0] != self.planes:
            raise ValueError("EventScorer.add: label must be [%d, rows, cols] (got %s)" % (self.planes, tuple(label.shape)))
        if confidence.shape != label.shape or truth.shape != label.shape:
            raise ValueError("EventScorer.add: label %s, confidence %s and truth %s differ in shape"
                             % (tuple(label.shape), tuple(confidence.shape), tuple(truth.shape)))
        if not (label.is_cuda and confidence.device == label.device and truth.device == label.device):
            raise ValueError("EventScorer.add: label, confidence and truth must be on one CUDA device (got %s, %s, %s)"
                             % (label.device, confidence.device, truth.device))
        if self._table is not None and self._table.device != label.device:
            raise ValueError("EventScorer.add: the table is on %s, the products on %s" % (self._table.device, label.device))
        if self._table is None and torch.device(self.device).index not in (None, label.device.index):
            raise ValueError("EventScorer.add: the scorer was made for %s, the products are on %s" % (self.device, label.device))
        return label.contiguous(), confidence.contiguous(), truth.contiguous()

    def add(self, products, truth):
        """score one event into the next row of the table: one launch on the current stream, no read-back"""
        import torch
        label, confidence, truth = self._check(products, truth)
        if self.events >= self.capacity:
            raise RuntimeError("EventScorer.add: the table is full (capacity %d); read() and reset()" % self.capacity)
        with torch.cuda.device(label.device):
            if self._table is None:
                if _score.table_words(self.planes, self.num_classes, self.bins) != self.words:
                    raise RuntimeError("EventScorer: the library counts another table size than %d words" % self.words)
                self._table = torch.empty((self.capacity, self.words), dtype=torch.int64, device=label.device)
                self._table.zero_()                           # one memset on the current stream
            row = self._table[self.events]
            _score.score_event(label.data_ptr(), confidence.data_ptr(), truth.data_ptr(),
                               _score.TRUTH_U8 if truth.dtype == torch.uint8 else _score.TRUTH_I64,
                               self.num_classes, self.fill_label, self.radius, self.interface_from, self._edges_c, self.bins,
                               row.data_ptr(), self.planes, label.shape[1], label.shape[2],
                               torch.cuda.current_stream(label.device).cuda_stream)
        self.events += 1

    def read(self) -> Score:
        """the events added since the last reset(), on the host: the one synchronisation"""
        if self._table is None or self.events == 0:
            tables = np.zeros((0, self.words), dtype=np.uint64)
        else:
            tables = self._table[:self.events].cpu().numpy().view(np.uint64)
        return Score(tables, self.planes, self.num_classes, self.edges)

    def reset(self):
        """forget the events: one memset on the current stream"""
        if self._table is not None:
            self._table.zero_()
        self.events = 0
