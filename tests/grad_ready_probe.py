"""FinalityProbe: a stand-in for the data-parallel reducer that checks the gradient-ready contract itself.

The backward schedule reports ranges flat[lo:hi] of the flat gradient buffer to model._grad_ready_hook and promises that a
range is FINAL once (a) the compute stream has reached the point of the call -- unless ordered=False -- and (b) every entry
of wait_events has been reached (Engine._stage_notifier, plan.backward).  GradAllReducer._launch all-reduces the range in
place on its own stream at exactly that moment.  The probe waits for exactly the same things on a stream of its own and
copies the range instead of exchanging it; after the pass, a copy that differs from the buffer's final content is a range
that was reported before it was written."""
import torch


def freeze_encoder(m):
    """the mixed pattern: stem, encoder and ASPP-branch BatchNorms frozen (eval mode), everything else training"""
    m.train()
    frozen = []
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d) and (name == "bn1" or name.startswith("enc_layer") or name.startswith("ASPP_layer_enc")):
            mod.eval()
            frozen.append(name)
    return frozen


class FinalityProbe:
    def __init__(self, model):
        self.model = model
        self.stream = None
        self.records = []           # (lo, hi, snapshot taken on the probe stream, flat)
        self.calls = 0
        model._grad_ready_hook = self

    def remove(self):
        self.model._grad_ready_hook = None

    def reset(self):
        self.records = []
        self.calls = 0

    # the reducer's signature (GradAllReducer._hook)
    def __call__(self, flat, lo, hi, wait_events=(), ordered=True):
        self.calls += 1
        if self.stream is None:
            # high priority, as the reducer's exchange stream: a hardware queue of its own, so the copy runs as soon as its
            # waits are satisfied instead of queueing behind the backward kernels
            self.stream = torch.cuda.Stream(device=flat.device, priority=-1)
        if ordered:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(flat.device))
            self.stream.wait_event(ev)
        with torch.cuda.stream(self.stream):
            for e in wait_events:
                if hasattr(e, "wait_on"):
                    e.wait_on(self.stream)          # ubresnet_amd.plan.TapeMark
                else:
                    self.stream.wait_event(e)
            snap = flat[lo:hi].clone()
        self.records.append((lo, hi, snap, flat))

    def ranges(self):
        return [(lo, hi) for lo, hi, _, _ in self.records]

    @staticmethod
    def _bits(t):
        return t.contiguous().view(torch.int32)

    @staticmethod
    def name_at(eng, idx):
        """the parameter whose (padded) slot of the flat buffer holds element idx"""
        best = None
        for name, _ in eng.grad_order:
            o = eng.grad_offsets[name]
            if o <= idx and (best is None or o > eng.grad_offsets[best]):
                best = name
        return best

    def check(self, eng, reference_flat=None, min_ranges=12):
        """call after the backward pass and one torch.cuda.synchronize().  reference_flat: the flat gradient buffer of the
        same pass (same weights, same input, fresh model) run with no hook installed and nothing poisoned"""
        assert self.records, "the hook was never called"
        flat = self.records[0][3]
        # (a) tiling
        assert all(r[3] is flat for r in self.records), "ranges of more than one flat buffer in one pass"
        assert flat is self.model.__dict__["_ubr_flat_grad"], "the reported buffer is not the one the .grad tensors alias"
        rs = self.ranges()
        assert rs[0][0] == 0, "first range starts at %d" % rs[0][0]
        for i, (lo, hi) in enumerate(rs):
            assert hi > lo, "stage %d: empty range [%d, %d)" % (i, lo, hi)
            if i:
                assert lo == rs[i - 1][1], "stage %d starts at %d, stage %d ended at %d" % (i, lo, i - 1, rs[i - 1][1])
        assert rs[-1][1] == flat.numel() == eng.grad_numel, "last range ends at %d of %d" % (rs[-1][1], flat.numel())
        assert len(rs) >= min_ranges, "%d ranges reported, expected at least %d" % (len(rs), min_ranges)
        # (b) finality, bit for bit (NaN payloads included)
        for i, (lo, hi, snap, _) in enumerate(self.records):
            diff = self._bits(snap) != self._bits(flat[lo:hi])
            if diff.any():
                first = lo + int(diff.nonzero()[0])
                raise AssertionError("stage %d reported flat[%d:%d] before it was final: %d elements changed afterwards, the first "
                                     "at %d in parameter %s" % (i, lo, hi, int(diff.sum()), first, self.name_at(eng, first)))
        # (c) neutrality: watching (and poisoning) changed nothing
        if reference_flat is not None:
            assert reference_flat.numel() == flat.numel()
            diff = self._bits(reference_flat) != self._bits(flat)
            if diff.any():
                first = int(diff.nonzero()[0])
                raise AssertionError("the probed pass differs from the unprobed one in %d elements, the first at %d in parameter %s "
                                     "(%r vs %r)" % (int(diff.sum()), first, self.name_at(eng, first),
                                                     float(flat[first]), float(reference_flat[first])))
        return rs
