#!/usr/bin/env python3
"""Record of what ubresnet_amd/deploy.py puts on the stream, per configuration of WholeViewSegmenter and segment_crops: every call
of ubr_crop_tiles, ubr_stitch_tiles and of the launching ubp_ / ubt_ / ubv_ / ubf_ / ubz_ entry points, every CUDAGraph.replay and
every eager forward, in issue order, with all integer and float arguments.  The kernels have exact tests of their own; this pins
WHICH launches a deployment call issues, with which arguments and on which buffers.

  * The seam is `BINDING._lib` of the six binding modules (_lib, _post, _tta, _blend, _calib, _sparse): a recording proxy stands
    there while a call is recorded.  Entry points that return a size and launch nothing (ubz_compact_scratch_bytes,
    ubf_scratch_bytes) and <prefix>_last_error / _version are passed through unrecorded.
  * A device address is replaced by "p<k>", k counting the distinct addresses in the order of their first appearance within the
    one call -- which buffer the crop writes, that the rescale works in place, that a kept buffer is the one the sink reads,
    without the address.  The stream is an address like any other (null: the default stream).  So that a number always means one
    buffer, every tensor a recorded forward returns is kept alive until the call ends, and a SparseEvent is given on the device.
  * A host descriptor array is recorded by content.
  * A forward is the entry ["forward", input, shape, output] (WholeViewSegmenter._forward_batch, or the model that segment_crops
    calls); a replay is ["graph.replay"].
  * Every configuration is first called once unrecorded: that call builds what is built once (weight packing, the warm-up forward,
    the graph capture).  Then it is called twice, recorded; the two traces must be equal, the buffers being reused.
  * The SHA-256 of every tensor the call returned goes beside the traces (a pixel list: its defined head).

A change that must alter neither launches nor results (a refactor of deploy.py) is checked by running this in a checkout of each
commit -- copy this file into the older one -- and comparing; two runs of ONE commit show what reproduces at all.
tests/golden/deploy_launches.json holds the traces alone, so a kernel change does not invalidate it.

    python tools/deploy_trace.py OUT.json [--fixture]           --fixture: also write tests/golden/deploy_launches.json
    python tools/deploy_trace.py --compare A.json B.json        exit 1 and the names if a trace or a hash differs"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "deploy_launches.json")
BINDINGS = ("_lib", "_post", "_tta", "_blend", "_calib", "_sparse")
ROWS, COLS, PLANES, TILE, THRESHOLD = 96, 160, 3, (64, 96), 10.0
_ALL = dict(tta=("rows", "cols", "both"), margin=8, blend="hann", temperature=(0.8, 1.0, 1.3))

# UResNet (ip16, 3 classes): 3 x 1 x 96 x 160 in tiles of 64 x 96 is 2 x 2 origins per plane with overlap in both axes, 12 tiles
# in chunks of 5, 5, 2.  ASPP_ResNet (the planes stacked as channels): 3 x 1 x 64 x 160 is 2 tiles, one partial chunk of batch 3.
SEGMENTER = [
    ("seg/01-scores", "uresnet", dict()),
    ("seg/02-products", "uresnet", dict(output="products")),
    ("seg/03-pixels", "uresnet", dict(output="pixels")),
    ("seg/04-scores-sparse", "uresnet", dict(sparse=True)),
    ("seg/05-scores-tta-cols", "uresnet", dict(tta=("cols",))),
    ("seg/06-products-tta-all", "uresnet", dict(output="products", tta=("rows", "cols", "both"))),
    ("seg/07-scores-margin", "uresnet", dict(margin=8)),
    ("seg/08-scores-linear", "uresnet", dict(margin=8, blend="linear")),
    ("seg/09-products-hann", "uresnet", dict(output="products", margin=8, blend="hann")),
    ("seg/10-scores-temperature", "uresnet", dict(temperature=(0.8, 1.0, 1.3))),
    ("seg/11-products-all", "uresnet", dict(output="products", **_ALL)),
    ("seg/12-pixels-sparse-all", "uresnet", dict(output="pixels", sparse=True, capacity=100, **_ALL)),
    ("seg/13-scores-eager", "uresnet", dict(use_graph=False)),
    ("seg/14-aspp-scores", "aspp", dict()),
    ("seg/15-aspp-products-tta-rows", "aspp", dict(output="products", tta=("rows",))),
]
# segment_crops: 5 crops of 1 x 64 x 96 in batches of 2, 2, 1
CROPS = [("crops/%s%s%s" % (output, "-tta" if tta else "", "-temperature" if temperature else ""),
          dict(output=output, tta=tta, temperature=temperature))
         for output in ("scores", "products") for tta in (None, ("rows", "both")) for temperature in (None, 1.3)]
IDS = [c[0] for c in SEGMENTER] + [c[0] for c in CROPS]


class Recorder:
    """the entries of one call; begin() starts the next one"""

    def __init__(self):
        self.begin()

    def begin(self):
        self.entries, self._ids, self._alive = [], {}, []

    def ptr(self, address):
        if not address:
            return None
        return "p%d" % self._ids.setdefault(int(address), len(self._ids))

    def launch(self, name, argtypes, args):
        row = [name]
        for kind, v in zip(argtypes, args):
            if kind is C.c_void_p:
                row.append(self.ptr(v))
            elif isinstance(v, C.Array):
                row.append(list(v))
            elif kind in (C.c_float, C.c_double):
                row.append(float(v))
            else:
                row.append(int(v))
        self.entries.append(row)

    def forward(self, fn, x):
        y = fn(x)
        self._alive.append(y)
        self.entries.append(["forward", self.ptr(x.data_ptr()), list(x.shape), self.ptr(y.data_ptr())])
        return y


class _Proxy:
    """stands at BINDING._lib: the launching entry points are recorded on their way through, everything else is the library's"""

    def __init__(self, binding, lib, rec):
        self._binding, self._lib, self._rec = binding, lib, rec

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        restype, argtypes = self._binding.table.get(name, (None, None))
        launches = restype is C.c_int and not name.endswith("_version")
        if self._binding.prefix == "ubr":
            launches = name in ("ubr_crop_tiles", "ubr_stitch_tiles")
        if not launches:
            return fn

        def call(*args):
            self._rec.launch(name, argtypes, args)
            return fn(*args)
        return call


@contextlib.contextmanager
def recording(rec, seg=None, model=None):
    """`rec` sees the six libraries, CUDAGraph.replay and the forwards of `seg` (_forward_batch) or of `model`"""
    import importlib
    import torch
    bindings = [importlib.import_module("ubresnet_amd." + b).BINDING for b in BINDINGS]
    libs = [b.lib() for b in bindings]
    replay = torch.cuda.CUDAGraph.replay

    def recorded_replay(graph):
        rec.entries.append(["graph.replay"])
        return replay(graph)
    owner = seg if seg is not None else model
    attr = "_forward_batch" if seg is not None else "forward"
    inner = getattr(owner, attr)
    try:
        for b, l in zip(bindings, libs):
            b._lib = _Proxy(b, l, rec)
        torch.cuda.CUDAGraph.replay = recorded_replay
        setattr(owner, attr, lambda x: rec.forward(inner, x))       # an instance attribute in front of the class's method
        yield rec
    finally:
        delattr(owner, attr)
        torch.cuda.CUDAGraph.replay = replay
        for b, l in zip(bindings, libs):
            b._lib = l


_CACHE = {}


def _model(arch):
    from oracle import uresnet_oracle as O
    from ubresnet_amd import deploy
    if arch not in _CACHE:
        if arch == "uresnet":
            sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
            _CACHE[arch] = deploy.load_model(None, "cuda:0", num_classes=3, state_dict=sd)
        else:
            sd = O.seeded_state_dict(O.aspp_resnet_schema(3, 3, 16), 42)
            _CACHE[arch] = deploy.load_model(None, "cuda:0", num_classes=3, input_channels=3, state_dict=sd, arch="aspp")
    return _CACHE[arch]


def _view(n, rows, cols, seed):
    """a tenth of the pixels carry charge, as on a wire plane, most of it above the threshold of the lit test"""
    import numpy as np
    import torch
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.rand(n, 1, rows, cols) * (rs.rand(n, 1, rows, cols) > 0.9) * 100.0).astype(np.float32)).cuda()


def _tensors(result, extra=None):
    """{name: tensor} of what a call returned"""
    import torch
    from ubresnet_amd import sparse
    if isinstance(result, torch.Tensor):
        out = {"scores": result}
    elif isinstance(result, sparse.PixelList):
        head = min(int(result.count.item()), result.capacity)
        out = {"index": result.index[:head], "label": result.label[:head], "confidence": result.confidence[:head],
               "count": result.count, "counts": result.counts}
    else:
        out = dict(zip(("label", "confidence", "counts"), result))
    if extra is not None:
        out["status"] = extra
    return out


def _sha(t):
    import torch
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def record(case_id):
    """-> (traces of the two recorded calls, {tensor name: sha256} of the second call's result)"""
    import torch
    from ubresnet_amd import deploy, sparse
    rec = Recorder()
    traces = []
    if case_id.startswith("seg/"):
        _, arch, kw = SEGMENTER[[c[0] for c in SEGMENTER].index(case_id)]
        kw = dict(kw)
        rows = 64 if arch == "aspp" else ROWS
        view = _view(PLANES, rows, COLS, 21)
        if kw.pop("sparse", False):
            ev = sparse.SparseEvent.from_dense(view.cpu())
            view = sparse.SparseEvent(ev.index.cuda(), ev.value.cuda(), PLANES, rows, COLS)
        seg = deploy.WholeViewSegmenter(_model(arch), rows, COLS, planes=PLANES, tile=TILE, batch=3 if arch == "aspp" else 5,
                                        adc_threshold=THRESHOLD, **kw)
        seg(view)
        for _ in range(2):
            with recording(rec, seg=seg):
                rec.begin()
                result = seg(view)
                traces.append(rec.entries)
        tensors = _tensors(result, seg.status)
    else:
        kw = dict(CROPS)[case_id]
        model, crops = _model("uresnet"), _view(5, 64, 96, 22)
        deploy.segment_crops(model, crops, batch=2, adc_threshold=THRESHOLD, **kw)
        for _ in range(2):
            with recording(rec, model=model):
                rec.begin()
                result = deploy.segment_crops(model, crops, batch=2, adc_threshold=THRESHOLD, **kw)
                traces.append(rec.entries)
        tensors = _tensors(result)
    torch.cuda.synchronize()
    hashes = {n: _sha(t) for n, t in tensors.items()}
    rec.begin()
    return traces, hashes


def first_difference(want, got, what):
    """None, or where two traces part"""
    for i, (a, b) in enumerate(zip(want, got)):
        if a != b:
            return "%s: entry %d is %s, expected %s" % (what, i, json.dumps(b), json.dumps(a))
    if len(want) != len(got):
        return "%s: %d entries, expected %d" % (what, len(got), len(want))
    return None


def load(path=FIXTURE):
    with open(path) as f:
        return json.load(f)


def dump(traces, path):
    """one entry per line, so that a changed launch is one changed line"""
    with open(path, "w") as f:
        f.write("{\n")
        for k, (case_id, entries) in enumerate(traces.items()):
            f.write("%s: [\n" % json.dumps(case_id))
            f.write(",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in entries))
            f.write("\n]%s\n" % ("," if k + 1 < len(traces) else ""))
        f.write("}\n")


def compare(pa, pb):
    a, b = load(pa), load(pb)
    ids = sorted(set(a["traces"]) | set(b["traces"]))
    bad_traces = [k for k in ids if a["traces"].get(k) != b["traces"].get(k)]
    for k in bad_traces:
        print("TRACE DIFFERS %s" % first_difference(a["traces"].get(k, []), b["traces"].get(k, []), k))
    bad = [(k, t) for k in ids for t in sorted(set(a["hashes"].get(k, {})) | set(b["hashes"].get(k, {})))
           if a["hashes"].get(k, {}).get(t) != b["hashes"].get(k, {}).get(t)]
    for k, t in bad:
        print("HASH DIFFERS %s %s" % (k, t))
    print("%s vs %s: %d of %d traces differ (%d launches), %d of %d result tensors differ"
          % (pa, pb, len(bad_traces), len(ids), sum(len(v) for v in a["traces"].values()), len(bad),
             sum(len(v) for v in a["hashes"].values())))
    return 1 if bad_traces or bad else 0


def main(out, fixture):
    sys.path.insert(0, ROOT)
    res = {"traces": {}, "hashes": {}}
    for case_id in IDS:
        (first, second), res["hashes"][case_id] = record(case_id)
        diff = first_difference(first, second, case_id + ", second call")
        assert diff is None, diff
        res["traces"][case_id] = first
    with open(out, "w") as f:
        json.dump(res, f)
    if fixture:
        dump(res["traces"], FIXTURE)
    print("wrote %s: %d configurations, %d launches, %d result tensors" % (out, len(IDS), sum(len(v) for v in res["traces"].values()),
                                                                          sum(len(v) for v in res["hashes"].values())))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) not in (2, 3) or (len(sys.argv) == 3 and sys.argv[2] != "--fixture"):
        sys.exit(__doc__)
    main(sys.argv[1], len(sys.argv) == 3)
