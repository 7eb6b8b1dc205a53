#!/usr/bin/env python3
"""Launch schedule of the graph executor at the smallest shapes that still reach every stage: what the forward and backward
tapes of each case hold -- tape size, every labelled operator call (op, kernel symbol, shape signature) in issue order, the
launches each call put on the tape, and the backward's hand-over stages.  Needs a GPU.

    python tests/golden/schedule/make_schedule.py             rewrite schedule.json (after a DELIBERATE schedule change)
    python tests/golden/schedule/make_schedule.py --check     compare against schedule.json, print the first difference

tests/test_gpu_schedule.py loads this file and compares the same records.  Only the executor's public surface is used
(model call, Engine._planned, Recording.labels / launches_per_operator / stages), so the script runs unchanged on older
checkouts."""
import contextlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
FIXTURE = os.path.join(HERE, "schedule.json")

DTYPES = {"bf16": "bfloat16", "f16": "float16", "fp32": "float32"}

# mode: train = every BatchNorm on batch statistics; frozen = model.eval(), gradients on (every tail one-pass);
#       mixed = train except enc_layer2.res1.bnpass (one block tail with its two sites in different modes);
#       infer = model.eval() under no_grad (fold: the folded inference schedule, or the training schedule without saving)
CASES = [
    dict(id="uresnet-bf16-train", net="uresnet", shape=(2, 1, 64, 64), dtype="bf16", mode="train"),
    dict(id="uresnet-fp32-train", net="uresnet", shape=(2, 1, 64, 64), dtype="fp32", mode="train"),
    dict(id="uresnet-bf16-frozen", net="uresnet", shape=(2, 1, 64, 64), dtype="bf16", mode="frozen"),
    dict(id="uresnet-bf16-mixed", net="uresnet", shape=(2, 1, 64, 64), dtype="bf16", mode="mixed"),
    dict(id="uresnet-f16-infer-folded", net="uresnet", shape=(2, 1, 64, 64), dtype="f16", mode="infer", fold=True),
    dict(id="uresnet-f16-infer-unfolded", net="uresnet", shape=(2, 1, 64, 64), dtype="f16", mode="infer", fold=False),
    dict(id="aspp-bf16-train", net="aspp", shape=(1, 3, 64, 96), dtype="bf16", mode="train"),
    dict(id="aspp-f16-infer-folded", net="aspp", shape=(1, 3, 64, 96), dtype="f16", mode="infer", fold=True),
]


def build(case):
    """-> (model on cuda:0 in the case's mode, image, labels, pixel weights)"""
    import torch
    from oracle import uresnet_oracle as O
    from ubresnet_amd import synthetic
    N, Cin, H, W = case["shape"]
    if case["net"] == "uresnet":
        from ubresnet_amd.models.ub_uresnet import UResNet
        m = UResNet(3, Cin, 16)
        m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, Cin, 16, 16), 42))
    else:
        from ubresnet_amd.models.ASPP_ResNet import ASPP_ResNet
        m = ASPP_ResNet(3, Cin, 16, False)
        m.load_state_dict(O.seeded_state_dict(O.aspp_resnet_schema(3, Cin, 16), 44))
    m = m.cuda().train()
    m.compute_dtype = getattr(torch, DTYPES[case["dtype"]])
    if case["mode"] in ("frozen", "infer"):
        m.eval()
    elif case["mode"] == "mixed":
        m.enc_layer2.res1.bnpass.eval()
    x, lab, wgt = synthetic.make_batch(N, H, W, 1000, planes=Cin)
    return m, torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(wgt).cuda()


@contextlib.contextmanager
def infer_fold(case):
    """the unfolded inference case runs with engine._INFER_FOLD off"""
    from ubresnet_amd import engine
    old = engine._INFER_FOLD
    engine._INFER_FOLD = case.get("fold", True)
    try:
        yield
    finally:
        engine._INFER_FOLD = old


def run_pass(case, m, x, lab, wgt):
    """one pass of the case: a train step without the optimizer, or a no-grad forward.  -> log-probabilities"""
    import torch
    if case["mode"] == "infer":
        with torch.no_grad():
            out = m(x)
    else:
        from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
        m.zero_grad()
        out = m(x)
        PixelWiseNLLLoss()(out, lab, wgt).backward()
    torch.cuda.synchronize()
    return out.detach()


def _tape(rec, streams, backward):
    d = {"size": rec.tape.size(),
         "calls": [None if meta is None else list(meta[:3]) for meta in rec.labels],
         "launches": rec.launches_per_operator(streams[:rec.nstreams])}
    if backward:
        d["stages"] = [[lo, hi, m1 is not None] for lo, hi, m0, m1 in rec.stages]
    return d


def schedule(case, m):
    """the record of a case whose two passes (record, replay) have run on m"""
    import torch
    eng = m.__dict__["_ubr_engine"]
    assert len(eng._planned) == 1, "expected one launch plan, got %d" % len(eng._planned)
    (key, plan), = eng._planned.items()
    shape, dt, training, frozen, save = key[:5]
    streams = [torch.cuda.current_stream().cuda_stream] + ([eng.side.cuda_stream] if eng.side is not None else [])
    rec = {"case": {"net": case["net"], "shape": list(shape), "dtype": str(dt), "training": training,
                    "frozen": [int(f) for f in frozen], "save": save, "infer_fold": case.get("fold", True)},
           "forward": _tape(plan.fwd, streams, False)}
    if case["mode"] != "infer":
        assert plan.bwd is not None and plan.uses == 2, "the backward tape was not recorded / replayed"
        rec["backward"] = _tape(plan.bwd, streams, True)
    torch.cuda.synchronize()
    return rec


def record(case):
    m, x, lab, wgt = build(case)
    with infer_fold(case):
        run_pass(case, m, x, lab, wgt)       # records the tapes
        run_pass(case, m, x, lab, wgt)       # replays them
        return schedule(case, m)


def first_difference(want, got, path=""):
    """None when equal, else a one-line description of the first place two records differ"""
    if isinstance(want, dict) and isinstance(got, dict):
        for k in want:
            if k not in got:
                return "%s: missing %r" % (path, k)
            d = first_difference(want[k], got[k], "%s/%s" % (path, k))
            if d:
                return d
        extra = [k for k in got if k not in want]
        return "%s: unexpected %r" % (path, extra) if extra else None
    if isinstance(want, list) and isinstance(got, list) and path.rsplit("/", 1)[-1] in ("calls", "launches", "stages"):
        for i, (a, b) in enumerate(zip(want, got)):
            if a != b:
                return "%s[%d]: expected %r, got %r" % (path, i, a, b)
        if len(want) != len(got):
            return "%s: expected %d entries, got %d (first surplus: %r)" % (path, len(want), len(got), (want + got)[min(len(want), len(got))])
        return None
    return None if want == got else "%s: expected %r, got %r" % (path, want, got)


# ---- fixture file: operator calls are interned (a pass repeats few distinct ones), one JSON value per line
def save(records, path=FIXTURE):
    table, index = [], {}

    def intern(tape):
        t = dict(tape)
        out = []
        for c in tape["calls"]:
            k = json.dumps(c)
            if k not in index:
                index[k] = len(table)
                table.append(c)
            out.append(index[k])
        t["calls"] = out
        return t
    packed = {cid: {k: (intern(v) if k in ("forward", "backward") else v) for k, v in r.items()} for cid, r in records.items()}
    js = lambda o: json.dumps(o, separators=(",", ":"))
    lines = ['{"operator_calls":[']
    lines += [js(c) + ("," if i + 1 < len(table) else "") for i, c in enumerate(table)]
    lines.append('],"cases":{')
    for n, (cid, r) in enumerate(packed.items()):
        lines.append("%s:{" % js(cid))
        parts = ["%s:%s" % (js(k), js(v)) for k, v in r.items()]
        lines += [p + ("," if i + 1 < len(parts) else "") for i, p in enumerate(parts)]
        lines.append("}" + ("," if n + 1 < len(packed) else ""))
    lines.append("}}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def load(path=FIXTURE):
    with open(path) as f:
        doc = json.load(f)
    table = doc["operator_calls"]
    out = {}
    for cid, r in doc["cases"].items():
        out[cid] = {k: (dict(v, calls=[table[i] for i in v["calls"]]) if k in ("forward", "backward") else v) for k, v in r.items()}
    return out


if __name__ == "__main__":
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    records = {c["id"]: record(c) for c in CASES}
    if "--check" in sys.argv:
        want, bad = load(), 0
        for cid, got in records.items():
            d = first_difference(want[cid], json.loads(json.dumps(got)), cid)
            print("%-28s %s" % (cid, d or "same"))
            bad += d is not None
        sys.exit(1 if bad else 0)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    save(records, out)
    for cid, r in records.items():
        print("%-28s forward %4d nodes, %3d calls%s" % (cid, r["forward"]["size"], len(r["forward"]["calls"]),
              "; backward %4d nodes, %3d calls, %d stages" % (r["backward"]["size"], len(r["backward"]["calls"]), len(r["backward"]["stages"])) if "backward" in r else ""))
