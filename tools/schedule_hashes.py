#!/usr/bin/env python3
"""Bitwise record of what the schedule cases (tests/golden/schedule/make_schedule.py) compute: SHA-256 of the log-probabilities,
of every BatchNorm buffer after the pass and of every parameter gradient, for the recorded and for the replayed pass of each case.
A change that must not alter results (a scheduler refactor) is checked by running this in a checkout of each commit -- copy this
file and the generator into the older one -- and comparing; two runs of ONE commit show what reproduces at all.

    python tools/schedule_hashes.py OUT.json
    python tools/schedule_hashes.py --compare A.json B.json       exit 1 and the tensors' names if any hash differs"""
import hashlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = [(k, t) for k in sorted(set(a) | set(b)) for t in sorted(set(a.get(k, {})) | set(b.get(k, {})))
           if a.get(k, {}).get(t) != b.get(k, {}).get(t)]
    for k, t in bad:
        print("DIFFERS %s %s" % (k, t))
    print("%s vs %s: %d of %d tensors differ over %d passes" % (pa, pb, len(bad), sum(len(v) for v in a.values()), len(a)))
    return 1 if bad else 0


def main(out):
    sys.path.insert(0, ROOT)
    spec = importlib.util.spec_from_file_location("make_schedule", os.path.join(ROOT, "tests", "golden", "schedule", "make_schedule.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    import torch

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()

    res = {}
    for case in S.CASES:
        m, x, lab, wgt = S.build(case)
        with S.infer_fold(case):
            for which in ("recorded", "replayed"):
                ts = {"logp": S.run_pass(case, m, x, lab, wgt)}
                ts.update(("buffer:" + n, b) for n, b in m.named_buffers())
                if case["mode"] != "infer":
                    ts.update(("grad:" + n, p.grad) for n, p in m.named_parameters())
                res["%s/%s" % (case["id"], which)] = {n: sha(t) for n, t in ts.items()}
        plan, = m.__dict__["_ubr_engine"]._planned.values()
        assert plan.uses == 2, "the second pass of %s did not replay" % case["id"]
    with open(out, "w") as f:
        json.dump(res, f)
    print("wrote %s: %d passes, %d tensors" % (out, len(res), sum(len(v) for v in res.values())))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
