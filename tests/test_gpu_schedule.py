"""The launch schedule as a whole: for both networks, in every mode that takes a different path through the executor, the
recorded forward and backward tapes hold exactly the operator calls of tests/golden/schedule/schedule.json -- tape size, every
labelled call's (op, kernel symbol, shape signature) in issue order, the launches each call put on the tape, and the backward's
hand-over stages (gradient range, side-stream mark).  The kernels have exact tests of their own; this pins WHICH launches a pass
issues and in what order.  A deliberate schedule change regenerates the fixture (tests/golden/schedule/make_schedule.py)."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schedule")
_spec = importlib.util.spec_from_file_location("make_schedule", os.path.join(_HERE, "make_schedule.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)


@pytest.fixture(scope="module")
def golden():
    return S.load()


def test_fixture_covers_exactly_the_cases(golden):
    assert list(golden) == [c["id"] for c in S.CASES]


@pytest.mark.parametrize("case", S.CASES, ids=[c["id"] for c in S.CASES])
def test_recorded_tapes_hold_the_golden_schedule(case, golden, monkeypatch):
    from ubresnet_amd import engine, plan
    monkeypatch.setattr(plan, "ENABLED", True)
    monkeypatch.setattr(engine, "_INFER_FOLD", case.get("fold", True))
    m, x, lab, wgt = S.build(case)
    S.run_pass(case, m, x, lab, wgt)        # records the tapes
    S.run_pass(case, m, x, lab, wgt)        # replays them
    got = json.loads(json.dumps(S.schedule(case, m)))
    want = golden[case["id"]]
    assert got["case"] == want["case"]
    diff = S.first_difference(want, got, case["id"])
    assert diff is None, diff
    assert got["forward"]["size"] >= sum(got["forward"]["launches"])
    assert ("backward" in got) == (case["mode"] != "infer")
