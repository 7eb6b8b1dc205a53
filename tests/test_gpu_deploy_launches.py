"""What a deployment call puts on the stream: for every configuration of tools/deploy_trace.py -- WholeViewSegmenter over output,
sparse input, tta, margin, blend, temperature, capacity, eager forward and stacked tiles, segment_crops over output, tta and
temperature -- the recorded calls of the deployment libraries, graph replays and eager forwards equal
tests/golden/deploy_launches.json entry for entry: symbol, every integer and float argument, the descriptors by content and the
device buffers by their order of first appearance.  Every configuration is recorded twice; the second call reuses the buffers of
the first and must issue the same launches.  The kernels have exact tests of their own; this pins WHICH launches a call issues.
A deliberate change of the launch sequence regenerates the fixture (python tools/deploy_trace.py OUT.json --fixture)."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import deploy_trace as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return T.load()


def test_fixture_covers_exactly_the_configurations(golden):
    assert list(golden) == T.IDS
    assert all(golden[k] for k in T.IDS)


@pytest.mark.parametrize("case_id", T.IDS)
def test_launches_are_the_golden_ones(case_id, golden):
    (first, second), hashes = T.record(case_id)
    for trace, which in ((first, "first call"), (second, "second call")):
        diff = T.first_difference(golden[case_id], trace, "%s, %s" % (case_id, which))
        assert diff is None, diff
    assert hashes and all(len(h) == 64 for h in hashes.values())
