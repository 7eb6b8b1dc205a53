"""Every row of tests/kernel_matrix.py on the GPU: the row's call runs on kref.exact_operands in NaN-guarded buffers with the
library's launch log on, its outputs are compared with the float64 reference by the replay functions of test_gpu_kernels_exact.py
(bit for bit; statistics exact or within kref's bound; the log-softmax epilogue within its derived bound; every byte outside the output
views untouched), and the log must hold exactly the kernels the row declares -- which, with test_cpu_kernel_matrix.py, means every
compiled instantiation of the covered families has been launched and checked.  Rows with `env` run in a fresh child process.
After the first HIP error, crash or timeout every later row fails at once without touching the GPU.  Prints one table line per row."""
import os
import subprocess
import sys

import pytest

import kernel_matrix as KM

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120        # seconds: process start, library load and one small launch
_TROUBLE = []              # set once by a HIP error, a crashed child or a timeout; every later row fails without a launch
_ROWS = []


def _trouble(why):
    if not _TROUBLE:
        _TROUBLE.append(why)


def _line(row, res, ms):
    return "%-62s %-10s %-44s %-22s %8.1f ms" % (" + ".join(row["symbols"]), row["entry"], row["shape"] + (" " + " ".join("%s=%s" % kv for kv in row["env"].items()) if row["env"] else ""), res, ms)


def _run_child(row):
    env = dict(os.environ, **row["env"])
    try:
        p = subprocess.run([sys.executable, "-m", "tests.kernel_matrix", row["id"]], cwd=REPO, env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _trouble("row %s: child timed out" % row["id"])
        raise AssertionError(_TROUBLE[0])
    out = p.stdout + p.stderr
    if p.returncode in (134, 139, -6, -11) or (p.returncode != 0 and ("HIP call failed" in out or "hipError" in out)):
        _trouble("row %s: child exit %d: %s" % (row["id"], p.returncode, out[-400:]))
    assert p.returncode == 0, "child exit %d:\n%s" % (p.returncode, out[-2000:])
    last = [l for l in p.stdout.split("\n") if l.startswith("RESULT ")][-1].split()
    return last[1], float(last[2])


@pytest.mark.parametrize("row", KM.ROWS, ids=[r["id"] for r in KM.ROWS])
def test_row_runs_its_kernels_and_matches_the_fp64_reference(row):
    assert not _TROUBLE, "not run: " + _TROUBLE[0]
    try:
        if row["env"]:
            res, ms = _run_child(row)
        else:
            try:
                res, ms = KM.run_row(row)
            except RuntimeError as e:          # a failed HIP call (ubresnet_amd._lib.check) or a torch device error
                _trouble("row %s: %s" % (row["id"], e))
                raise
    except BaseException:
        _ROWS.append(_line(row, "FAIL", 0.0))
        raise
    assert res.startswith(("exact", "bounded")), res
    _ROWS.append(_line(row, res, ms))


def test_matrix_table(capsys):
    """the table of profiles/kernel_matrix.txt: one line per row that ran in this session"""
    with capsys.disabled():
        print("\nkernel matrix: %d rows, %d distinct kernels" % (len(_ROWS), len({s for r in KM.ROWS for s in r["symbols"]})))
        for l in _ROWS:
            print("  " + l)
    assert not _TROUBLE, _TROUBLE[0]
