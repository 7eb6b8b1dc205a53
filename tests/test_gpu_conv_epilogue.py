"""The epilogue branches of conv_igemm_kernel / conv_pc_kernel that only a switch or a training descriptor selects, against the
float64 references of tests/kref.py through the replay of test_gpu_kernels_exact.py (bit for bit; statistics exact or within kref's
bound; the log-softmax epilogue within its derived bound; sentinels untouched; the launch log must name the row's kernel).

  * The generic (64-bit address) epilogue for plain NHWC output runs only under UBR_CONV_FAST_EPI=0, which the library reads once
    per process: every conv row of tests/kernel_matrix.py of the two families, and the three ragged cases below, replay in ONE
    fresh child process with the switch set.  The child runs under its own time limit; after a failed child nothing more is started.
  * In this process, per dtype, on the smallest igemm tile (FW, NT, TWF) = (1, 1, 1) and the matrix's ragged 2 x 2-tile extent
    (2 TH - 1) x (2 TW - 3) with a cut last channel group (try_thin never sees this tile): addend + addend_mask (the masked arm of
    the buffer-addressed epilogue), bnb_c + statistics and the three-class log-softmax (both always on the generic path)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (HERE, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import kernel_matrix as KM

pytestmark = pytest.mark.gpu

SWITCH = "UBR_CONV_FAST_EPI"
FAMILIES = ("conv_igemm_kernel", "conv_pc_kernel")
CHILD_TIMEOUT = 240        # seconds: process start, library load and ~85 launches of a few milliseconds each
_TROUBLE = []              # set once by a HIP error, a crashed child or a timeout; every later test fails without a launch

FW, NT, TWF = 1, 1, 1
TILE_HINT = KM.TILES.index((FW, NT, TWF)) + 1
TH, TW, TN = 4 * FW // TWF, 16 * TWF, 16 * NT
CASES = ("mask", "bnb", "logsoftmax")


def matrix_rows():
    return [r for r in KM.ROWS if r["op"] == "conv" and KM.family(r["symbols"][0]) in FAMILIES]


def ragged_row(T, case):
    """a call in the form of a kernel-matrix row (not part of the matrix): two images, 2 x 2 tiles of 4 x 16 pixels, the last ragged"""
    cpu = KM.CPU[T]
    a = dict(N=2, OH=2 * TH - 1, OW=2 * TW - 3, k=3, tile_hint=TILE_HINT, Cin=cpu)
    if case == "mask":          # whole channel units (the mask holds a byte per unit): 12 of 16 channels in fp32, 8 of 16 in 16 bits
        cout = (TN - 4) // cpu * cpu
        a.update(Cout=cout, ywidth=TN + 8, yoff=4, addend=True, mask=True)
    elif case == "bnb":
        a.update(Cout=TN - 4, ywidth=TN + 8, yoff=4, bnb=True)
    else:
        a.update(Cout=3, bias=True, logsoftmax=True)
    row = dict(symbols=("conv_igemm_kernel<%s, %d, %d, %d, false>" % (T, FW, NT, TWF),), op="conv", dtype=T, args=a, entry="ubr_conv", env=None)
    row["id"] = "ragged-%s-%s" % (T, case)
    return row


def _run(row):
    res, ms = KM.run_row(row)
    assert res.startswith(("exact", "bounded")), (row["id"], res)
    return res, ms


def test_generic_epilogue_of_every_igemm_and_pc_row_in_one_child_with_the_switch_off():
    assert not _TROUBLE, "not run: " + _TROUBLE[0]
    env = dict(os.environ, **{SWITCH: "0"})
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, "-m", "tests.test_gpu_conv_epilogue"]
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True)
    out = p.stdout + p.stderr
    if p.returncode != 0:
        _TROUBLE.append("child exit %d: %s" % (p.returncode, out[-400:]))
    assert p.returncode == 0, "child exit %d:\n%s" % (p.returncode, out[-3000:])
    done = [l.split()[1] for l in p.stdout.split("\n") if l.startswith("RESULT ")]
    want = [r["id"] for r in matrix_rows()] + ["ragged-%s-%s" % (T, c) for T in KM.DTYPES for c in CASES]
    assert done == want, "the child ran %d of %d rows" % (len(done), len(want))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("T", KM.DTYPES)
def test_ragged_smallest_igemm_tile(T, case):
    assert not _TROUBLE, "not run: " + _TROUBLE[0]
    try:
        _run(ragged_row(T, case))
    except RuntimeError as e:          # a failed HIP call (ubresnet_amd._lib.check) or a torch device error
        _TROUBLE.append("%s %s: %s" % (T, case, e))
        raise


def _main():
    assert os.environ.get(SWITCH) == "0", "%s must be 0 in this process" % SWITCH
    rows = matrix_rows() + [ragged_row(T, c) for T in KM.DTYPES for c in CASES]
    for row in rows:          # the first mismatch or HIP error ends the process: nothing runs after it
        res, ms = _run(row)
        print("RESULT %s %s %.1f" % (row["id"], res, ms), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(_main())
