"""The kernel matrix (tests/kernel_matrix.py) against the built library, without a GPU: the symbols its rows declare are exactly the
kernels compiled into libubresnet_hip.so -- an instantiation without a row, or a row for a kernel that is not compiled, fails by
name -- and every row is well-formed.  tests/test_gpu_kernel_matrix.py runs the rows."""
import os
import sys

import pytest

import kernel_matrix as KM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "ubresnet_amd", "libubresnet_hip.so")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from ubresnet_amd._lib import SYMBOLS as ENTRY_POINTS  # noqa: E402


@pytest.fixture(scope="module")
def compiled():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    return kernel_symbols.kernels(LIB)


def test_rows_equal_the_compiled_kernels(compiled):
    have = set(compiled)
    assert len(have) > 100, "symbol listing broken?"
    declared = {}
    for r in KM.ROWS:
        for s in r["symbols"]:
            declared.setdefault(s, r["id"])
    missing = sorted(have - set(declared))
    assert not missing, "compiled kernels without a row in tests/kernel_matrix.py: %s" % ", ".join(missing)
    stale = sorted("%s (row %s)" % (s, declared[s]) for s in set(declared) - have)
    assert not stale, "rows for kernels that are not compiled: %s" % ", ".join(stale)


def test_normalize_takes_mangled_and_demangled_names():
    n = kernel_symbols.normalize(["_ZN12_GLOBAL__N_114conv_pc_kernelIfLi4ELi2ELi9EEEvNS_5ConvKE",
                                  "void (anonymous namespace)::conv_pc_kernel<float, 4, 2, 9>((anonymous namespace)::ConvK)",
                                  "bn_finalize_kernel(double const*, double)", ""])
    assert n == ["conv_pc_kernel<float, 4, 2, 9>", "conv_pc_kernel<float, 4, 2, 9>", "bn_finalize_kernel"]


def test_rows_are_well_formed():
    ids = [r["id"] for r in KM.ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    firsts = [r["symbols"][0] for r in KM.ROWS if not r.get("tag")]
    assert len(firsts) == len(set(firsts)), "two rows claim the same kernel"
    for r in KM.ROWS:
        assert r["dtype"] in KM.DTYPES and r["entry"] in ENTRY_POINTS and r["op"] in KM.OPS and r["symbols"], r["id"]
        assert all(s.split("<")[1].startswith(r["dtype"]) for s in r["symbols"] if "<" in s), r["id"]
        for k in (r["env"] or {}):
            assert k in KM.ENV_SWITCHES, "%s: unknown switch %s" % (r["id"], k)
        if r["op"] in ("conv", "wgrad"):
            a = r["args"]
            assert a["Cin"] % KM.CPU[r["dtype"]] == 0 and a["N"] >= 2, r["id"]


def test_env_switches_are_read_by_the_sources_and_used_by_rows():
    src = open(os.path.join(REPO, "ubresnet_amd", "csrc", "ubr_wgrad.hip")).read()
    for k in KM.ENV_SWITCHES:
        assert 'getenv("%s")' % k in src, k
    assert {k for r in KM.ROWS for k in (r["env"] or {})} == set(KM.ENV_SWITCHES)


@pytest.mark.parametrize("row", [r for r in KM.ROWS if r["op"] == "wgrad"], ids=lambda r: r["id"])
def test_the_restated_wgrad_planner_picks_the_rows_kernel(row):
    a = row["args"]
    sym, nsplit = KM.wgrad_variant(row["dtype"], a["N"], a["GH"], a["GW"], a["Cin"], a["Cout"], a["k"], a.get("dil", 1), env=row["env"])
    assert sym == row["symbols"][0], (sym, nsplit)
    assert ("wgrad_reduce_flat_kernel" if nsplit <= 8 else "wgrad_reduce_kernel") in row["symbols"], nsplit
