"""Temperature calibration without a GPU: the ADDONS entry of libubresnet_calib.so, its include closure and a forced build; header,
binding, plan, reference and library agree on entry points and limits; the library stands alone and exports exactly its binding's
symbols; the compiled kernels are exactly those the GPU module's case table runs; every argument refusal returns UBF_EINVAL with a
message before any HIP call; g and h of the reference against central finite differences of its own NLL; the solver of
ubresnet_amd/calibration.py against the reference solver and on drawn labels; TemperatureScale; the launch plans as a stand-alone
program under the host sanitizers (tests/calib_host.cpp); the refusals of the Python surface that need no device."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import calib_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ubresnet_amd")
HEADER = os.path.join(REPO, "include", "ubresnet_calib.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
import cpu_helpers as H  # noqa: E402
from ubresnet_amd import _calib as F  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd import calibration as CB  # noqa: E402
from ubresnet_amd import deploy  # noqa: E402
from ubresnet_amd.training import epoch  # noqa: E402

LIB = B.ADDONS["calib"].out


# ------------------------------------------------------------------------------------------------------------------------
# the build table
# ------------------------------------------------------------------------------------------------------------------------
def _include_closure(files):
    seen, todo = set(), [os.path.realpath(f) for f in files]
    while todo:
        f = todo.pop()
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f).read(), flags=re.M):
            p = os.path.realpath(os.path.join(os.path.dirname(f), inc))
            if p not in seen:
                seen.add(p)
                todo.append(p)
    return seen


def test_the_addons_entry_is_appended_and_lists_the_true_include_closure():
    lib = B.ADDONS["calib"]
    assert isinstance(lib, B.Lib) and lib.sources == [os.path.join("extra", "ubr_calib.hip")] and lib.binding == "_calib"
    assert "calib" not in B.LIBS and "calib" not in B.EXTRAS and list(B.ADDONS)[:4] == ["blend", "sparse", "crop", "calib"]
    listed = [os.path.realpath(os.path.join(B.CSRC, h)) for h in lib.headers]
    assert len(listed) == len(set(listed)) and set(listed) == _include_closure([os.path.join(B.CSRC, s) for s in lib.sources])
    assert os.path.realpath(HEADER) in listed and os.path.realpath(os.path.join(B.CSRC, "ubr_calib_plan.h")) in listed
    assert not set(B.SOURCES + B.HEADERS) & set(lib.sources + lib.headers), "source_hash() covers the network's library only"


def test_a_forced_build_of_calib_is_one_compile_and_one_link(monkeypatch, capsys):
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    capsys.readouterr()
    built = B.build_addons(force=True, only=["calib"])
    monkeypatch.undo()
    lib = B.ADDONS["calib"]
    src, obj = os.path.join(B.CSRC, lib.sources[0]), os.path.join(B.CSRC, "extra", "ubr_calib.o")
    assert built == [lib.out] and len(lines) == 2
    assert lines[0] == [B.HIPCC] + B.FLAGS + ["-c", src, "-o", obj]
    assert lines[1] == [B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib.out, obj]
    io = capsys.readouterr()
    assert io.out == "" and io.err.strip().split("\n") == [" ".join(c) for c in lines]


def test_entry_point_reports_calib_on_stderr_before_the_score_line(monkeypatch, capsys):
    import __graft_entry__ as entry
    for lib in [l for t in (B.LIBS, B.ADDONS, B.EXTRAS) for l in t.values()]:
        H.need_lib(lib.out)
    for f in ("build", "build_addons", "build_extras"):
        monkeypatch.setattr(B, f, lambda *a, **kw: None)
    capsys.readouterr()
    entry.build()
    io = capsys.readouterr()
    err = io.err.strip().split("\n")
    assert "calib" not in io.out and "built %s ABI version 1" % LIB in err
    assert err[-1] == "built %s ABI version 1" % B.EXTRAS["score"].out
    assert err.index("built %s ABI version 1" % B.ADDONS["crop"].out) < err.index("built %s ABI version 1" % LIB) < len(err) - 1


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, plan, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_calib.h"\n'
                     'int main(void) {\n'
                     '  int64_t (*b)(int, int, int, int) = ubf_scratch_bytes;\n'
                     '  int (*a)(const float*, const void*, int, const float*, float, const uint8_t*, const float*, int, int, int, int, int, int,\n'
                     '           double*, unsigned long long*, void*, int64_t, void*) = ubf_accumulate;\n'
                     '  int (*p)(const float*, float*, const float*, int, int, int, int, void*) = ubf_apply;\n'
                     '  const char* (*e)(void) = ubf_last_error;\n'
                     '  int (*v)(void) = ubf_version;\n'
                     '  return b == 0 || a == 0 || p == 0 || e == 0 || v == 0 || UBF_OK != 0 || UBF_EINVAL != -1 || UBF_ELAUNCH != -2;\n}\n')
    r = subprocess.run([H.cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_plan_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(ubf_[a-z_0-9]+)\s*\(", text)
    assert declared == F.SYMBOLS == ["ubf_scratch_bytes", "ubf_accumulate", "ubf_apply", "ubf_last_error", "ubf_version"]
    limits = {k: int(v) for k, v in re.findall(r"#define\s+UBF_(MAX_CLASSES|REG_CLASSES|MAX_TEMPS|MAX_GROUPS|MAX_IMAGES|TRUTH_U8|TRUTH_I64)\s+(\d+)", text)}
    assert limits == dict(MAX_CLASSES=F.MAX_CLASSES, REG_CLASSES=F.REG_CLASSES, MAX_TEMPS=F.MAX_TEMPS, MAX_GROUPS=F.MAX_GROUPS,
                          MAX_IMAGES=F.MAX_IMAGES, TRUTH_U8=F.TRUTH_U8, TRUTH_I64=F.TRUTH_I64)
    assert F.MAX_TEMPS >= 33 >= 32, "the default grid of 33 temperatures is one call"
    assert (R.MAX_TEMPS, R.MAX_CLASSES, R.REG_CLASSES) == (F.MAX_TEMPS, F.MAX_CLASSES, F.REG_CLASSES)
    plan = open(os.path.join(B.CSRC, "ubr_calib_plan.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (BLOCK|UNROLL|LANE_PIXELS|MAX_ROWS|MAX_TEMPS|MAX_CLASSES|REG_CLASSES) = (\d+);", plan)}
    assert consts == dict(BLOCK=R.BLOCK, UNROLL=R.UNROLL, LANE_PIXELS=R.LANE_PIXELS, MAX_ROWS=R.MAX_ROWS, MAX_TEMPS=R.MAX_TEMPS,
                          MAX_CLASSES=R.MAX_CLASSES, REG_CLASSES=R.REG_CLASSES)
    assert "hip" not in re.sub(r"//.*", "", plan).lower() and "#include <stdint.h>" in plan
    for phrase in ("No atomic", "no workgroup", "ADDED to", "are\n * not read", "0x7FC00000", "all C outputs -inf", "S >= 1"):
        assert phrase in raw, phrase
    H.need_lib(LIB)
    assert F.lib().ubf_version() == F.BINDING.version() == 1


def test_library_stands_alone_and_exports_exactly_its_bindings_symbols():
    bd = F.BINDING
    assert bd.prefix == "ubf" and bd.path == LIB and os.path.basename(LIB) == "libubresnet_calib.so" and os.path.dirname(LIB) == PKG
    assert bd.symbols[-2:] == ["ubf_last_error", "ubf_version"]
    assert (F.LIB_PATH, F.SYMBOLS, F.lib, F.check) == (bd.path, bd.symbols, bd.lib, bd.check)
    H.need_lib(LIB)
    assert "libubresnet_" not in H.readelf("-d", LIB).replace("libubresnet_calib", "")
    assert sorted(n for n in H.defined_symbols(LIB) if re.match(r"ub[a-z]_", n)) == sorted(bd.symbols)
    others = [importlib.import_module("ubresnet_amd." + lib.binding).BINDING.prefix
              for t in (B.LIBS, B.EXTRAS, B.ADDONS) for n, lib in t.items() if n != "calib"]
    assert "ubf" not in others and len(set(others)) == len(others)
    tree = open(os.path.join(PKG, "_calib.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy)", tree, flags=re.M) and "from ._binding import Binding" in tree
    src = open(os.path.join(B.CSRC, B.ADDONS["calib"].sources[0])).read()
    assert '#include "../ubr_sat.h"' in src and '#include "../ubr_calib_plan.h"' in src and "SAT_EXPORTS(ubf, UBF_VERSION)" in src
    assert "Malloc" not in src and "hipFree" not in src and "Synchronize" not in src, "no allocation, free or sync"
    assert not re.findall(r"\batomic\w*\(", re.sub(r"//.*", "", src)), "no atomic operation"


def test_a_missing_library_is_a_runtime_error(monkeypatch):
    import importlib.util
    nowhere = os.path.join(REPO, "no_such_dir", "libubresnet_calib.so")
    monkeypatch.setenv("UBF_LIB", nowhere)
    spec = importlib.util.spec_from_file_location("ubresnet_amd._calib_missing", os.path.join(PKG, "_calib.py"))
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    for call in (lambda: fresh.scratch_bytes(1, 2, 2, 1), lambda: fresh.apply(0x1000, 0x1000, 0x2000, 1, 2, 2, 2)):
        with pytest.raises(RuntimeError, match="is missing; build it with") as e:
            call()
        assert nowhere in str(e.value) and "There is no CPU fallback" in str(e.value)


def test_the_compiled_kernels_are_the_case_table():
    """no allow-list: every compiled kernel is launched by a case of test_gpu_calib_exact.py, and the table names nothing else"""
    H.need_lib(LIB)
    compiled = kernel_symbols.kernels(LIB)
    assert compiled == sorted(R.KERNEL_CASES), (compiled, sorted(R.KERNEL_CASES))
    assert all(R.KERNEL_CASES.values()), [k for k, v in R.KERNEL_CASES.items() if not v]
    ran = H.case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_calib_exact.py"))
    assert ran == set(R.ACC_CASES) | set(R.APPLY_CASES) == set(i for v in R.KERNEL_CASES.values() for i in v)
    shapes = {c["shape"] for c in R.ACC_CASES.values()}
    assert {(1, 2, 1, 1), (2, 3, 7, 33), (2, 3, 64, 96)} <= shapes
    assert {c["K"] for c in R.ACC_CASES.values()} >= {1, 32, 33, 64}
    assert {c["shape"][1] for c in R.ACC_CASES.values()} >= {1, 2, 3, 4, 5, 16}


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals: every call below is refused on the host, before any HIP call; the addresses are never dereferenced
# ------------------------------------------------------------------------------------------------------------------------
_P = 0x100000
_ACC = dict(scores=_P, truth=_P + 0x10000, kind=1, lit=_P + 0x20000, thr=10.0, group=_P + 0x30000, betas=_P + 0x31000, K=3, N=2, C=3,
            H=4, W=5, G=2, table=_P + 0x40000, counters=_P + 0x41000, scratch=_P + 0x50000, sbytes=8 * 2 * 12)
_BAD_ACC = {
    "truth kind": (dict(kind=2), "truth_kind=2 must be"),
    "K 0": (dict(K=0), "K=0 must be 1..64"),
    "K 65": (dict(K=65), "K=65 must be 1..64"),
    "C 0": (dict(C=0), "C=0 must be 1..16"),
    "C 17": (dict(C=17), "C=17 must be 1..16"),
    "G 0": (dict(G=0), "G=0 must be 1..256"),
    "G 257": (dict(G=257), "G=257 must be 1..256"),
    "threshold NaN": (dict(thr=float("nan")), "lit_threshold is NaN"),
    "N 0": (dict(N=0), "N=0 must be 1..65535"),
    "N 65536": (dict(N=65536), "must be 1..65535"),
    "H 0": (dict(H=0), "H=0 and W=5 >= 1"),
    "W negative": (dict(W=-1), "W=-1 >= 1"),
    "2^40 pixels": (dict(N=2, H=1 << 20, W=1 << 20), "at most 2^40"),
    "null scores": (dict(scores=None), "null pointer (scores"),
    "null truth": (dict(truth=None), "null pointer (scores"),
    "null group": (dict(group=None), "null pointer (scores"),
    "null betas": (dict(betas=None), "null pointer (scores"),
    "null table": (dict(table=None), "null pointer (table"),
    "null counters": (dict(counters=None), "null pointer (table"),
    "null scratch": (dict(scratch=None), "null pointer (table"),
    "short scratch": (dict(sbytes=8 * 2 * 12 - 8), "is short of the 192"),
    "scores alignment": (dict(scores=_P + 2), "4-byte aligned"),
    "lit alignment": (dict(lit=_P + 0x20001), "4-byte aligned"),
    "truth alignment": (dict(truth=_P + 0x10004), "int64 truth must be 8-byte aligned"),
    "table alignment": (dict(table=_P + 0x40004), "8-byte aligned"),
    "scratch alignment": (dict(scratch=_P + 0x50004), "8-byte aligned"),
    "counters inside table": (dict(counters=_P + 0x40000 + 8), "two of table, counters and scratch overlap"),
    "scratch is table": (dict(scratch=_P + 0x40000), "two of table, counters and scratch overlap"),
    "table inside scores": (dict(table=_P + 16), "table overlaps an input"),
    "scratch is lit": (dict(scratch=_P + 0x20000), "scratch overlaps an input"),
    "counters is betas": (dict(counters=_P + 0x31000), "counters overlaps an input"),
}
_APP = dict(src=_P, dst=_P, betas=_P + 0x10000, n=2, C=3, th=4, tw=6)
_BAD_APP = {
    "C 0": (dict(C=0), "C=0 must be 1..16"),
    "C 17": (dict(C=17), "C=17 must be 1..16"),
    "n 0": (dict(n=0), "must be >= 1"),
    "th negative": (dict(th=-4), "must be >= 1"),
    "tw 0": (dict(tw=0), "must be >= 1"),
    "2^40 elements": (dict(n=4, th=1 << 19, tw=1 << 19), "at most 2^40"),
    "null in": (dict(src=None), "null pointer"),
    "null out": (dict(dst=None), "null pointer"),
    "null betas": (dict(betas=None), "null pointer"),
    "in alignment": (dict(src=_P + 1), "4-byte aligned"),
    "betas alignment": (dict(betas=_P + 0x10002), "4-byte aligned"),
    "partial overlap": (dict(dst=_P + 16), "out overlaps in without being in"),
    "out is betas": (dict(src=_P + 0x20000, dst=_P + 0x10000), "out overlaps betas"),
}


def _refused(rc, prefix, message):
    msg = F.lib().ubf_last_error().decode()
    assert rc == -1 and msg.startswith(prefix + ":") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=prefix):
        F.check(rc, "refused")


@pytest.mark.parametrize("name", sorted(_BAD_ACC))
def test_accumulate_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD_ACC[name]
    a = dict(_ACC, **change)
    rc = F.lib().ubf_accumulate(a["scores"], a["truth"], a["kind"], a["lit"], a["thr"], a["group"], a["betas"], a["K"], a["N"], a["C"], a["H"],
                                a["W"], a["G"], a["table"], a["counters"], a["scratch"], a["sbytes"], None)
    _refused(rc, "ubf_accumulate", message)


@pytest.mark.parametrize("name", sorted(_BAD_APP))
def test_apply_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD_APP[name]
    a = dict(_APP, **change)
    _refused(F.lib().ubf_apply(a["src"], a["dst"], a["betas"], a["n"], a["C"], a["th"], a["tw"], None), "ubf_apply", message)


def test_scratch_bytes_follow_the_plan():
    H.need_lib(LIB)
    for name, c in sorted(R.ACC_CASES.items()) + [("event", dict(shape=(3, 4, 1008, 3456), K=33))]:
        N, _, Hh, W = c["shape"]
        trips = -(-Hh * W // R.TRIP_PIXELS)
        gx = min(trips, max(1, R.MAX_ROWS // N))
        assert F.scratch_bytes(N, Hh, W, c["K"]) == 8 * N * gx * (3 * c["K"] + 3), name
    assert F.lib().ubf_scratch_bytes(1, 4, 4, 65) == 0 and b"K=65 must be 1..64" in F.lib().ubf_last_error()
    with pytest.raises(RuntimeError, match="ubf_scratch_bytes"):
        F.scratch_bytes(0, 4, 4, 1)


# ------------------------------------------------------------------------------------------------------------------------
# the reference and the solver
# ------------------------------------------------------------------------------------------------------------------------
def _logits(seed, M=4000, C=4, sigma=2.0):
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((M, C)) * sigma
    return rs, (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)


def test_g_and_h_of_the_reference_are_the_derivatives_of_its_nll():
    rs, l = _logits(3, M=50, C=5)
    t = rs.randint(0, 5, size=50)
    for beta in (0.25, 0.7, 1.0, 2.5, 4.0):
        eps = 1e-5 * beta
        lo, mid, hi = (R.pixel_terms(l, t, [b])[0][:, 0, :] for b in (beta - eps, beta, beta + eps))
        g_fd = (hi[:, 0] - lo[:, 0]) / (2 * eps)
        h_fd = (hi[:, 1] - lo[:, 1]) / (2 * eps)
        # central differences: the truncation is eps^2 f''' / 6, far below these tolerances; the rounding is 1e-16 / eps
        assert np.abs(g_fd - mid[:, 1]).max() <= 1e-8 * (1 + np.abs(mid[:, 1]).max()), beta
        assert np.abs(h_fd - mid[:, 2]).max() <= 1e-8 * (1 + np.abs(mid[:, 2]).max()), beta
        assert (mid[:, 2] >= 0).all()
    terms, bounds = R.pixel_terms(l, t, R.betas32(R.default_temps()))
    assert terms.shape == bounds.shape == (50, 33, 3) and (bounds > 0).all() and (bounds < 1e-3).all()
    assert abs(R.nll_sum(l, t, 0.5) - R.pixel_terms(l, t, [0.5])[0][:, 0, 0].sum()) <= 1e-10


def test_the_solver_is_the_reference_solver():
    rs = np.random.RandomState(5)
    for trial in range(200):
        b0 = rs.uniform(0.2, 3.0)
        b1 = b0 + rs.uniform(0.01, 0.5)
        # a convex stretch: g rises, h >= 0 and close to the secant so that the interpolant is monotone (one root)
        sec = rs.uniform(0.1, 50.0)
        g0 = -rs.uniform(0.01, 1.0) * sec * (b1 - b0)
        g1 = g0 + sec * (b1 - b0)
        h0, h1 = sec * rs.uniform(0.5, 1.5), sec * rs.uniform(0.5, 1.5)
        mine, ref = CB.hermite_root(b0, b1, g0, g1, h0, h1), R.hermite_root(b0, b1, g0, g1, h0, h1)
        assert b0 < mine < b1 and abs(mine - ref) <= 1e-12 * b1, (trial, mine, ref)
    assert CB.hermite_root(1.0, 2.0, 0.0, 3.0, 1.0, 1.0) == 1.0 and CB.hermite_root(1.0, 2.0, -3.0, 0.0, 1.0, 1.0) == 2.0
    assert CB.hermite_root(1.0, 3.0, -1.0, 1.0, 1.0, 1.0) == 2.0                     # the straight line
    with pytest.raises(ValueError, match="change sign"):
        CB.hermite_root(1.0, 2.0, 1.0, 2.0, 1.0, 1.0)


@pytest.mark.parametrize("T0", [0.6, 1.0, 1.7, 3.1])
def test_the_temperature_of_drawn_labels_lies_inside_the_sign_change_interval(T0):
    rs, l = _logits(int(T0 * 10))
    t = R.drawn_labels(rs, l, T0)
    temps = R.default_temps()
    betas = R.betas32(temps).astype(np.float64)
    table = R.pixel_terms(l, t, betas)[0].sum(0)[None]                                 # [1, K, 3]
    cal = CB.Calibration(temps, table, np.array([[len(t), 0, 0]], dtype=np.uint64))
    beta, edge, empty, interval = R.solve(betas, table[0, :, 1], table[0, :, 2], len(t))
    assert not edge and not empty and interval is not None
    assert cal.at_edge == [False] and cal.empty == [False]
    mine = cal.inverse_temperatures[0]
    assert interval[0] < mine < interval[1], "not strictly inside the interval where g changes sign"
    assert abs(mine - beta) <= 1e-12 * beta and cal.temperature(0) == 1.0 / mine
    # convexity: the NLL at any point of the interval is at most the larger of its ends
    assert R.nll_sum(l, t, mine) <= max(R.nll_sum(l, t, interval[0]), R.nll_sum(l, t, interval[1]))
    assert abs(np.log(cal.temperature(0) / T0)) < 0.2, "the fit is nowhere near the temperature the labels were drawn at"
    assert cal.nll(0).shape == (33,) and np.allclose(cal.nll(0) * len(t), table[0, :, 0]) and cal.gradient(0)[0] != 0
    assert cal.scale().temperatures == cal.temperatures


def test_at_edge_and_empty_behave_as_specified():
    rs, l = _logits(11)
    temps = R.default_temps()
    betas = R.betas32(temps).astype(np.float64)
    hot = R.pixel_terms(l, R.drawn_labels(rs, l, 9.0), betas)[0].sum(0)               # wants T = 9: beyond the grid's 4
    cold = R.pixel_terms(l, l.argmax(1), betas)[0].sum(0)                             # always right: wants T -> 0
    table = np.stack([hot, cold, np.zeros_like(hot), cold])
    counters = np.array([[len(l), 0, 0], [len(l), 5, 1], [0, 7, 0], [0, 0, 0]], dtype=np.uint64)
    cal = CB.Calibration(temps, table, counters)
    assert (hot[:, 1] > 0).all() and (cold[:, 1] < 0).all()
    assert cal.at_edge == [True, True, False, False] and cal.empty == [False, False, True, True]
    assert cal.temperatures[0] == 1.0 / float(betas.min()) and abs(cal.temperatures[0] - 4.0) < 1e-6
    assert cal.temperatures[1] == 1.0 / float(betas.max()) and abs(cal.temperatures[1] - 0.25) < 1e-7
    assert cal.temperatures[2:] == [1.0, 1.0], "a group without a counted pixel keeps T = 1, whatever its table holds"
    assert cal.tallies(1) == dict(counted=len(l), ignored=5, nonfinite=1) and np.isnan(cal.nll(2)).all()
    exact = CB.solve_group([0.5, 1.0, 2.0], [-1.0, 0.0, 1.0], [1.0, 1.0, 1.0], 10)
    assert exact == (1.0, False, False)
    assert CB.solve_group([1.0], [2.0], [1.0], 3) == (1.0, True, False)
    assert "at the edge" in str(cal) and "no pixel" in str(cal)
    with pytest.raises(ValueError, match="expected table"):
        CB.Calibration(temps, table[:, :5], counters)


def test_temperature_scale_validation_and_state_dict_round_trip(tmp_path):
    for bad in (0.0, -1.0, float("inf"), float("nan"), [1.0, 0.0], [], "1.0", True, None, [1.0, float("nan")]):
        with pytest.raises(ValueError, match="TemperatureScale"):
            CB.TemperatureScale(bad)
    one, three = CB.TemperatureScale(1.5), CB.TemperatureScale([0.8, 1.0, np.float32(2.0)])
    assert one.temperatures == [1.5] and len(three) == 3 and CB.TemperatureScale(three).temperatures == three.temperatures
    assert one.group_list(4) == [0, 0, 0, 0] and three.group_list(3) == [0, 1, 2] and three.group_list(2, [2, 2]) == [2, 2]
    for n, groups in ((2, None), (2, [0, 3]), (2, [0]), (2, [-1, 0])):
        with pytest.raises(ValueError, match="TemperatureScale"):
            three.group_list(n, groups)
    b = three.betas_for([2, 0, 0])
    assert b.dtype == np.float32 and b.tolist() == [0.5, float(np.float32(1.25)), float(np.float32(1.25))]
    path = str(tmp_path / "ck.tar")
    deploy.save_checkpoint({"state_dict": {}, "temperature": three.state_dict()}, False, 0, filename=path)
    back = torch.load(path, map_location="cpu", weights_only=True)["temperature"]
    assert CB.TemperatureScale(1.0).load_state_dict(back).temperatures == three.temperatures
    with pytest.raises(ValueError, match="positive and finite"):
        CB.TemperatureScale(1.0).load_state_dict({"temperature": torch.tensor([1.0, -2.0])})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        one.apply_(torch.zeros(1, 2, 2, 2))
    with pytest.raises(ValueError, match="float32"):
        one.apply_(torch.zeros(1, 2, 2, 2, dtype=torch.float64))
    assert CB.as_scale(None) is None and CB.as_scale(2.0).temperatures == [2.0] and CB.as_scale(three).temperatures == three.temperatures


def test_temperature_fit_refusals_without_a_device():
    for kw in (dict(num_classes=0), dict(num_classes=17), dict(num_classes=4, groups=0), dict(num_classes=4, groups=257),
               dict(num_classes=4, temps=[1.0, -1.0]), dict(num_classes=4, temps=[]), dict(num_classes=4, temps=[1.0] * 65),
               dict(num_classes=4, adc_threshold=float("nan")), dict(num_classes=True)):
        with pytest.raises(ValueError, match="TemperatureFit"):
            CB.TemperatureFit(**kw)
    fit = CB.TemperatureFit(4, groups=3)
    assert fit.temps == CB.default_temps() == R.default_temps() and len(fit.temps) == 33
    assert fit.temps[0] == 0.25 and fit.temps[16] == 1.0 and fit.temps[-1] == 4.0
    assert np.array_equal(fit.betas, R.betas32(fit.temps)) and fit.betas.dtype == np.float32
    s, t, v = torch.zeros(3, 4, 6, 8), torch.zeros(3, 6, 8, dtype=torch.int64), torch.zeros(3, 1, 6, 8)
    for args, kw in (((s.double(), t), {}), ((s, t.int()), {}), ((s[:, :3], t), {}), ((s, t[:2]), {}), ((s, t, v.double()), {}),
                     ((s, t, v[:, :, :5]), {}), ((s, t, v), dict(groups=[0, 1])), ((s, t, v), dict(groups=[0, 1, 3])), ((s[:2], t[:2]), {})):
        with pytest.raises(ValueError, match="TemperatureFit.add"):
            fit.add(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit.add(s, t, v)
    cal = fit.read()                                                                   # nothing added: zeros, every group empty
    assert cal.empty == [True] * 3 and cal.temperatures == [1.0] * 3 and fit.calls == 0
    stacked = CB.TemperatureFit(4)._shapes(s[0], t[0], v)                              # [C, rows, cols] with the view of three planes
    assert stacked[0].shape == (1, 4, 6, 8) and stacked[1].shape == (1, 6, 8) and stacked[2].shape == (1, 6, 8)


class _Conv:
    in_channels, out_channels = 1, 3


class _Model:
    conv1 = conv11 = _Conv()

    def eval(self):
        raise AssertionError("the arguments are checked before the model is touched")


def test_the_deployment_keyword_without_a_device():
    kw = dict(planes=3, tile=(64, 96), batch=4)
    sig = inspect.signature(deploy.WholeViewSegmenter.__init__).parameters
    assert sig["temperature"].default is None and inspect.signature(deploy.segment_crops).parameters["temperature"].default is None
    assert inspect.signature(epoch.validate).parameters["calibration"].default is None
    base = deploy.WholeViewSegmenter(_Model(), 96, 160, **kw)
    assert base.scale is None and base._tile_groups is None
    one = deploy.WholeViewSegmenter(_Model(), 96, 160, temperature=1.5, **kw)
    assert one.tiles == base.tiles and one.scale.temperatures == [1.5] and one._tile_groups == [0] * len(base.tiles)
    per = deploy.WholeViewSegmenter(_Model(), 96, 160, temperature=[0.5, 1.0, 2.0], **kw)
    assert per._tile_groups == [t[0] for t in base.tiles] and set(per._tile_groups) == {0, 1, 2}
    assert deploy.WholeViewSegmenter(_Model(), 96, 160, temperature=CB.TemperatureScale([1, 2, 3]), **kw).scale.temperatures == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="one value or one per plane"):
        deploy.WholeViewSegmenter(_Model(), 96, 160, temperature=[1.0, 2.0], **kw)
    for bad in (0.0, [1.0, -1.0, 1.0], "hot"):
        with pytest.raises(ValueError, match="TemperatureScale"):
            deploy.WholeViewSegmenter(_Model(), 96, 160, temperature=bad, **kw)
    with pytest.raises(ValueError, match="single value"):
        deploy.segment_crops(_Model(), torch.zeros(1, 1, 8, 8), temperature=[1.0, 2.0])
    assert "temperature" in deploy.WholeViewSegmenter.__doc__ and "single-view" in deploy.WholeViewSegmenter.__doc__


# ------------------------------------------------------------------------------------------------------------------------
# the plans as a program
# ------------------------------------------------------------------------------------------------------------------------
def test_plans_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/calib_host.cpp has its own main and includes ubr_calib_plan.h; built with -fsanitize=address,undefined and run as a
    process of its own over every accumulate case of the table and a sweep of its own"""
    exe = str(tmp_path / "calib_host")
    r = subprocess.run([H.cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "calib_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    calls = sorted({(c["shape"][0], c["shape"][2], c["shape"][3], c["K"]) for c in R.ACC_CASES.values()})
    p = subprocess.run([exe] + [str(v) for c in calls for v in c], capture_output=True, text=True)
    assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
    rows = [[int(v) for v in l.split()[1:]] for l in p.stdout.strip().split("\n") if l.startswith("A ")]
    assert [tuple(r[:4]) for r in rows] == calls
    H.need_lib(LIB)
    for N, Hh, W, K, hw, trips, gx, nrows, words, sbytes in rows:
        assert hw == Hh * W and trips == -(-hw // R.TRIP_PIXELS) and gx == min(trips, max(1, R.MAX_ROWS // N)) and nrows == N * gx
        assert words == 3 * K + 3 and sbytes == F.scratch_bytes(N, Hh, W, K)
    by = {tuple(r[:4]): r for r in rows}
    assert by[(2, 64, 96, 33)][5:7] == [3, 3] and by[(1, 40, 60, 5)][5:7] == [2, 2] and by[(1100, 1, 2049, 1)][5:7] == [2, 1]
    assert p.stdout.strip().split("\n")[-1].split()[:7] == ["G"] + [str(v) for v in (R.BLOCK, R.UNROLL, R.LANE_PIXELS, R.TRIP_PIXELS, R.MAX_ROWS,
                                                                                     R.MAX_TEMPS)]
