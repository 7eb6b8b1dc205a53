"""Event crops without a GPU: the Philox known answer; the numpy reference of tests/crop_ref.py against brute force and against
cases written out by hand; the branch case covers every branch of the selection; libubresnet_crop.so's header is C99, header,
binding, reference and library agree; the compiled kernels are exactly those the GPU module's case table runs; the library stands
alone and exports its binding's symbols; the ADDONS entry, its include closure and a forced build; every argument refusal returns
UBN_EINVAL with a message before any HIP call; the rule as a stand-alone program under the host sanitizers (tests/crop_host.cpp)
against the reference; the refusals of the Python surface that need no device, the choice of the cell among them."""
import importlib
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import crop_ref as R
import det_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ubresnet_amd")
HEADER = os.path.join(REPO, "include", "ubresnet_crop.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
import cpu_helpers as H  # noqa: E402
from ubresnet_amd import _crop as N  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd import crops, sparse, synthetic  # noqa: E402

LIB = B.ADDONS["crop"].out
f32, u8, i32, i64 = np.float32, np.uint8, np.int32, np.int64


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answer_under_the_crop_tag():
    assert N.PHILOX_TAG == R.PHILOX_TAG == 0x43524F50 != det_ref.PHILOX_TAG
    assert tuple(int(v) for v in det_ref.philox(1, 0, 0, 0, 0, R.PHILOX_TAG)) == (3488071712, 2852949502, 2108613644, 1460095574)


@pytest.mark.parametrize("name", ["branch", "g4-tails", "g64", "wide-scan", "stacked", "class-mask", "lit-rule", "label-f32-edges", "one-position"])
def test_sat_windows_equal_brute_force_at_every_legal_position(name):
    a = R.inputs(name)
    ref = R.reference(a)
    count, s, geo, g = ref["count"], ref["sat"], a["geo"], a["g"]
    assert s.shape == N.sat_shape(a["Q"], a["rows"], a["cols"], g) and s.dtype == i32
    assert not s[:, 0, :].any() and not s[:, :, 0].any() and (s[:, -1, -1] == count.reshape(a["Q"], -1).sum(axis=1)).all()
    for q in range(a["Q"]):
        for i in range(geo["NR"]):
            for j in range(geo["NC"]):
                assert R.window(s, geo, q, i, j) == R.window_brute(count, q, i * g, j * g, a["H"], a["W"]), (q, i, j)
    assert geo["NR"] == (a["rows"] - a["H"]) // g + 1 and geo["NC"] == (a["cols"] - a["W"]) // g + 1


def test_the_branch_case_takes_every_branch():
    """a condition on the inputs of tests/test_gpu_crops_exact.py, from the reference alone"""
    a = R.inputs("branch")
    assert (a["P"], a["rows"], a["cols"], a["H"], a["W"], a["g"], a["K"], a["T"], a["min_lit"], a["seed"], a["number"]) == (3, 48, 80, 16, 32, 16, 8, 3, 256, 18, 2)
    assert (a["geo"]["NR"], a["geo"]["NC"]) == (3, 4)
    t = R.reference(a)["table"]
    assert t[0].tolist() == [0, 0, 0, 512, 0, 1, 1, 0] and t[5].tolist() == [1, 32, 48, 1, 2, 0, 0, 0]
    lit, tries, acc = t[:, 3], t[:, 4], t[:, 5]
    assert ((acc == 1) & (tries == 0)).any(), "an acceptance at try 0"
    assert ((acc == 1) & (lit == 256)).any(), "an acceptance with exactly min_lit"
    assert ((acc == 1) & (tries == 2)).any(), "an acceptance at the last try"
    assert ((acc == 0) & (lit == 1) & (tries == 2)).any(), "a fallback that found its best late"
    assert ((acc == 0) & (lit == 0) & (tries == 0)).any(), "an all-zero fallback keeps try 0"
    assert {tuple(r) for r in t[:, 6:].tolist()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert not np.array_equal(t, R.reference(R.inputs("other-number"))["table"])


def test_the_cases_cover_what_they_must():
    C = R.CASES
    assert {R.inputs(n)["g"] for n in C} >= {4, 16, 64}
    assert {c["kind"] for c in C.values()} == {R.U8, R.I64, R.F32} and {c["offset"] for c in C.values()} == {0, -1}
    assert {(c["K"], c["T"]) for c in C.values()} >= {(1, 1), (257, 2), (3, 64)} and 257 > N.LANES
    assert any(c["shift"] for c in C.values()) and any(c["stacked"] for c in C.values()) and any(not c["weight"] for c in C.values())
    assert (C["one-position"]["rows"], C["one-position"]["cols"]) == (C["one-position"]["H"], C["one-position"]["W"])
    wide = R.inputs("wide-scan")
    assert wide["g"] == 4 and wide["geo"]["CC"] == 260 > N.LANES and wide["geo"]["CR"] == 2 and (R.reference(wide)["sat"][:, 1, 1:] > 0).all()
    g4 = R.inputs("g4-tails")
    assert (g4["rows"], g4["cols"], g4["H"], g4["W"], g4["g"]) == (20, 36, 8, 12, 4) and g4["W"] // 4 % 2 == 1
    st = R.reference(R.inputs("stacked"))
    assert R.inputs("stacked")["label"].shape == (48, 80) and st["image"].shape[1] == 3 and st["sat"].shape[0] == 1
    assert {0, 1} <= set(st["table"][:, 5].tolist()) or st["table"][:, 4].max() > 0
    own = R.inputs("own-table")
    assert R.reference(own)["bad"] == 9 and own["status0"] > 2 ** 32
    on, off = R.reference(R.inputs("switches-on"))["table"], R.reference(R.inputs("switches-off"))["table"]
    assert len({tuple(r) for r in on[:, 6:].tolist()}) == 4 and not off[:, 6:].any() and np.array_equal(on[:, :3], off[:, :3])
    assert (R.reference(g4)["table"][:, 1:3] % 8 != 0).any()
    assert set(R.reference(R.inputs("planes-list"))["table"][:, 0].tolist()) == {0, 2}
    assert R.reference(R.inputs("t64"))["table"][:, 4].max() > 3
    k1 = R.reference(R.inputs("k1-t1"))["table"]
    assert k1.shape == (1, 8) and k1[0, 4] == 0 and k1[0, 5] == 0
    mixed = R.reference(R.inputs("g4-tails"))["table"][:, 5]
    assert mixed.any() and not mixed.all()


def test_reference_by_hand():
    assert R.convert_labels(R.EDGE_LABELS, -1).tolist() == R.EDGE_LABELS_MINUS_1
    assert R.convert_labels(np.array([0, 255], u8), -1).tolist() == [-1, 254]
    assert R.convert_labels(np.array([-2 ** 63, 5], i64), -1).tolist() == [2 ** 63 - 1, 4]               # wraps
    assert R.label_counts(np.array([0, 1, 31, 32, -1, R.NO_LABEL]), (1 << 31) | 1).tolist() == [True, False, True, False, False, False]
    nan, inf = f32(np.nan), f32(np.inf)
    img = np.array([[[10.0, np.nextafter(f32(10), inf), nan, inf]], [[11.0, 0.0, 0.0, -inf]]], f32)
    assert R.counting(img, None, 0, 0, False, 10.0).tolist() == [[[False, True, False, True]], [[True, False, False, False]]]
    assert R.counting(img, None, 0, 0, True, 10.0).tolist() == [[[True, True, False, True]]]
    lab = np.array([[1, 2, 1, 0]], u8)
    assert R.counting(img, lab, 0, 0b010, True, 10.0).tolist() == [[[True, False, False, False]]]
    # one 4 x 8 plane, cell 4: two cells; a 4 x 4 crop at either; flips of a gather by hand
    image = np.arange(32, dtype=f32).reshape(1, 4, 8)
    s = R.sat(image > 19.5, 4)
    assert s.tolist() == [[[0, 0, 0], [0, 4, 12]]]
    oi, ol, ow, bad = R.gather(image, np.zeros((1, 4, 8), u8), 0, None, False, np.array([[0, 0, 4, 0, 0, 0, 1, 1], [0, 1, 0, 0, 0, 0, 0, 0]], i32), 4, 4)
    assert bad == 1 and oi[0, 0, 0].view(f32).tolist() == [31.0, 30.0, 29.0, 28.0] and oi[0, 0, 3, 3].view(f32) == 4.0 and not oi[1].any()
    assert (ow[0] == 0x3F800000).all() and not ow[1].any()
    for rows, cols, Hc, Wc, g in ((1008, 3456, 512, 512, 16), (1008, 3456, 512, 832, 16), (20, 36, 8, 12, 4), (128, 192, 64, 128, 64), (10, 10, 6, 6, 0)):
        assert R.largest_cell(rows, cols, Hc, Wc) == N.largest_cell(rows, cols, Hc, Wc) == g


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_crop.h"\n'
                     'int main(void) {\n'
                     '  int (*o)(const float*, const void*, int, int32_t, uint32_t, int, float, int, int, int, int, int32_t*, void*) = ubn_occupancy;\n'
                     '  int (*c)(const int32_t*, int, int, int, int, int, int, const int32_t*, int, int, int, int32_t, uint32_t, uint32_t, uint32_t,\n'
                     '           int, int, int32_t*, void*) = ubn_choose;\n'
                     '  int (*g)(const float*, const void*, int, int32_t, const float*, int, int, int, int, int, int, const int32_t*, int, float*,\n'
                     '           int64_t*, float*, unsigned long long*, void*) = ubn_gather;\n'
                     '  const char* (*e)(void) = ubn_last_error;\n'
                     '  int (*v)(void) = ubn_version;\n'
                     '  return o == 0 || c == 0 || g == 0 || e == 0 || v == 0 || UBN_OK != 0 || UBN_EINVAL != -1 || UBN_ELAUNCH != -2\n'
                     '         || UBN_PHILOX_TAG != 0x43524F50u;\n}\n')
    r = subprocess.run([H.cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(ubn_[a-z_0-9]+)\s*\(", text)
    assert declared == N.SYMBOLS == ["ubn_occupancy", "ubn_choose", "ubn_gather", "ubn_last_error", "ubn_version"]
    names = "LANES|MIN_CELL|MAX_CELL|MAX_CELL_COLS|MAX_PLANES|MAX_CROPS|MAX_TRIES|TABLE_FIELDS|LABEL_NONE|LABEL_U8|LABEL_I64|LABEL_F32"
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBN_(%s)\s+(\d+)" % names, text)}
    assert geometry == {k: getattr(N, k) for k in names.split("|")}
    assert (R.LANES, R.MIN_CELL, R.MAX_CELL, R.MAX_CELL_COLS, R.MAX_PLANES, R.MAX_CROPS, R.MAX_TRIES, R.TABLE_FIELDS) == (
        N.LANES, N.MIN_CELL, N.MAX_CELL, N.MAX_CELL_COLS, N.MAX_PLANES, N.MAX_CROPS, N.MAX_TRIES, N.TABLE_FIELDS)
    assert (R.NONE, R.U8, R.I64, R.F32) == (N.LABEL_NONE, N.LABEL_U8, N.LABEL_I64, N.LABEL_F32) and len(N.FIELDS) == N.TABLE_FIELDS
    assert re.search(r"#define\s+UBN_PHILOX_TAG\s+0x43524F50u", text)
    for phrase in ("strict; NaN is not lit", "earliest on\n * ties", "ADDED to status[0]", "Every element is written", "No atomic",
                   "No workgroup waits for another", "relative\n * bias below N / 2^32", "Two crops may be the same", "nothing is read through it"):
        assert phrase in raw, phrase
    H.need_lib(LIB)
    assert N.lib().ubn_version() == N.BINDING.version() == 1


def test_library_stands_alone_and_exports_exactly_its_bindings_symbols():
    bd = N.BINDING
    assert bd.prefix == "ubn" and bd.path == LIB and os.path.basename(LIB) == "libubresnet_crop.so" and os.path.dirname(LIB) == PKG
    assert bd.symbols[-2:] == ["ubn_last_error", "ubn_version"]
    assert (N.LIB_PATH, N.SYMBOLS, N.lib, N.check) == (bd.path, bd.symbols, bd.lib, bd.check)
    H.need_lib(LIB)
    assert "libubresnet_" not in H.readelf("-d", LIB).replace("libubresnet_crop", "")
    assert sorted(n for n in H.defined_symbols(LIB) if re.match(r"ub[a-z]_", n)) == sorted(bd.symbols)
    tables = [t for t in (B.LIBS, B.EXTRAS, B.ADDONS)]
    others = [importlib.import_module("ubresnet_amd." + lib.binding).BINDING.prefix for t in tables for n, lib in t.items() if n != "crop"]
    assert "ubn" not in others and len(set(others)) == len(others)
    tree = open(os.path.join(PKG, "_crop.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy)", tree, flags=re.M) and "from ._binding import Binding" in tree
    src = open(os.path.join(B.CSRC, B.ADDONS["crop"].sources[0])).read()
    assert '#include "../ubr_sat.h"' in src and '#include "../ubr_crop_rule.h"' in src and "SAT_EXPORTS(ubn, UBN_VERSION)" in src
    assert "Malloc" not in src and "hipFree" not in src and "Synchronize" not in src, "no allocation, free or sync"
    code = re.sub(r"//.*", "", src)
    assert len(re.findall(r"\batomic\w*\(", code)) == 1 and "atomicAdd(a.status" in code, "the one atomic is the status word's"
    assert code.count("count_mask(") == 2, "the predicate: defined once, called once"
    assert code.count("<<<") == 4, "two launches of the occupancy, one of the choice, one of the gather"
    rule = open(os.path.join(B.CSRC, "ubr_crop_rule.h")).read()
    assert '#include "ubr_det_rule.h"' in rule and "ubx::philox(" in rule and "0xD2511F53" not in rule, "Philox is included, not copied"
    assert "ubn::choose(" in code and "ubn::row_is_valid(" in code and "hip" not in re.sub(r"//.*", "", rule).replace("__HIPCC__", "").lower()


def test_a_missing_library_is_a_runtime_error(monkeypatch):
    nowhere = os.path.join(REPO, "no_such_dir", "libubresnet_crop.so")
    monkeypatch.setenv("UBN_LIB", nowhere)
    spec = importlib.util.spec_from_file_location("ubresnet_amd._crop_missing", os.path.join(PKG, "_crop.py"))
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert fresh.LIB_PATH == nowhere
    with pytest.raises(RuntimeError, match="is missing; build it with") as e:
        fresh.occupancy(0x1000, None, 0, 0, 0, False, 10.0, 1, 16, 16, 16, 0x2000)
    assert nowhere in str(e.value) and "There is no CPU fallback" in str(e.value)


def test_the_compiled_kernels_are_the_case_table():
    """no allow-list: every compiled kernel is launched by a case of test_gpu_crops_exact.py, and the table names nothing else"""
    H.need_lib(LIB)
    compiled = kernel_symbols.kernels(LIB)
    assert compiled == sorted(R.KERNEL_CASES), (compiled, sorted(R.KERNEL_CASES))
    assert all(R.KERNEL_CASES.values())
    ran = H.case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_crops_exact.py"))
    assert ran == set(R.CASES) == set(i for v in R.KERNEL_CASES.values() for i in v)
    for k, ids in R.KERNEL_CASES.items():
        assert set(ids) & ran, k


def test_the_store_hazard_scan_finds_nothing():
    H.need_lib(LIB)
    spec = importlib.util.spec_from_file_location("check_store_hazard", os.path.join(REPO, "tools", "check_store_hazard.py"))
    hz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hz)
    assert hz.scan(LIB)[1] == []


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


def test_the_addons_entry_lists_the_true_include_closure():
    lib = B.ADDONS["crop"]
    assert isinstance(lib, B.Lib) and lib.sources == [os.path.join("extra", "ubr_crop.hip")] and lib.binding == "_crop"
    assert "crop" not in B.LIBS and "crop" not in B.EXTRAS and list(B.ADDONS)[:3] == ["blend", "sparse", "crop"]
    listed = [os.path.realpath(os.path.join(B.CSRC, h)) for h in lib.headers]
    assert len(listed) == len(set(listed)) and set(listed) == _include_closure([os.path.join(B.CSRC, s) for s in lib.sources])
    for h in (HEADER, os.path.join(B.CSRC, "ubr_crop_rule.h"), os.path.join(B.CSRC, "ubr_det_rule.h"), os.path.join(REPO, "include", "ubresnet_det.h")):
        assert os.path.realpath(h) in listed, h
    assert not set(B.SOURCES + B.HEADERS) & set(lib.sources + lib.headers), "source_hash() covers the network's library only"


def test_a_forced_build_of_crop_is_one_compile_and_one_link(monkeypatch, capsys):
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    capsys.readouterr()
    built = B.build_addons(force=True, only=["crop"])
    monkeypatch.undo()
    lib = B.ADDONS["crop"]
    src, obj = os.path.join(B.CSRC, lib.sources[0]), os.path.join(B.CSRC, "extra", "ubr_crop.o")
    assert built == [lib.out] and len(lines) == 2
    assert lines[0] == [B.HIPCC] + B.FLAGS + ["-c", src, "-o", obj]
    assert lines[1] == [B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib.out, obj]
    io = capsys.readouterr()
    assert io.out == "" and io.err.strip().split("\n") == [" ".join(c) for c in lines]


def test_entry_point_reports_crop_on_stderr_before_the_score_line(monkeypatch, capsys):
    import __graft_entry__ as entry
    for lib in [l for t in (B.LIBS, B.ADDONS, B.EXTRAS) for l in t.values()]:
        H.need_lib(lib.out)
    for f in ("build", "build_addons", "build_extras"):
        monkeypatch.setattr(B, f, lambda *a, **kw: None)
    capsys.readouterr()
    entry.build()
    io = capsys.readouterr()
    err = io.err.strip().split("\n")
    assert "crop" not in io.out and "built %s ABI version 1" % LIB in err
    assert err[-1] == "built %s ABI version 1" % B.EXTRAS["score"].out and err.index("built %s ABI version 1" % LIB) < len(err) - 1
    assert err.index("built %s ABI version 1" % B.ADDONS["sparse"].out) < err.index("built %s ABI version 1" % LIB)


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals: every call below is refused on the host, before any HIP call; the addresses are never dereferenced
# ------------------------------------------------------------------------------------------------------------------------
_P = 0x100000
_OCC = dict(image=_P, label=_P + 0x10000, kind=1, off=0, mask=6, stacked=0, thr=10.0, P=2, rows=32, cols=48, cell=16, sat=_P + 0x40000)
_BAD_OCC = {
    "null image": (dict(image=None), "null pointer (image, sat)"),
    "null sat": (dict(sat=None), "null pointer (image, sat)"),
    "P 0": (dict(P=0), "must be positive"),
    "rows negative": (dict(rows=-32), "must be positive"),
    "P 65": (dict(P=65), "P=65 must be at most 64"),
    "2^31 pixels": (dict(P=2, rows=32768, cols=32768), "below 2^31 pixels"),
    "cell 2": (dict(cell=2), "cell=2 must be a power of two in 4..64"),
    "cell 128": (dict(cell=128), "cell=128 must be a power of two in 4..64"),
    "cell 12": (dict(cell=12), "cell=12 must be a power of two"),
    "cell does not divide rows": (dict(rows=40), "cell=16 must divide rows=40"),
    "cell does not divide cols": (dict(cols=56), "cell=16 must divide rows=32 and cols=56"),
    "too many cells": (dict(cols=4 * 4100, cell=4), "cols / cell = 4100 must be at most 4096"),
    "kind 4": (dict(kind=4), "label_kind=4 must be 0..3"),
    "kind negative": (dict(kind=-1), "label_kind=-1 must be 0..3"),
    "label without kind": (dict(kind=0), "a label needs a kind"),
    "kind without label": (dict(label=None), "a label needs a kind"),
    "image alignment": (dict(image=_P + 2), "image and sat must be 4-byte aligned"),
    "sat alignment": (dict(sat=_P + 0x40001), "image and sat must be 4-byte aligned"),
    "int64 label alignment": (dict(kind=2, label=_P + 0x10004), "label must be 8-byte aligned"),
    "float label alignment": (dict(kind=3, label=_P + 0x10002), "label must be 4-byte aligned"),
    "sat inside image": (dict(sat=_P + 64), "sat overlaps an input"),
    "sat inside label": (dict(sat=_P + 0x10000 + 8), "sat overlaps an input"),
}
_CHOOSE = dict(sat=_P, Q=2, rows=32, cols=48, H=16, W=16, cell=16, planes=None, nplanes=0, K=8, T=3, min_lit=5, lo=1, hi=0, number=0, fr=1, fc=1,
               table=_P + 0x1000)
_BAD_CHOOSE = {
    "null sat": (dict(sat=None), "null pointer (sat, table)"),
    "null table": (dict(table=None), "null pointer (sat, table)"),
    "Q 0": (dict(Q=0), "must be positive"),
    "Q 65": (dict(Q=65), "must be at most 64"),
    "crop larger than the view": (dict(H=48), "must be positive and fit"),
    "W 0": (dict(W=0), "must be positive and fit"),
    "cell 3": (dict(cell=3), "cell=3 must be a power of two"),
    "cell does not divide the slack": (dict(rows=40), "cell=16 must divide H=16, W=16, rows - H=24"),
    "cell does not divide W": (dict(W=24), "cell=16 must divide"),
    "no cell at all": (dict(rows=33, cell=4), "cell=4 must divide"),
    "nplanes 0": (dict(planes=[0], nplanes=0), "nplanes=0 must be 1..Q=2"),
    "nplanes 3": (dict(planes=[0, 1, 1], nplanes=3), "nplanes=3 must be 1..Q=2"),
    "plane out of range": (dict(planes=[0, 2], nplanes=2), "planes must be distinct and in 0..1"),
    "plane negative": (dict(planes=[-1], nplanes=1), "planes must be distinct and in 0..1"),
    "plane twice": (dict(planes=[1, 1], nplanes=2), "planes must be distinct"),
    "K 0": (dict(K=0), "K=0 must be 1..4096"),
    "K 4097": (dict(K=4097), "K=4097 must be 1..4096"),
    "T 0": (dict(T=0), "T=0 must be 1..64"),
    "T 65": (dict(T=65), "T=65 must be 1..64"),
    "min_lit negative": (dict(min_lit=-1), "min_lit=-1 must be >= 0"),
    "sat alignment": (dict(sat=_P + 2), "4-byte aligned"),
    "table alignment": (dict(table=_P + 0x1001), "4-byte aligned"),
    "table inside sat": (dict(table=_P + 16), "table overlaps sat"),
}
_GATHER = dict(image=_P, label=_P + 0x10000, kind=3, off=0, weight=_P + 0x20000, stacked=0, P=2, rows=32, cols=48, H=16, W=16, table=_P + 0x30000,
               K=4, oi=_P + 0x40000, ol=_P + 0x50000, ow=_P + 0x60000, status=_P + 0x70000)
_BAD_GATHER = {
    "null image": (dict(image=None), "null pointer (image, label, table)"),
    "null label": (dict(label=None), "null pointer (image, label, table)"),
    "null table": (dict(table=None), "null pointer (image, label, table)"),
    "null out_image": (dict(oi=None), "null pointer (out_image"),
    "null out_label": (dict(ol=None), "null pointer (out_image"),
    "null out_weight": (dict(ow=None), "null pointer (out_image"),
    "null status": (dict(status=None), "null pointer (out_image"),
    "P 0": (dict(P=0), "must be positive"),
    "2^31 pixels": (dict(P=2, rows=32768, cols=32768), "below 2^31 pixels"),
    "crop larger than the view": (dict(W=52), "must be positive and fit"),
    "H 0": (dict(H=0), "must be positive and fit"),
    "W 18": (dict(W=18), "W=18 must be a multiple of 4"),
    "kind 0": (dict(kind=0), "label_kind=0 must be 1..3"),
    "kind 4": (dict(kind=4), "label_kind=4 must be 1..3"),
    "K 0": (dict(K=0), "K=0 must be 1..4096"),
    "K 4097": (dict(K=4097), "K=4097 must be 1..4096"),
    "image alignment": (dict(image=_P + 1), "4-byte aligned"),
    "weight alignment": (dict(weight=_P + 0x20002), "4-byte aligned"),
    "table alignment": (dict(table=_P + 0x30002), "4-byte aligned"),
    "label alignment": (dict(kind=2, label=_P + 0x10004), "label must be 8-byte aligned"),
    "out_label alignment": (dict(ol=_P + 0x50004), "8-byte aligned"),
    "status alignment": (dict(status=_P + 0x70004), "8-byte aligned"),
    "out_image inside image": (dict(oi=_P + 128), "overlaps an input"),
    "out_weight is table": (dict(ow=_P + 0x30000), "overlaps an input"),
    "status inside label": (dict(status=_P + 0x10008), "overlaps an input"),
    "status inside out_label": (dict(status=_P + 0x50008), "two outputs overlap"),
    "out_weight inside out_image": (dict(ow=_P + 0x40000 + 64), "two outputs overlap"),
}


def _refused(rc, prefix, message, name):
    msg = N.lib().ubn_last_error().decode()
    assert rc == -1 and msg.startswith(prefix + ":") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=prefix):
        N.check(rc, name)


@pytest.mark.parametrize("name", sorted(_BAD_OCC))
def test_occupancy_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD_OCC[name]
    a = dict(_OCC, **change)
    rc = N.lib().ubn_occupancy(a["image"], a["label"], a["kind"], a["off"], a["mask"], a["stacked"], a["thr"], a["P"], a["rows"], a["cols"], a["cell"],
                               a["sat"], None)
    _refused(rc, "ubn_occupancy", message, name)


@pytest.mark.parametrize("name", sorted(_BAD_CHOOSE))
def test_choose_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD_CHOOSE[name]
    a = dict(_CHOOSE, **change)
    planes = None if a["planes"] is None else (N.i32 * len(a["planes"]))(*a["planes"])
    rc = N.lib().ubn_choose(a["sat"], a["Q"], a["rows"], a["cols"], a["H"], a["W"], a["cell"], planes, a["nplanes"], a["K"], a["T"], a["min_lit"],
                            a["lo"], a["hi"], a["number"], a["fr"], a["fc"], a["table"], None)
    _refused(rc, "ubn_choose", message, name)


@pytest.mark.parametrize("name", sorted(_BAD_GATHER))
def test_gather_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD_GATHER[name]
    a = dict(_GATHER, **change)
    rc = N.lib().ubn_gather(a["image"], a["label"], a["kind"], a["off"], a["weight"], a["stacked"], a["P"], a["rows"], a["cols"], a["H"], a["W"],
                            a["table"], a["K"], a["oi"], a["ol"], a["ow"], a["status"], None)
    _refused(rc, "ubn_gather", message, name)


# ------------------------------------------------------------------------------------------------------------------------
# the rule as a program
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/crop_host.cpp has its own main and includes ubr_crop_rule.h; built with -fsanitize=address,undefined and run as a
    process of its own; nothing is preloaded"""
    exe = str(tmp_path_factory.mktemp("crop_host") / "crop_host")
    r = subprocess.run([H.cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "crop_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args, ok=0):
        p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert p.returncode == ok, "sanitizer or program failure:\n" + p.stderr[-2000:]
        return [l.split()[1:] for l in p.stdout.strip().split("\n") if l]
    return run


def test_rule_as_a_program_under_the_host_sanitizers(host_program, tmp_path):
    run = host_program
    assert run("words", 1, 0, 0, 0, 0) == [["3488071712", "2852949502", "2108613644", "1460095574"]]
    rs = np.random.RandomState(5)
    for k0, k1, c0, c1, c2 in rs.randint(0, 2 ** 32, (4, 5), dtype=np.uint64).tolist() + [[2 ** 32 - 1] * 5]:
        assert [int(v) for v in run("words", k0, k1, c0, c1, c2)[0]] == [int(v) for v in det_ref.philox(k0, k1, c0, c1, c2, R.PHILOX_TAG)]
    for rows, cols, Hc, Wc in ((1008, 3456, 512, 512), (1008, 3456, 512, 832), (20, 36, 8, 12), (128, 192, 64, 128), (10, 10, 6, 6), (16, 32, 16, 32)):
        assert int(run("cell", rows, cols, Hc, Wc)[0][0]) == R.largest_cell(rows, cols, Hc, Wc)
    mask = (1 << 31) | 0b0101
    got = run("labels", -1, mask, *[int(b) for b in R.EDGE_LABELS.view(np.uint32)])
    assert [int(g[0]) for g in got] == R.EDGE_LABELS_MINUS_1
    assert [int(g[1]) for g in got] == R.label_counts(np.array(R.EDGE_LABELS_MINUS_1), mask).astype(int).tolist()
    got = run("ints", -1, mask, *R.INT_LABELS.tolist())
    assert [int(g[0]) for g in got] == R.convert_labels(R.INT_LABELS, -1).tolist()
    assert [int(g[1]) for g in got] == R.label_counts(R.convert_labels(R.INT_LABELS, -1), mask).astype(int).tolist()
    own = R.inputs("own-table")
    for stacked in (0, 1):
        for row in own["table"]:
            want = R.row_is_valid(row, stacked, own["P"], own["rows"], own["cols"], own["H"], own["W"])
            assert run("valid", stacked, own["P"], own["rows"], own["cols"], own["H"], own["W"], row[0], row[1], row[2], row[6], row[7]) == [[str(int(want))]]
    # the selection over the tables of the reference, the branch case among them
    for name in ("branch", "other-number", "g4-tails", "stacked", "planes-list", "t64", "k1-t1", "k257", "switches-off", "rows-only", "seed-hi"):
        a = R.inputs(name)
        ref = R.reference(a)
        f = tmp_path / (name + ".txt")
        f.write_text(" ".join(str(int(v)) for v in ref["sat"].reshape(-1)))
        got = run("choose", f, a["Q"], a["rows"], a["cols"], a["H"], a["W"], a["g"], a["K"], a["T"], a["min_lit"], a["seed"] & 0xFFFFFFFF, a["seed"] >> 32,
                  a["number"], int(a["flip_rows"]), int(a["flip_cols"]), *(a["planes"] or []))
        assert np.array_equal(np.array(got, dtype=np.int64), ref["table"]), name
    run("choose", f, 2, 33, 48, 16, 16, 4, 1, 1, 0, 0, 0, 0, 0, 0, ok=1)           # no cell fits: refused


# ------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------------
def test_cell_choice_and_cropper_refusals_without_a_device():
    assert crops.choose_cell(1008, 3456, 512, 512) == 16 and crops.choose_cell(1008, 3456, 512, 832) == 16
    assert crops.choose_cell(20, 36, 8, 12) == 4 and crops.choose_cell(128, 192, 64, 128) == 64 and crops.choose_cell(128, 192, 64, 128, cell=8) == 8
    for bad in ((10, 10, 6, 6), (1008, 3456, 510, 512), (50, 64, 16, 16)):
        with pytest.raises(ValueError, match="no cell"):
            crops.choose_cell(*bad)
    with pytest.raises(ValueError, match="does not fit"):
        crops.choose_cell(16, 16, 32, 16)
    with pytest.raises(ValueError, match="cell=32 does not divide"):
        crops.choose_cell(1008, 3456, 512, 512, cell=32)
    c = crops.EventCropper()
    assert (c.crop, c.per_event, c.min_lit, c.tries, c.classes, c.planes, c.stacked, c.adc_threshold) == ((512, 512), 16, 0, 8, None, None, False, 10.0)
    assert (c.flip_rows, c.flip_cols, c.label_offset, c.seed, c.cell, c.class_mask, c.sat, c.table) == (False, False, 0, 0, None, None, None, None)
    assert c.geometry(3, 1008, 3456) == (3, 16) and crops.EventCropper(stacked=True, crop=(512, 832)).geometry(3, 1008, 3456) == (1, 16)
    assert crops.EventCropper(classes={2, 31}).class_mask == (1 << 31) | 4
    for kw in (dict(crop=512), dict(crop=(0, 16)), dict(crop=(16.0, 16)), dict(per_event=0), dict(per_event=4097), dict(per_event=True), dict(min_lit=-1),
               dict(tries=0), dict(tries=65), dict(classes=[]), dict(classes=[32]), dict(classes=[-1]), dict(planes=[]), dict(planes=[0, 0]),
               dict(planes=[64]), dict(planes=[0], stacked=True), dict(label_offset=2 ** 31), dict(seed=-1), dict(seed=2 ** 64), dict(cell=12),
               dict(cell=2), dict(cell=128), dict(cell=True)):
        with pytest.raises(ValueError, match="EventCropper"):
            crops.EventCropper(**kw)
    c = crops.EventCropper(crop=(16, 32), per_event=4, planes=[0, 2])
    img, lab = torch.zeros((3, 48, 80)), torch.zeros((3, 48, 80), dtype=torch.uint8)
    with pytest.raises(TypeError, match="image must be float32"):
        c(img.double(), lab)
    with pytest.raises(TypeError, match="label must be uint8 / int64 / float32"):
        c(img, lab.int())
    with pytest.raises(TypeError, match="torch tensor or a SparseEvent"):
        c(img.numpy(), lab)
    with pytest.raises(ValueError, match=r"image must be \[planes,rows,cols\]"):
        c(img[0], lab)
    with pytest.raises(ValueError, match="label must be"):
        c(img, lab[0])
    with pytest.raises(ValueError, match="weight must be"):
        c(img, lab, weight=torch.zeros((48, 80)))
    with pytest.raises(ValueError, match="no cell"):
        c(torch.zeros((3, 50, 80)), torch.zeros((3, 50, 80), dtype=torch.uint8))
    with pytest.raises(ValueError, match="names a plane"):
        c(img[:2], lab[:2])
    for bad in (-1, 2 ** 32, 1.0, True):
        with pytest.raises(ValueError, match="number"):
            c(img, lab, number=bad)
    with pytest.raises(TypeError, match="table must be an int32"):
        c(img, lab, table=torch.zeros((4, 8)))
    with pytest.raises(ValueError, match=r"table must be \[K,8\]"):
        c(img, lab, table=torch.zeros((4, 7), dtype=torch.int32))
    with pytest.raises(ValueError, match="label list is for"):
        c(img, sparse.SparseEvent(torch.zeros(0, dtype=torch.int32), torch.zeros(0), 1, 48, 80))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c(img, lab)                                             # every argument is fine: the tensors are on the host
    with pytest.raises(RuntimeError, match="no call yet"):
        c.read()
    s = crops.EventCropper(crop=(16, 32), stacked=True)
    with pytest.raises(ValueError, match=r"label must be \(48, 80\)"):
        s(img, lab)
    assert crops.CropBatch._fields == ("adc", "label", "weight", "table", "status") and crops.LabelledEvent._fields == ("image", "label", "weight")
    assert crops.LabelledEvent(img, lab).weight is None


def test_stager_refusals_and_the_synthetic_event():
    c = crops.EventCropper(crop=(16, 32), per_event=4)
    with pytest.raises(TypeError, match="must be an EventCropper"):
        crops.EventCropStager([], object())
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="events_per_batch"):
            crops.EventCropStager([], c, events_per_batch=bad)
    with pytest.raises(ValueError, match="more than 4096"):
        crops.EventCropStager([], c, events_per_batch=1025)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crops.EventCropStager([], c, device="cpu")
    image, label = synthetic.make_labelled_event(2, 96, 160, 7)
    again = synthetic.make_labelled_event(2, 96, 160, 7)
    assert image.shape == label.shape == (2, 96, 160) and image.dtype == f32 and label.dtype == u8
    assert np.array_equal(image, again[0]) and np.array_equal(label, again[1]) and not np.array_equal(image[0], image[1])
    assert set(np.unique(label).tolist()) <= {0, 1, 2} and ((label > 0) == (image > 0)).all()
    assert np.array_equal(image[1], synthetic.make_crop(96, 160, 8)[0])
