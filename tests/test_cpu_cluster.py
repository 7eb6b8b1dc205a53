"""EventClusters without a GPU: the numpy reference of tests/cluster_ref.py against a brute-force flood fill on tiny views and
against cases written out by hand; libubresnet_cluster.so's header is C99, and header, binding, reference, plan and library agree
on entry points and geometry; the library stands alone and exports its binding's symbols; the ADDONS entry, its include closure
and a forced build; a missing library is a RuntimeError; every argument refusal returns UBI_EINVAL with a message before any HIP
call; the launch plan, the host numbering and a model of the union loop as a stand-alone program under the host sanitizers
(tests/cluster_host.cpp); the refusals of the Python surface that need no device."""
import importlib
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cluster_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ubresnet_amd")
HEADER = os.path.join(REPO, "include", "ubresnet_cluster.h")
import cpu_helpers as H  # noqa: E402
from ubresnet_amd import _cluster as I  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd import clusters  # noqa: E402

LIB = B.ADDONS["cluster"].out
u8, u16 = np.uint8, np.uint16


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def test_reference_by_hand():
    F = R.FILL
    lab = np.array([[[0, F, 1],
                     [F, 1, F],
                     [9, F, F]],
                    [[2, 2, F],
                     [F, F, F],
                     [F, F, 3]]], u8)
    root, foreign = R.roots(lab, 4, F, 8, False)
    assert foreign == 1
    assert root.tolist() == [[[0, -1, 0], [-1, 0, -1], [-1, -1, -1]], [[9, 9, -1], [-1, -1, -1], [-1, -1, 17]]]
    assert R.roots(lab, 4, F, 4, False)[0].tolist() == [[[0, -1, 2], [-1, 4, -1], [-1, -1, -1]], [[9, 9, -1], [-1, -1, -1], [-1, -1, 17]]]
    assert R.roots(lab, 4, F, 8, True)[0].tolist() == [[[0, -1, 2], [-1, 2, -1], [-1, -1, -1]], [[9, 9, -1], [-1, -1, -1], [-1, -1, 17]]]
    conf = np.zeros(lab.shape, u16)
    conf[0, 0, 0], conf[0, 0, 2], conf[0, 1, 1] = 0x3C00, 0x0001, 0x7C00        # 1.0, the smallest subnormal, inf
    conf[1, 0, 0], conf[1, 0, 1], conf[1, 2, 2] = 0x8000, 0xBC00, 0x3800        # -0, -1.0, 0.5
    ids, table, count = R.tabulate(lab, conf, root, 4)
    assert count == 3 and ids.tolist() == [[[0, -1, 0], [-1, 0, -1], [-1, -1, -1]], [[1, 1, -1], [-1, -1, -1], [-1, -1, 2]]]
    assert table.tolist() == [[0, 3, 0, 1, 0, 2, (1 << 24) + 1, 1, 1, 2, 0, 0],
                              [9, 2, 0, 0, 0, 1, 0, 1, 0, 0, 2, 0],
                              [17, 1, 2, 2, 2, 2, 1 << 23, 0, 0, 0, 0, 1]]
    val, bad = R.fix(np.array([0x0000, 0x0001, 0x03FF, 0x0400, 0x3C00, 0x7BFF, 0x8000, 0x8001, 0x7C00, 0x7E00, 0xFC00], u16))
    assert val.tolist() == [0, 1, 1023, 1024, 1 << 24, 2047 << 29, 0, 0, 0, 0, 0]
    assert bad.tolist() == [False] * 7 + [True] * 4


@pytest.mark.parametrize("view", ["1x1x1", "tiny", "wide"])
@pytest.mark.parametrize("pattern", sorted(R.PATTERNS))
def test_reference_against_flood_fill(view, pattern):
    shape = {"1x1x1": (1, 1, 1), "tiny": (2, 7, 9), "wide": (1, 3, R.T_W + 2)}[view]
    lab = R.PATTERNS[pattern](*shape)
    assert lab.dtype == u8 and lab.shape == shape
    for conn, by_class in R.MODES:
        got, _ = R.roots(lab, R.C4, R.FILL, conn, by_class)
        assert (got == R.flood_fill(lab, R.C4, R.FILL, conn, by_class)).all(), (conn, by_class)


def test_the_patterns_are_what_their_names_say():
    P, rows, cols = R.VIEWS["four-tiles"]
    assert (P, rows, cols) == (2, 2 * R.T_H + 3, 2 * R.T_W + 5) and R.VIEWS["one-short"] == (3, R.T_H - 1, R.T_W - 1)
    assert R.VIEWS["row"] == (1, 1, R.T_W + 1) and R.VIEWS["col"] == (1, R.T_H + 1, 1)
    ref = lambda name, conn=8, by_class=False: R.reference(R.PATTERNS[name](P, rows, cols), np.zeros((P, rows, cols), u16), R.C4, R.FILL, conn, by_class)
    assert ref("empty")["count"] == 0 and ref("all-lit")["count"] == P and ref("all-lit")["table"][:, 1].tolist() == [rows * cols] * P
    assert ref("checker")["count"] == P and ref("checker", 4)["count"] == P * ((rows * cols + 1) // 2)
    serp = ref("serpentine")
    assert serp["count"] == P and serp["table"][:, 0].tolist() == [0, rows * cols] and ref("serpentine", 4)["count"] == P
    u = ref("u")
    assert u["count"] == P and (R.PATTERNS["u"](P, rows, cols)[:, :rows - 1, 2] == R.FILL).all(), "the arms join in the last row only"
    assert ref("corner")["count"] == 2 and ref("corner", 4)["count"] == 4
    corner = R.PATTERNS["corner"](P, rows, cols)
    assert corner[0, R.T_H - 1, R.T_W - 1] == 1 and corner[0, R.T_H, R.T_W] == 1 and corner[1, R.T_H - 1, R.T_W] == 2 and corner[1, R.T_H, R.T_W - 1] == 2
    assert ref("row-wrap")["count"] == 2 * P and ref("plane-wrap")["count"] == 2 * P
    assert ref("stripes")["count"] == P and ref("stripes", 8, True)["count"] == P * -(-cols // 3)
    assert ref("foreign")["foreign"] > 100 and ref("diagonal")["count"] >= P
    lit = [float(R.lit_mask(R.PATTERNS["random-%d" % pc](P, rows, cols), R.C4, R.FILL).mean()) for pc in (1, 41, 59, 90)]
    assert all(abs(l - pc / 100.0) < 0.02 for l, pc in zip(lit, (1, 41, 59, 90)))
    bits = set(R.confidence_bits((P, rows, cols)).reshape(-1).tolist())
    assert {0x0001, 0x03FF, 0x8000, 0x8001, 0xBC00, 0x7C00, 0xFC00, 0x7E00, 0xFFFF} <= bits


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_cluster.h"\n'
                     'int main(void) {\n'
                     '  int64_t (*b)(int, int, int) = ubi_scratch_bytes;\n'
                     '  int (*l)(const uint8_t*, int, int, int, int, int32_t*, unsigned long long*, int, int, int, void*) = ubi_label;\n'
                     '  int (*t)(const uint8_t*, const uint16_t*, const int32_t*, int, int, int32_t*, long long*, int64_t,\n'
                     '           unsigned long long*, void*, int, int, int, void*) = ubi_tabulate;\n'
                     '  int (*g)(const int32_t*, const int32_t*, const unsigned long long*, int64_t, int32_t*, int64_t, void*) = ubi_gather_ids;\n'
                     '  const char* (*e)(void) = ubi_last_error;\n'
                     '  int (*v)(void) = ubi_version;\n'
                     '  return b == 0 || l == 0 || t == 0 || g == 0 || e == 0 || v == 0 || UBI_OK != 0 || UBI_EINVAL != -1 || UBI_ELAUNCH != -2\n'
                     '         || UBI_TILE_W + UBI_TILE_H > UBI_BORDER_LANES;\n}\n')
    r = subprocess.run([H.cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(ubi_[a-z_0-9]+)\s*\(", text)
    assert declared == I.SYMBOLS == ["ubi_scratch_bytes", "ubi_label", "ubi_tabulate", "ubi_gather_ids", "ubi_last_error", "ubi_version"]
    names = "TILE_H|TILE_W|LANES|BORDER_LANES|PIXEL_BLOCK|SCAN_WIDTH|MAX_GRID|MAX_CLASSES|TABLE_FIXED"
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBI_(%s)\s+(\d+)" % names, text)}
    assert geometry == {k: getattr(I, k) for k in names.split("|")}
    assert (R.TILE_H, R.TILE_W, R.PIXEL_BLOCK, R.TABLE_FIXED) == (I.TILE_H, I.TILE_W, I.PIXEL_BLOCK, I.TABLE_FIXED)
    assert len(I.COLUMNS) == I.TABLE_FIXED and "{%s, n_0 .. n_{C-1}}" % ", ".join(I.COLUMNS) in raw
    for phrase in ("ADDED to", "STORED", "are not written", "ascending root order", "smallest pixel index", "no spinning",
                   "strictly decreases", "does not wrap", "Every element"):
        assert phrase in raw, phrase
    # fix(h) is that of ubresnet_score.h
    rule = "a subnormal is its mantissa m, a normal is"
    assert rule in raw and rule in " ".join(open(os.path.join(REPO, "include", "ubresnet_score.h")).read().split()).replace("* ", "")
    H.need_lib(LIB)
    assert I.lib().ubi_version() == I.BINDING.version() == 1


def test_library_stands_alone_and_exports_exactly_its_bindings_symbols():
    bd = I.BINDING
    assert bd.prefix == "ubi" and bd.path == LIB and os.path.basename(LIB) == "libubresnet_cluster.so" and os.path.dirname(LIB) == PKG
    assert bd.symbols[-2:] == ["ubi_last_error", "ubi_version"]
    assert (I.LIB_PATH, I.SYMBOLS, I.lib, I.check) == (bd.path, bd.symbols, bd.lib, bd.check)
    H.need_lib(LIB)
    assert "libubresnet_" not in H.readelf("-d", LIB).replace("libubresnet_cluster", "")
    assert sorted(n for n in H.defined_symbols(LIB) if re.match(r"ub[a-z]_", n)) == sorted(bd.symbols)
    tables = [t for t in (B.LIBS, B.EXTRAS, B.ADDONS)]
    others = [importlib.import_module("ubresnet_amd." + lib.binding).BINDING.prefix for t in tables for n, lib in t.items() if n != "cluster"]
    assert "ubi" not in others and len(set(others)) == len(others)
    tree = open(os.path.join(PKG, "_cluster.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy)", tree, flags=re.M) and "from ._binding import Binding" in tree
    src = open(os.path.join(B.CSRC, B.ADDONS["cluster"].sources[0])).read()
    assert '#include "../ubr_sat.h"' in src and '#include "../ubr_cluster_plan.h"' in src and "SAT_EXPORTS(ubi, UBI_VERSION)" in src
    assert "ubr_sparse_plan.h" not in re.sub(r"//.*", "", src) and "asm" not in re.sub(r"//.*", "", src)
    assert "Malloc" not in src and "hipFree" not in src and "Synchronize" not in src, "no allocation, free or sync"
    code = re.sub(r"//.*", "", src)
    assert "cooperative" not in code.lower() and "while (true)" not in code and "__threadfence" not in code
    assert code.count("is_lit(") == 5, "the lit test: defined once; the local pass, the border pass (twice) and the tally call it"
    # the plan compiles without HIP: it reaches the shared scan plan and nothing else, and neither file names HIP outside comments
    plan, shared = os.path.join(B.CSRC, "ubr_cluster_plan.h"), os.path.join(B.CSRC, "ubr_scan_plan.h")
    assert _include_closure([plan]) == {os.path.realpath(shared)} and _include_closure([shared]) == set()
    for f in (plan, shared):
        assert "hip" not in re.sub(r"//.*", "", open(f).read()).lower(), f
    assert re.findall(r"#\s*include\s*<([^>]+)>", open(plan).read() + open(shared).read()) == ["stdint.h"]


def test_a_missing_library_is_a_runtime_error(monkeypatch):
    nowhere = os.path.join(REPO, "no_such_dir", "libubresnet_cluster.so")
    monkeypatch.setenv("UBI_LIB", nowhere)
    spec = importlib.util.spec_from_file_location("ubresnet_amd._cluster_missing", os.path.join(PKG, "_cluster.py"))
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert fresh.LIB_PATH == nowhere
    for call in (lambda: fresh.label(0x1000, 4, 255, 8, False, 0x2000, 0x3000, 1, 2, 2), lambda: fresh.scratch_bytes(1, 2, 2),
                 lambda: fresh.gather_ids(0x1000, 0x2000, 0x3000, 4, 0x4000, 16)):
        with pytest.raises(RuntimeError, match="is missing; build it with") as e:
            call()
        assert nowhere in str(e.value) and "There is no CPU fallback" in str(e.value)


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
    lib = B.ADDONS["cluster"]
    assert isinstance(lib, B.Lib) and lib.sources == [os.path.join("extra", "ubr_cluster.hip")] and lib.binding == "_cluster"
    assert "cluster" not in B.LIBS and "cluster" not in B.EXTRAS and list(B.ADDONS)[:5] == ["blend", "sparse", "crop", "calib", "cluster"]
    listed = [os.path.realpath(os.path.join(B.CSRC, h)) for h in lib.headers]
    assert len(listed) == len(set(listed)) and set(listed) == _include_closure([os.path.join(B.CSRC, s) for s in lib.sources])
    assert os.path.realpath(HEADER) in listed and os.path.realpath(os.path.join(B.CSRC, "ubr_cluster_plan.h")) in listed
    assert os.path.realpath(os.path.join(B.CSRC, "ubr_sparse_plan.h")) not in listed
    assert not set(B.SOURCES + B.HEADERS) & set(lib.sources + lib.headers), "source_hash() covers the network's library only"


def test_a_forced_build_of_cluster_is_one_compile_and_one_link(monkeypatch, capsys):
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    capsys.readouterr()
    built = B.build_addons(force=True, only=["cluster"])
    monkeypatch.undo()
    lib = B.ADDONS["cluster"]
    src, obj = os.path.join(B.CSRC, lib.sources[0]), os.path.join(B.CSRC, "extra", "ubr_cluster.o")
    assert built == [lib.out] and len(lines) == 2
    assert "-ffp-contract=off" in B.FLAGS and lines[0] == [B.HIPCC] + B.FLAGS + ["-c", src, "-o", obj]
    assert lines[1] == [B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib.out, obj]
    io = capsys.readouterr()
    assert io.out == "" and io.err.strip().split("\n") == [" ".join(c) for c in lines]


def test_entry_point_reports_cluster_on_stderr_before_the_score_line(monkeypatch, capsys):
    import __graft_entry__ as entry
    for lib in [l for t in (B.LIBS, B.ADDONS, B.EXTRAS) for l in t.values()]:
        H.need_lib(lib.out)
    for f in ("build", "build_addons", "build_extras"):
        monkeypatch.setattr(B, f, lambda *a, **kw: None)
    capsys.readouterr()
    entry.build()
    io = capsys.readouterr()
    err = io.err.strip().split("\n")
    assert "cluster" not in io.out and "built %s ABI version 1" % LIB in err
    assert err.index("built %s ABI version 1" % B.ADDONS["calib"].out) < err.index("built %s ABI version 1" % LIB) < len(err) - 1
    assert err[-1] == "built %s ABI version 1" % B.EXTRAS["score"].out


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals: every call below is refused on the host, before any HIP call; the addresses are never dereferenced
# ------------------------------------------------------------------------------------------------------------------------
_P = 0x100000
_LABEL = dict(label=_P, C=4, fill=255, conn=8, by_class=0, root=_P + 0x1000, status=_P + 0x2000, P=2, rows=3, cols=5)
_BAD_LABEL = {
    "null label": (dict(label=None), "null pointer (label, root, status)"),
    "null root": (dict(root=None), "null pointer (label, root, status)"),
    "null status": (dict(status=None), "null pointer (label, root, status)"),
    "C 0": (dict(C=0), "C=0 must be 1..16"),
    "C 17": (dict(C=17), "C=17 must be 1..16"),
    "fill 256": (dict(fill=256), "fill_label=256 must be 0..255"),
    "fill negative": (dict(fill=-1), "fill_label=-1 must be 0..255"),
    "connectivity 6": (dict(conn=6), "connectivity=6 must be 4 or 8"),
    "connectivity 0": (dict(conn=0), "connectivity=0 must be 4 or 8"),
    "by_class 2": (dict(by_class=2), "by_class=2 must be 0 or 1"),
    "P 0": (dict(P=0), "must be positive"),
    "rows negative": (dict(rows=-3), "must be positive"),
    "cols 0": (dict(cols=0), "must be positive"),
    "2^31 pixels": (dict(P=2, rows=32768, cols=32768), "below 2^31 pixels"),
    "far too large": (dict(P=1 << 20, rows=1 << 20, cols=1 << 20), "below 2^31 pixels"),
    "root alignment": (dict(root=_P + 0x1002), "4-byte aligned"),
    "status alignment": (dict(status=_P + 0x2004), "8-byte aligned"),
    "root is label": (dict(root=_P), "overlap"),
    "status inside root": (dict(status=_P + 0x1000 + 8), "overlap"),
}
_TAB = dict(label=_P, conf=_P + 0x1000, root=_P + 0x2000, C=4, fill=255, ids=_P + 0x3000, table=_P + 0x4000, capacity=30,
            count=_P + 0x8000, scratch=_P + 0x9000, P=2, rows=3, cols=5)
_BAD_TAB = {
    "null label": (dict(label=None), "null pointer (label, confidence, root)"),
    "null confidence": (dict(conf=None), "null pointer (label, confidence, root)"),
    "null root": (dict(root=None), "null pointer (label, confidence, root)"),
    "null ids": (dict(ids=None), "null pointer (ids, table, count)"),
    "null table": (dict(table=None), "null pointer (ids, table, count)"),
    "null count": (dict(count=None), "null pointer (ids, table, count)"),
    "null scratch": (dict(scratch=None), "null pointer (scratch)"),
    "C 0": (dict(C=0), "C=0 must be 1..16"),
    "C 17": (dict(C=17), "C=17 must be 1..16"),
    "fill 256": (dict(fill=256), "fill_label=256 must be 0..255"),
    "capacity 0": (dict(capacity=0), "capacity=0 must be >= 1"),
    "capacity negative": (dict(capacity=-5), "capacity=-5 must be >= 1"),
    "P 0": (dict(P=0), "must be positive"),
    "2^31 pixels": (dict(P=2, rows=32768, cols=32768), "below 2^31 pixels"),
    "confidence alignment": (dict(conf=_P + 0x1001), "2-byte"),
    "root alignment": (dict(root=_P + 0x2002), "4-byte"),
    "ids alignment": (dict(ids=_P + 0x3002), "4-byte"),
    "table alignment": (dict(table=_P + 0x4004), "8-byte"),
    "count alignment": (dict(count=_P + 0x8004), "8-byte"),
    "scratch alignment": (dict(scratch=_P + 0x9008), "scratch must be 16-byte aligned"),
    "ids is root": (dict(ids=_P + 0x2000), "overlaps an input"),
    "table inside confidence": (dict(table=_P + 0x1008), "overlaps an input"),
    "count inside ids": (dict(count=_P + 0x3000 + 112), "two outputs overlap"),
    "scratch inside table": (dict(scratch=_P + 0x4000 + 16), "two outputs overlap"),
}
_GATHER = dict(ids=_P, index=_P + 0x1000, count=_P + 0x2000, capacity=8, out=_P + 0x3000, pixels=30)
_BAD_GATHER = {
    "null ids": (dict(ids=None), "null pointer"),
    "null index": (dict(index=None), "null pointer"),
    "null count": (dict(count=None), "null pointer"),
    "null out": (dict(out=None), "null pointer"),
    "capacity 0": (dict(capacity=0), "list_capacity=0 must be in 1..2^31-1"),
    "capacity 2^31": (dict(capacity=1 << 31), "must be in 1..2^31-1"),
    "pixels 0": (dict(pixels=0), "pixels=0 must be in 1..2^31-1"),
    "pixels 2^31": (dict(pixels=1 << 31), "must be in 1..2^31-1"),
    "index alignment": (dict(index=_P + 0x1002), "4-byte aligned"),
    "count alignment": (dict(count=_P + 0x2004), "8-byte aligned"),
    "out is index": (dict(out=_P + 0x1000), "out overlaps an input"),
    "out inside ids": (dict(out=_P + 64), "out overlaps an input"),
}


def _refused(rc, prefix, message, name):
    msg = I.lib().ubi_last_error().decode()
    assert rc == -1 and msg.startswith(prefix + ":") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=prefix):
        I.check(rc, name)


@pytest.mark.parametrize("name", sorted(_BAD_LABEL))
def test_label_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD_LABEL[name]
    a = dict(_LABEL, **change)
    rc = I.lib().ubi_label(a["label"], a["C"], a["fill"], a["conn"], a["by_class"], a["root"], a["status"], a["P"], a["rows"], a["cols"], None)
    _refused(rc, "ubi_label", message, name)


@pytest.mark.parametrize("name", sorted(_BAD_TAB))
def test_tabulate_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD_TAB[name]
    a = dict(_TAB, **change)
    rc = I.lib().ubi_tabulate(a["label"], a["conf"], a["root"], a["C"], a["fill"], a["ids"], a["table"], a["capacity"], a["count"],
                              a["scratch"], a["P"], a["rows"], a["cols"], None)
    _refused(rc, "ubi_tabulate", message, name)


@pytest.mark.parametrize("name", sorted(_BAD_GATHER))
def test_gather_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD_GATHER[name]
    a = dict(_GATHER, **change)
    rc = I.lib().ubi_gather_ids(a["ids"], a["index"], a["count"], a["capacity"], a["out"], a["pixels"], None)
    _refused(rc, "ubi_gather_ids", message, name)


def test_scratch_bytes_follow_the_plan():
    H.need_lib(LIB)
    for image in sorted(R.VIEWS.values()) + [(3, 1008, 3456), (3, 200, 700)]:
        blocks = -(-(image[0] * image[1] * image[2]) // I.PIXEL_BLOCK)
        assert I.scratch_bytes(*image) == 4 * (-(-blocks // 4) * 4), image
    assert I.lib().ubi_scratch_bytes(2, 32768, 32768) == 0 and b"below 2^31 pixels" in I.lib().ubi_last_error()
    with pytest.raises(RuntimeError, match="ubi_scratch_bytes"):
        I.scratch_bytes(0, 4, 4)


# ------------------------------------------------------------------------------------------------------------------------
# the plan, the numbering and the union loop as a program
# ------------------------------------------------------------------------------------------------------------------------
def test_plan_and_union_model_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/cluster_host.cpp has its own main and includes ubr_cluster_plan.h; built with -fsanitize=address,undefined and run as
    a process of its own over every view of the GPU tests: the plan's numbers and scratch layout, count / scan / number restated
    on the host against brute force with buffers of exactly the planned sizes, and a sequential model of the union loop on
    adversarial forests (long chains; other unions landing between any two of its memory operations): it ends within its bound
    and leaves every component rooted at its smallest member"""
    exe = str(tmp_path / "cluster_host")
    r = subprocess.run([H.cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "cluster_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    images = sorted(R.VIEWS.values()) + [(3, 200, 700)]
    p = subprocess.run([exe] + [str(v) for im in images for v in im], capture_output=True, text=True)
    assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
    rows = [[int(v) for v in l.split()[1:]] for l in p.stdout.strip().split("\n") if l.startswith("I ")]
    assert [tuple(r[:3]) for r in rows] == images
    for P, rows_, cols, pixels, ty, tx, tiles, blocks, trips, sbytes in rows:
        assert pixels == P * rows_ * cols and (ty, tx) == (-(-rows_ // I.TILE_H), -(-cols // I.TILE_W)) and tiles == P * ty * tx
        assert blocks == -(-pixels // I.PIXEL_BLOCK) and trips == -(-blocks // I.SCAN_WIDTH) and sbytes == 4 * (-(-blocks // 4) * 4)
    by_image = {tuple(r[:3]): r for r in rows}
    assert by_image[R.VIEWS["four-tiles"]][4:7] == [3, 3, 18] and by_image[R.VIEWS["one-short"]][4:7] == [1, 1, 3]
    assert by_image[R.VIEWS["row"]][4:7] == [1, 2, 2] and by_image[R.VIEWS["col"]][4:7] == [2, 1, 2]
    assert p.stdout.strip().split("\n")[-1].split() == ["G"] + [str(v) for v in (I.TILE_H, I.TILE_W, I.LANES, I.BORDER_LANES, I.PIXEL_BLOCK,
                                                                                 I.SCAN_WIDTH, I.MAX_GRID)]


# ------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------------
def test_clusterer_refusals_without_a_device():
    good = dict(planes=2, rows=3, cols=5, num_classes=4, connectivity=8, by_class=False, fill_label=255, capacity=8, device="cpu")
    for bad, match in ((dict(planes=0), "planes"), (dict(rows=-1), "rows"), (dict(cols=2.0), "cols"), (dict(planes=True), "planes"),
                       (dict(num_classes=0), "num_classes"), (dict(num_classes=17), "num_classes"), (dict(fill_label=256), "fill_label"),
                       (dict(capacity=0), "capacity"), (dict(capacity=1.5), "capacity"), (dict(connectivity=6), "connectivity must be 4 or 8"),
                       (dict(by_class=1), "by_class must be a bool"), (dict(planes=2, rows=32768, cols=32768), "int32 pixel index")):
        with pytest.raises(ValueError, match=match):
            clusters.EventClusterer(**dict(good, **bad))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clusters.EventClusterer(**good)                          # every argument is fine: the device is the host


def test_clusters_read_and_table_without_a_device():
    table = torch.zeros((2, 12), dtype=torch.int64)
    table[0] = torch.tensor([0, 3, 0, 1, 0, 2, (1 << 24) + (1 << 23), 1, 1, 2, 0, 0])
    table[1] = torch.tensor([17, 1, 2, 2, 2, 2, 0, 1, 0, 0, 0, 1])
    ids = torch.full((2, 3, 3), -1, dtype=torch.int32)
    found = clusters.Clusters(ids, ids.clone(), table, torch.tensor([5]), torch.zeros(1, dtype=torch.int64))
    assert found.capacity == 2 and clusters.Clusters._fields == ("ids", "root", "table", "count", "status")
    with pytest.raises(OverflowError, match="5 clusters, capacity 2"):
        found.read()
    tab = found._replace(count=torch.tensor([2])).read()
    assert len(tab) == 2 and tab.total == 2 and tab.plane.tolist() == [0, 1] and tab.pixels.tolist() == [3, 1] and tab.root.tolist() == [0, 17]
    assert tab.bbox.tolist() == [[0, 1, 0, 2], [2, 2, 2, 2]] and tab.class_counts.tolist() == [[1, 2, 0, 0], [0, 0, 0, 1]]
    assert tab.fractions().tolist() == [[1 / 3, 2 / 3, 0, 0], [0, 0, 0, 1]]
    mean = tab.mean_confidence()
    assert float(mean[0]) == 0.75 and bool(torch.isnan(mean[1]))
    big = found._replace(count=torch.tensor([2])).read(min_pixels=2)
    assert len(big) == 1 and big.total == 2 and big.pixels.tolist() == [3]
    assert len(found._replace(count=torch.tensor([1])).read()) == 1
    with pytest.raises(ValueError, match="min_pixels"):
        found.read(min_pixels=-1)


def test_of_pixels_refusals_without_a_device():
    from ubresnet_amd import sparse
    ids = torch.full((1, 3, 5), -1, dtype=torch.int32)
    found = clusters.Clusters(ids, ids.clone(), torch.zeros((2, 12), dtype=torch.int64), torch.tensor([0]), torch.zeros(1, dtype=torch.int64))
    pl = sparse.PixelList(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.uint8), torch.zeros(2, dtype=torch.float16),
                          torch.tensor([1]), None, 1, 3, 5, 255)
    with pytest.raises(TypeError, match="1-D int32"):
        clusters.of_pixels(found, pl._replace(index=pl.index.long()))
    with pytest.raises(ValueError, match="1 x 3 x 6 image"):
        clusters.of_pixels(found, pl._replace(cols=6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clusters.of_pixels(found, pl)
