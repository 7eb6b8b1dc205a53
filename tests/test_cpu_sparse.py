"""Sparse event I/O without a GPU: the numpy references of tests/sparse_ref.py against cases written out by hand; libubresnet_sparse.so's
header is C99, header, binding, reference, plan and library agree on entry points and geometry; the compiled kernels are exactly
those the GPU module's case table runs; the library stands alone and exports its binding's symbols; the ADDONS entry and a forced
build; every argument refusal returns UBZ_EINVAL with a message before any HIP call; the launch plan and a host restatement of
count / scan / write as a stand-alone program under the host sanitizers (tests/sparse_host.cpp), and the shared scan plan
beneath it as another (tests/scan_host.cpp); the refusals of the Python surface that need no device."""
import ctypes as C
import importlib
import importlib.util
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sparse_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ubresnet_amd")
HEADER = os.path.join(REPO, "include", "ubresnet_sparse.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
import cpu_helpers as H  # noqa: E402
from ubresnet_amd import _sparse as Z  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd import deploy, sparse  # noqa: E402

LIB = B.ADDONS["sparse"].out
u8, u16, u32, i32 = np.uint8, np.uint16, np.uint32, np.int32


# ------------------------------------------------------------------------------------------------------------------------
# the references by hand
# ------------------------------------------------------------------------------------------------------------------------
def test_reference_scatter_by_hand():
    idx = np.array([1, 4, 4, 3, 6, 9, -1, 2], i32)             # 4 again: equal; 3: descending; 9: out of range; -1: low; 2 > -1: valid
    val = np.arange(10, 18).astype(u32)
    view, status, named = R.scatter_view(idx, val, None, 8, 100)
    assert status == 104 and view.tolist() == [0, 10, 17, 0, 11, 0, 14, 0]
    assert named.tolist() == [False, True, True, True, True, False, True, False]
    view, status, _ = R.scatter_view(idx, val, 2, 8, 0)        # a device count below n
    assert status == 0 and view.tolist() == [0, 10, 0, 0, 11, 0, 0, 0]
    assert R.scatter_view(idx, val, 99, 8, 0)[1] == 4           # and above it: n entries
    view, status, named = R.scatter_view(np.zeros(0, i32), np.zeros(0, u32), None, 3, 5)
    assert status == 5 and view.tolist() == [0, 0, 0] and not named.any()
    assert R.valid_entries(np.array([0], i32), 1, 1).tolist() == [True] and R.valid_entries(np.array([1], i32), 1, 1).tolist() == [False]


def test_reference_expand_and_compact_by_hand():
    lab, conf, status, named = R.expand(np.array([0, 2, 2, 5], i32), np.array([9, 8, 7, 6], u8), np.array([1, 2, 3, 4], u16), None, 255, 5, 0)
    assert lab.tolist() == [9, 255, 8, 255, 255] and conf.tolist() == [1, 0, 2, 0, 0] and status == 2 and named.tolist() == [True, False, True, False, False]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    adc = np.array([[[10.0, np.nextafter(np.float32(10), inf), nan, inf, -inf, 9.0]]], np.float32)
    assert R.lit_mask(adc, 1, 10.0, 1, 1, 6).tolist() == [False, True, False, True, False, False]
    # two planes of one pixel row stacked: lit where either is above
    adc2 = np.array([[[0.0, 11.0, nan]], [[12.0, nan, nan]]], np.float32)
    assert R.lit_mask(adc2, 2, 10.0, 1, 1, 3).tolist() == [True, True, False]
    assert R.lit_mask(None, 1, 10.0, 2, 1, 2).all()
    label, cbits = np.array([1, 2, 3, 4, 5, 6], u8), np.array([10, 20, 30, 40, 50, 60], u16)
    oi, ol, oc = np.full(4, -7, i32), np.full(4, 77, u8), np.full(4, 777, u16)
    assert R.compact(label, cbits, adc, 1, 10.0, 1, 1, 6, oi, ol, oc) == 2
    assert oi.tolist() == [1, 3, -7, -7] and ol.tolist() == [2, 4, 77, 77] and oc.tolist() == [20, 40, 777, 777]
    oi, ol, oc = np.full(1, -7, i32), np.full(1, 77, u8), np.full(1, 777, u16)           # overflow: the total, the first entry only
    assert R.compact(label, cbits, adc, 1, 10.0, 1, 1, 6, oi, ol, oc) == 2 and oi.tolist() == [1]


def test_the_cases_cover_what_they_must():
    B_, S_ = R.B, R.S
    sizes = {R.pixels_of(c["image"]) for c in R.CASES.values() if c["call"] == "compact"}
    assert {1, B_ - 1, B_, B_ + 1, S_ * B_} <= sizes
    assert -(-R.pixels_of(R.IMG_SP1) // B_) == S_ + 1 and max(sizes) == R.pixels_of(R.IMG_SP1) <= 8 << 20
    assert {c["image"][2] for c in R.CASES.values()} == {1, 3, 61, 67}
    assert all(c["image"][1] * c["image"][2] % 4 for c in R.CASES.values() if c["image"][2] in (61, 67)), "a plane that is 16-byte aligned"
    assert {c["image"][0] for c in R.CASES.values()} == {1, 3} and R.CASES["c-stacked"]["vplanes"] == 3 and R.CASES["c-stacked"]["image"][0] == 1
    assert {c["occ"] for c in R.CASES.values() if c["call"] == "compact"} >= {"dark", "all", "first", "last", "wave", "checker", "random", "blocks", "rule"}
    assert {c["cap"] for c in R.CASES.values() if c["call"] == "compact"} == {"total", "total-1", 1}
    short = R.compact_inputs("c-cap-short")
    assert short["capacity"] == short["total"] - 1 > 1 and R.compact_inputs("c-cap-1")["total"] > 1
    assert R.compact_inputs("c-all-dark")["total"] == 0 and R.compact_inputs("c-null-adc")["adc"] is None
    wave = R.compact_inputs("c-per-wave")["lit"]
    per = np.add.reduceat(wave, np.arange(0, len(wave), 256))
    assert (per[:-1] == 1).all() and len(set(np.flatnonzero(wave) % 256)) > 20
    rule = R.compact_inputs("c-lit-rule")["adc"].reshape(-1)
    assert (rule == R.THR).any() and np.isnan(rule).any() and np.isposinf(rule).any() and np.isneginf(rule).any()
    assert (rule == np.nextafter(R.THR, np.float32(np.inf))).any()
    for name in ("s-invalid", "e-invalid"):
        a = R.list_inputs(name)
        n = R.pixels_of(a["image"])
        ok = R.valid_entries(a["index"], len(a["index"]), n)
        assert (~ok).sum() == 9 and a["status0"] > 0 and a["index"].min() < 0 and a["index"].max() >= n
        assert (np.diff(a["index"].astype(np.int64)) == 0).any() and (np.diff(a["index"].astype(np.int64)) < 0).any()
    for name in ("s-stride", "e-stride"):
        assert len(R.list_inputs(name)["index"]) > R.MAX_GRID * R.LANES, "no second trip of the scatter's grid"
    assert 4 * R.pixels_of(R.IMG_FILL) // 16 > R.MAX_GRID * R.LANES, "no second trip of the fill's grid"
    ends = R.list_inputs("s-ends")
    assert ends["index"][0] == 0 and ends["index"][-1] == R.pixels_of(ends["image"]) - 1 and ends["offset"] == 1
    assert {0x80000000, 0x00000001, 0x7FC12345, 0x7F800000} <= set(ends["value"].tolist())
    small, large = R.list_inputs("s-count-small"), R.list_inputs("s-count-large")
    assert 0 < small["count"] < len(small["index"]) and large["count"] > len(large["index"])
    assert R.list_inputs("s-random")["status0"] > 0 and len(R.list_inputs("s-empty")["index"]) == 0


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_sparse.h"\n'
                     'int main(void) {\n'
                     '  int (*s)(const int32_t*, const float*, int64_t, const unsigned long long*, float*, int, int, int,\n'
                     '           unsigned long long*, void*) = ubz_scatter_view;\n'
                     '  int64_t (*b)(int, int, int) = ubz_compact_scratch_bytes;\n'
                     '  int (*c)(const uint8_t*, const uint16_t*, const float*, int, float, int, int, int, int64_t, int32_t*, uint8_t*,\n'
                     '           uint16_t*, unsigned long long*, void*, int64_t, void*) = ubz_compact;\n'
                     '  int (*x)(const int32_t*, const uint8_t*, const uint16_t*, int64_t, const unsigned long long*, int, uint8_t*,\n'
                     '           uint16_t*, int, int, int, unsigned long long*, void*) = ubz_expand;\n'
                     '  const char* (*e)(void) = ubz_last_error;\n'
                     '  int (*v)(void) = ubz_version;\n'
                     '  return s == 0 || b == 0 || c == 0 || x == 0 || e == 0 || v == 0 || UBZ_OK != 0 || UBZ_EINVAL != -1 || UBZ_ELAUNCH != -2\n'
                     '         || UBZ_PIXEL_BLOCK != UBZ_LANES * UBZ_LANE_PIXELS;\n}\n')
    r = subprocess.run([H.cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(ubz_[a-z_0-9]+)\s*\(", text)
    assert declared == Z.SYMBOLS == ["ubz_scatter_view", "ubz_compact_scratch_bytes", "ubz_compact", "ubz_expand", "ubz_last_error", "ubz_version"]
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBZ_(LANES|LANE_PIXELS|PIXEL_BLOCK|SCAN_WIDTH|MAX_GRID|MAX_VPLANES)\s+(\d+)", text)}
    assert geometry == dict(LANES=Z.LANES, LANE_PIXELS=Z.LANE_PIXELS, PIXEL_BLOCK=Z.PIXEL_BLOCK, SCAN_WIDTH=Z.SCAN_WIDTH, MAX_GRID=Z.MAX_GRID,
                            MAX_VPLANES=Z.MAX_VPLANES)
    assert (R.LANES, R.LANE_PIXELS, R.PIXEL_BLOCK, R.SCAN_WIDTH, R.MAX_GRID) == (Z.LANES, Z.LANE_PIXELS, Z.PIXEL_BLOCK, Z.SCAN_WIDTH, Z.MAX_GRID)
    assert Z.SCAN_WIDTH * Z.PIXEL_BLOCK <= 8 << 20
    # the lit test is that of ubresnet_post.h, word for word
    rule = "lit    <=> adc == NULL, or max over v < vplanes of adc[plane*vplanes + v][oy][ox] > adc_threshold (strict; NaN is not lit)"
    assert rule in raw and rule in open(os.path.join(REPO, "include", "ubresnet_post.h")).read()
    for phrase in ("raw predecessor", "ADDED to status[0]", "STORED", "are not written", "ascending pixel-index order", "No atomic",
                   "no workgroup waits for another", "same predicate function"):
        assert phrase in raw, phrase
    H.need_lib(LIB)
    assert Z.lib().ubz_version() == Z.BINDING.version() == 1


def test_library_stands_alone_and_exports_exactly_its_bindings_symbols():
    bd = Z.BINDING
    assert bd.prefix == "ubz" and bd.path == LIB and os.path.basename(LIB) == "libubresnet_sparse.so" and os.path.dirname(LIB) == PKG
    assert bd.symbols[-2:] == ["ubz_last_error", "ubz_version"]
    assert (Z.LIB_PATH, Z.SYMBOLS, Z.lib, Z.check) == (bd.path, bd.symbols, bd.lib, bd.check)
    H.need_lib(LIB)
    assert "libubresnet_" not in H.readelf("-d", LIB).replace("libubresnet_sparse", "")
    assert sorted(n for n in H.defined_symbols(LIB) if re.match(r"ub[a-z]_", n)) == sorted(bd.symbols)
    tables = [t for t in (B.LIBS, B.EXTRAS, B.ADDONS)]
    others = [importlib.import_module("ubresnet_amd." + lib.binding).BINDING.prefix for t in tables for n, lib in t.items() if n != "sparse"]
    assert "ubz" not in others and len(set(others)) == len(others)
    tree = open(os.path.join(PKG, "_sparse.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy)", tree, flags=re.M) and "from ._binding import Binding" in tree
    src = open(os.path.join(B.CSRC, B.ADDONS["sparse"].sources[0])).read()
    assert '#include "../ubr_sat.h"' in src and '#include "../ubr_sparse_plan.h"' in src and "SAT_EXPORTS(ubz, UBZ_VERSION)" in src
    assert "Malloc" not in src and "hipFree" not in src and "Synchronize" not in src, "no allocation, free or sync"
    code = re.sub(r"//.*", "", src)
    assert len(re.findall(r"\batomic\w*\(", code)) == 1 and "atomicAdd(status" in code, "the one atomic is the status word's"
    assert code.count("lit_mask(") == 3, "the predicate: defined once, called by the count pass and by the write pass"
    # the plan compiles without HIP: it reaches the shared scan plan and nothing else, and neither file names HIP outside comments
    plan, shared = os.path.join(B.CSRC, "ubr_sparse_plan.h"), os.path.join(B.CSRC, "ubr_scan_plan.h")
    assert _include_closure([plan]) == {os.path.realpath(shared)} and _include_closure([shared]) == set()
    for f in (plan, shared):
        assert "hip" not in re.sub(r"//.*", "", open(f).read()).lower(), f
    assert re.findall(r"#\s*include\s*<([^>]+)>", open(plan).read() + open(shared).read()) == ["stdint.h"]


def test_a_missing_library_is_a_runtime_error(monkeypatch):
    nowhere = os.path.join(REPO, "no_such_dir", "libubresnet_sparse.so")
    monkeypatch.setenv("UBZ_LIB", nowhere)
    spec = importlib.util.spec_from_file_location("ubresnet_amd._sparse_missing", os.path.join(PKG, "_sparse.py"))
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert fresh.LIB_PATH == nowhere
    for call in (lambda: fresh.scatter_view(0x1000, 0x2000, 1, None, 0x3000, 1, 2, 2, 0x4000), lambda: fresh.compact_scratch_bytes(1, 2, 2)):
        with pytest.raises(RuntimeError, match="is missing; build it with") as e:
            call()
        assert nowhere in str(e.value) and "There is no CPU fallback" in str(e.value)


def test_the_compiled_kernels_are_the_case_table():
    """no allow-list: every compiled kernel is launched by a case of test_gpu_sparse_exact.py, and the table names nothing else"""
    H.need_lib(LIB)
    compiled = kernel_symbols.kernels(LIB)
    assert compiled == sorted(R.KERNEL_CASES), (compiled, sorted(R.KERNEL_CASES))
    assert all(R.KERNEL_CASES.values())
    ran = H.case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_sparse_exact.py"))
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
    lib = B.ADDONS["sparse"]
    assert isinstance(lib, B.Lib) and lib.sources == [os.path.join("extra", "ubr_sparse.hip")] and lib.binding == "_sparse"
    assert "sparse" not in B.LIBS and "sparse" not in B.EXTRAS and list(B.ADDONS)[0] == "blend"
    listed = [os.path.realpath(os.path.join(B.CSRC, h)) for h in lib.headers]
    assert len(listed) == len(set(listed)) and set(listed) == _include_closure([os.path.join(B.CSRC, s) for s in lib.sources])
    assert os.path.realpath(HEADER) in listed and os.path.realpath(os.path.join(B.CSRC, "ubr_sparse_plan.h")) in listed
    assert not set(B.SOURCES + B.HEADERS) & set(lib.sources + lib.headers), "source_hash() covers the network's library only"


def test_a_forced_build_of_sparse_is_one_compile_and_one_link(monkeypatch, capsys):
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    capsys.readouterr()
    built = B.build_addons(force=True, only=["sparse"])
    monkeypatch.undo()
    lib = B.ADDONS["sparse"]
    src, obj = os.path.join(B.CSRC, lib.sources[0]), os.path.join(B.CSRC, "extra", "ubr_sparse.o")
    assert built == [lib.out] and len(lines) == 2
    assert lines[0] == [B.HIPCC] + B.FLAGS + ["-c", src, "-o", obj]
    assert lines[1] == [B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib.out, obj]
    io = capsys.readouterr()
    assert io.out == "" and io.err.strip().split("\n") == [" ".join(c) for c in lines]


def test_entry_point_reports_sparse_on_stderr_before_the_score_line(monkeypatch, capsys):
    import __graft_entry__ as entry
    for lib in [l for t in (B.LIBS, B.ADDONS, B.EXTRAS) for l in t.values()]:
        H.need_lib(lib.out)
    for f in ("build", "build_addons", "build_extras"):
        monkeypatch.setattr(B, f, lambda *a, **kw: None)
    capsys.readouterr()
    entry.build()
    io = capsys.readouterr()
    err = io.err.strip().split("\n")
    assert "sparse" not in io.out and "built %s ABI version 1" % LIB in err
    assert err[-1] == "built %s ABI version 1" % B.EXTRAS["score"].out and err.index("built %s ABI version 1" % LIB) < len(err) - 1
    assert len(io.out.strip().split("\n")) + len(err) >= 15 + 2


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals: every call below is refused on the host, before any HIP call; the addresses are never dereferenced
# ------------------------------------------------------------------------------------------------------------------------
_P = 0x100000
_SCATTER = dict(index=_P, value=_P + 0x1000, n=4, count=_P + 0x2000, view=_P + 0x10000, P=2, rows=3, cols=5, status=_P + 0x3000)
_BAD_SCATTER = {
    "null index": (dict(index=None), "null pointer (an entry array"),
    "null value": (dict(value=None), "null pointer (an entry array"),
    "null view": (dict(view=None), "null pointer (view)"),
    "null status": (dict(status=None), "null pointer (status)"),
    "n negative": (dict(n=-1), "n=-1 must be in 0..2^31-1"),
    "n 2^31": (dict(n=1 << 31), "must be in 0..2^31-1"),
    "P 0": (dict(P=0), "must be positive"),
    "rows negative": (dict(rows=-3), "must be positive"),
    "cols 0": (dict(cols=0), "must be positive"),
    "2^31 pixels": (dict(P=2, rows=32768, cols=32768), "below 2^31 pixels"),
    "far too large": (dict(P=1 << 20, rows=1 << 20, cols=1 << 20), "below 2^31 pixels"),
    "index alignment": (dict(index=_P + 2), "4-byte aligned"),
    "count alignment": (dict(count=_P + 0x2004), "8-byte aligned"),
    "status alignment": (dict(status=_P + 0x3001), "8-byte aligned"),
    "value alignment": (dict(value=_P + 0x1001), "value and view must be 4-byte aligned"),
    "view alignment": (dict(view=_P + 0x10002), "value and view must be 4-byte aligned"),
    "view is index": (dict(view=_P), "view overlaps"),
    "status inside view": (dict(status=_P + 0x10000 + 8), "view overlaps"),
}
_COMPACT = dict(label=_P, conf=_P + 0x1000, adc=_P + 0x2000, vplanes=1, thr=10.0, P=2, rows=3, cols=5, capacity=30, oi=_P + 0x4000,
                ol=_P + 0x5000, oc=_P + 0x6000, count=_P + 0x7000, scratch=_P + 0x8000, sbytes=16)
_BAD_COMPACT = {
    "null label": (dict(label=None), "null pointer (label, confidence)"),
    "null confidence": (dict(conf=None), "null pointer (label, confidence)"),
    "null out_index": (dict(oi=None), "null pointer (out_index"),
    "null out_label": (dict(ol=None), "null pointer (out_index"),
    "null out_confidence": (dict(oc=None), "null pointer (out_index"),
    "null count": (dict(count=None), "null pointer (out_index"),
    "null scratch": (dict(scratch=None), "null pointer (scratch)"),
    "P 0": (dict(P=0), "must be positive"),
    "2^31 pixels": (dict(P=2, rows=32768, cols=32768), "below 2^31 pixels"),
    "vplanes 0": (dict(vplanes=0), "vplanes=0 must be 1..64"),
    "vplanes 65": (dict(vplanes=65), "vplanes=65 must be 1..64"),
    "capacity 0": (dict(capacity=0), "capacity=0 must be >= 1"),
    "capacity negative": (dict(capacity=-5), "capacity=-5 must be >= 1"),
    "short scratch": (dict(sbytes=15), "scratch_bytes=15 is short of the 16"),
    "scratch alignment": (dict(scratch=_P + 0x8008), "scratch must be 16-byte aligned"),
    "confidence alignment": (dict(conf=_P + 0x1001), "2-byte"),
    "adc alignment": (dict(adc=_P + 0x2002), "4-byte"),
    "out_index alignment": (dict(oi=_P + 0x4002), "4-byte"),
    "count alignment": (dict(count=_P + 0x7004), "8-byte aligned"),
    "out_label inside label": (dict(ol=_P + 29), "overlaps an input"),
    "scratch is adc": (dict(scratch=_P + 0x2000), "overlaps an input"),
    "count inside out_index": (dict(count=_P + 0x4000 + 112), "two outputs overlap"),
}
_EXPAND = dict(index=_P, label=_P + 0x1000, conf=_P + 0x2000, n=4, count=None, fill=255, ol=_P + 0x10000, oc=_P + 0x20000, P=2, rows=3,
               cols=5, status=_P + 0x3000)
_BAD_EXPAND = {
    "null index": (dict(index=None), "null pointer (an entry array"),
    "null label": (dict(label=None), "null pointer (an entry array"),
    "null confidence": (dict(conf=None), "null pointer (an entry array"),
    "null status": (dict(status=None), "null pointer (status)"),
    "null out_label": (dict(ol=None), "null pointer (out_label, out_confidence)"),
    "null out_confidence": (dict(oc=None), "null pointer (out_label, out_confidence)"),
    "n negative": (dict(n=-2), "n=-2 must be in 0..2^31-1"),
    "2^31 pixels": (dict(P=2, rows=32768, cols=32768), "below 2^31 pixels"),
    "fill 256": (dict(fill=256), "fill_label=256 must be 0..255"),
    "fill negative": (dict(fill=-1), "fill_label=-1 must be 0..255"),
    "confidence alignment": (dict(conf=_P + 0x2001), "2-byte aligned"),
    "out_confidence alignment": (dict(oc=_P + 0x20001), "2-byte aligned"),
    "out_label is label": (dict(ol=_P + 0x1000), "overlaps an input"),
    "outputs overlap": (dict(oc=_P + 0x10000 + 28), "out_label overlaps out_confidence"),
}


def _refused(rc, prefix, message, name):
    msg = Z.lib().ubz_last_error().decode()
    assert rc == -1 and msg.startswith(prefix + ":") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=prefix):
        Z.check(rc, name)


@pytest.mark.parametrize("name", sorted(_BAD_SCATTER))
def test_scatter_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD_SCATTER[name]
    a = dict(_SCATTER, **change)
    rc = Z.lib().ubz_scatter_view(a["index"], a["value"], a["n"], a["count"], a["view"], a["P"], a["rows"], a["cols"], a["status"], None)
    _refused(rc, "ubz_scatter_view", message, name)


@pytest.mark.parametrize("name", sorted(_BAD_COMPACT))
def test_compact_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD_COMPACT[name]
    a = dict(_COMPACT, **change)
    rc = Z.lib().ubz_compact(a["label"], a["conf"], a["adc"], a["vplanes"], a["thr"], a["P"], a["rows"], a["cols"], a["capacity"], a["oi"],
                             a["ol"], a["oc"], a["count"], a["scratch"], a["sbytes"], None)
    _refused(rc, "ubz_compact", message, name)


@pytest.mark.parametrize("name", sorted(_BAD_EXPAND))
def test_expand_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD_EXPAND[name]
    a = dict(_EXPAND, **change)
    rc = Z.lib().ubz_expand(a["index"], a["label"], a["conf"], a["n"], a["count"], a["fill"], a["ol"], a["oc"], a["P"], a["rows"], a["cols"],
                            a["status"], None)
    _refused(rc, "ubz_expand", message, name)


def test_scratch_bytes_follow_the_plan():
    H.need_lib(LIB)
    for image in sorted({c["image"] for c in R.CASES.values()}) + [(3, 1008, 3456)]:
        blocks = -(-R.pixels_of(image) // R.PIXEL_BLOCK)
        assert Z.compact_scratch_bytes(*image) == 4 * (-(-blocks // 4) * 4), image
    assert Z.lib().ubz_compact_scratch_bytes(2, 32768, 32768) == 0 and b"below 2^31 pixels" in Z.lib().ubz_last_error()
    with pytest.raises(RuntimeError, match="ubz_compact_scratch_bytes"):
        Z.compact_scratch_bytes(0, 4, 4)


# ------------------------------------------------------------------------------------------------------------------------
# the plan as a program
# ------------------------------------------------------------------------------------------------------------------------
def test_plan_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/sparse_host.cpp has its own main and includes ubr_sparse_plan.h; built with -fsanitize=address,undefined and run as a
    process of its own over every image of the case table (and every size from 1 pixel to three blocks and one): the plan's
    numbers, and count / scan / write restated on the host against brute force, with buffers of exactly the planned sizes"""
    exe = str(tmp_path / "sparse_host")
    r = subprocess.run([H.cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "sparse_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    images = sorted({c["image"] for c in R.CASES.values()})
    p = subprocess.run([exe] + [str(v) for im in images for v in im], capture_output=True, text=True)
    assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
    rows = [[int(v) for v in l.split()[1:]] for l in p.stdout.strip().split("\n") if l.startswith("I ")]
    assert [tuple(r[:3]) for r in rows] == images
    for P, rows_, cols, pixels, blocks, trips, sbytes in rows:
        assert pixels == P * rows_ * cols and blocks == -(-pixels // R.PIXEL_BLOCK) and trips == -(-blocks // R.SCAN_WIDTH)
        assert sbytes == 4 * (-(-blocks // 4) * 4)
    by_image = {tuple(r[:3]): r for r in rows}
    assert by_image[R.IMG_S][4:6] == [R.S, 1] and by_image[R.IMG_SP1][4:6] == [R.S + 1, 2] and by_image[R.IMG_BP1][4] == 2 and by_image[R.IMG_B][4] == 1
    assert p.stdout.strip().split("\n")[-1].split() == ["G"] + [str(v) for v in (Z.LANES, Z.LANE_PIXELS, Z.PIXEL_BLOCK, Z.SCAN_WIDTH, Z.MAX_GRID)]


def test_shared_scan_plan_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/scan_host.cpp has its own main and includes ubr_scan_plan.h alone; built with -fsanitize=address,undefined and run as a
    process of its own: the shared host_count / host_scan / host_rank against brute force at 1, B - 1, B, B + 1 pixels and at S and
    S + 1 blocks, with a scratch buffer of exactly the planned words, and stride_grid at 0, 1, lanes + 1 and past the cap"""
    exe = str(tmp_path / "scan_host")
    r = subprocess.run([H.cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "scan_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
    lines = p.stdout.strip().split("\n")
    rows = [[int(v) for v in l.split()[1:]] for l in lines if l.startswith("I ")]
    B_, S_ = R.PIXEL_BLOCK, R.SCAN_WIDTH
    assert [r[0] for r in rows] == [1, B_ - 1, B_, B_ + 1, S_ * B_, S_ * B_ + 1]
    assert [r[1:3] for r in rows] == [[1, 1], [1, 1], [1, 1], [2, 1], [S_, 1], [S_ + 1, 2]]
    assert all(sbytes == 4 * (-(-blocks // 4) * 4) for _, blocks, _, sbytes in rows)
    assert lines[-1].split() == ["G"] + [str(v) for v in (Z.LANES, Z.LANE_PIXELS, Z.PIXEL_BLOCK, Z.SCAN_WIDTH)]


# ------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------------
class _Conv:
    in_channels, out_channels = 1, 3


class _Model:
    conv1 = conv11 = _Conv()

    def eval(self):
        raise AssertionError("the arguments are checked before the model is touched")


def test_sparse_event_refusals_and_from_dense():
    idx, val = torch.tensor([0, 3], dtype=torch.int32), torch.tensor([1.0, 2.0])
    ev = sparse.SparseEvent(idx, val, 1, 2, 2)
    assert ev.n == 2 and ev.validate() is ev and (ev.planes, ev.rows, ev.cols) == (1, 2, 2)
    for bad in (dict(index=idx.long()), dict(value=val.double()), dict(index=[0, 3])):
        with pytest.raises(TypeError, match="SparseEvent"):
            sparse.SparseEvent(**dict(dict(index=idx, value=val, planes=1, rows=2, cols=2), **bad))
    for bad in (dict(index=idx[:1]), dict(value=val.reshape(2, 1)), dict(index=idx.reshape(1, 2), value=val.reshape(1, 2))):
        with pytest.raises(ValueError, match="1-D of one length"):
            sparse.SparseEvent(**dict(dict(index=idx, value=val, planes=1, rows=2, cols=2), **bad))
    for bad in (dict(planes=0), dict(rows=-1), dict(cols=2.0), dict(planes=True)):
        with pytest.raises(ValueError, match="positive int"):
            sparse.SparseEvent(**dict(dict(index=idx, value=val, planes=1, rows=2, cols=2), **bad))
    with pytest.raises(ValueError, match="int32 pixel index"):
        sparse.SparseEvent(idx, val, 2, 32768, 32768)
    for bad in ([0, 4], [-1, 2], [2, 2], [3, 1]):
        with pytest.raises(ValueError, match="outside|strictly ascending"):
            sparse.SparseEvent(torch.tensor(bad, dtype=torch.int32), val, 1, 2, 2).validate()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.to_view("cpu")
    # from_dense: every element whose bits are not +0.0, in index order, bit for bit; or the elements above a threshold
    bits = np.array([0, 0x80000000, 0x7FC12345, 1, 0, 0x41300000, 0x41200000, 0], np.uint32)
    view = torch.from_numpy(bits.view(np.float32).reshape(2, 1, 2, 2).copy())
    ev = sparse.SparseEvent.from_dense(view).validate()
    assert (ev.planes, ev.rows, ev.cols) == (2, 2, 2) and ev.index.dtype == torch.int32 and ev.index.tolist() == [1, 2, 3, 5, 6]
    assert ev.value.numpy().view(np.uint32).tolist() == [0x80000000, 0x7FC12345, 1, 0x41300000, 0x41200000]
    above = sparse.SparseEvent.from_dense(view[:, 0], threshold=10.0)
    assert above.index.tolist() == [5] and above.value.tolist() == [11.0]
    with pytest.raises(TypeError, match="float32"):
        sparse.SparseEvent.from_dense(view.double())
    with pytest.raises(ValueError, match="planes"):
        sparse.SparseEvent.from_dense(view.reshape(8))


def test_compact_and_pixel_list_refusals_without_a_device():
    lab, conf = torch.zeros((2, 3, 5), dtype=torch.uint8), torch.zeros((2, 3, 5), dtype=torch.float16)
    view = torch.zeros((2, 1, 3, 5))
    good = deploy.Products(lab, conf, None)
    with pytest.raises(TypeError, match="uint8"):
        sparse.compact(deploy.Products(lab.int(), conf, None), view)
    with pytest.raises(TypeError, match="float16"):
        sparse.compact(deploy.Products(lab, conf.float(), None), view)
    with pytest.raises(ValueError, match="rows,cols"):
        sparse.compact(deploy.Products(lab.reshape(-1), conf.reshape(-1), None), view)
    with pytest.raises(ValueError, match="rows,cols"):
        sparse.compact(deploy.Products(lab, conf[:1], None), view)
    with pytest.raises(TypeError, match="view must be a float32"):
        sparse.compact(good, view.double())
    with pytest.raises(ValueError, match="planes of"):
        sparse.compact(good, view, vplanes=3)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="capacity"):
            sparse.compact(good, view, capacity=bad)
    for bad in (0, 65, "1"):
        with pytest.raises(ValueError, match="vplanes"):
            sparse.compact(good, view, vplanes=bad)
    with pytest.raises(ValueError, match="fill_label"):
        sparse.compact(good, view, fill_label=256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sparse.compact(good, view)                              # every argument is fine: the tensors are on the host
    # read() of a list that overflowed raises before any entry is copied; the count still holds the total
    pl = sparse.PixelList(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.uint8), torch.zeros(2, dtype=torch.float16),
                          torch.tensor([5]), None, 1, 3, 5, 255)
    assert pl.capacity == 2 and int(pl.count) == 5
    with pytest.raises(OverflowError, match="5 lit pixels, capacity 2"):
        pl.read()
    ok = pl._replace(count=torch.tensor([1]), index=torch.tensor([4, 9], dtype=torch.int32))
    i, l, c = ok.read()
    assert i.tolist() == [4] and l.shape == c.shape == (1,)
    assert sparse.PixelList._fields == ("index", "label", "confidence", "count", "counts", "planes", "rows", "cols", "fill_label")


def test_segmenter_output_names_and_capacity_without_a_device():
    kw = dict(planes=3, tile=(64, 96), batch=4)
    with pytest.raises(ValueError, match="output must be"):
        deploy.WholeViewSegmenter(_Model(), 96, 160, output="labels", **kw)
    for bad in ("pixel", "Pixels", "", None, 1):
        with pytest.raises(ValueError, match="output must be"):
            deploy.WholeViewSegmenter(_Model(), 96, 160, output=bad, **kw)
    with pytest.raises(ValueError, match="output must be 'scores' or 'products'"):
        deploy.segment_crops(_Model(), torch.zeros(1, 1, 8, 8), output="pixels")         # segment_crops has no pixel list
    sig = inspect.signature(deploy.WholeViewSegmenter.__init__).parameters
    assert sig["capacity"].default is None and list(sig)[-1] == "capacity" and sig["output"].default == "scores"
    for bad in (0, -4, 2.5, True, "9"):
        with pytest.raises(ValueError, match="capacity must be None or an int"):
            deploy.WholeViewSegmenter(_Model(), 96, 160, output="pixels", capacity=bad, **kw)
    with pytest.raises(ValueError, match="needs output='pixels'"):
        deploy.WholeViewSegmenter(_Model(), 96, 160, output="products", capacity=100, **kw)
    seg = deploy.WholeViewSegmenter(_Model(), 96, 160, output="pixels", capacity=100, **kw)
    assert seg.capacity == 100 and seg.status is None and seg._view_buf is None and seg._compactor is None and seg._pix_dense is None
    base = deploy.WholeViewSegmenter(_Model(), 96, 160, output="products", **kw)
    assert base.tiles == seg.tiles and base.capacity is None and base._compactor is None
    with pytest.raises(RuntimeError, match="expected a SparseEvent of 3 x 96 x 160"):
        seg(sparse.SparseEvent(torch.zeros(0, dtype=torch.int32), torch.zeros(0), 3, 96, 161))
    assert "pixels" in deploy.WholeViewSegmenter.__doc__ and "SparseEvent" in deploy.WholeViewSegmenter.__doc__
