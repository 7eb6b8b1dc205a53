"""PlaneMatch without a GPU: libubresnet_match.so's header is C99, and header, binding, reference, plan and library agree on entry
points and constants; the library stands alone and exports its binding's symbols; the ADDONS entry, its include closure and a
forced build; every argument refusal returns UBU_EINVAL with a message before any HIP call; the plan, the tile enumeration, the
trip counts and the bounds as a stand-alone program under the host sanitizers (tests/match_host.cpp); the numpy reference on a
hand-made event; PlaneTable on hand-made tables; make_matched_event; and the numpy reference recovering the instance pairing of
matched events."""
import importlib
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import match_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ubresnet_amd")
HEADER = os.path.join(REPO, "include", "ubresnet_match.h")
import cpu_helpers as H  # noqa: E402
from ubresnet_amd import _match as M  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd import planes, synthetic  # noqa: E402

LIB = B.ADDONS["match"].out
PLAN = os.path.join(B.CSRC, "ubr_match_plan.h")
NAMES = ("LANES|TRIP_PIXELS|MAX_GRID|TILE|CHUNK_BINS|MIN_PLANES|MAX_PLANES|MIN_SLOTS|MAX_SLOTS|MAX_TIME_BIN|MAX_SHIFT|MAX_ROWS|MAX_COLS|"
         "MAX_PLANE_PIXELS|MAX_BIN_PIXELS|MAX_CLASSES|CLUSTER_FIXED|CAND_COLUMNS|PAIR_COLUMNS|MAX_WEIGHT|MAX_SCALE")


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def _hand_made():
    """2 x 4 x 6: plane 0 holds cluster 0 (rows 0..1, five pixels) and cluster 1 (row 3, one pixel); plane 1 holds cluster 2
    (rows 1..2, four pixels)"""
    ids = np.full((2, 4, 6), -1, np.int32)
    ids[0, 0, 0:3], ids[0, 1, 1:3], ids[0, 3, 5], ids[1, 1, 2:4], ids[1, 2, 3:5] = 0, 0, 1, 2, 2
    table = np.zeros((3, 12), np.int64)
    table[:, 0], table[:, 1] = [0, 23, 24 + 8], [5, 1, 4]
    view = np.zeros((2, 4, 6), np.float32)
    view[0, 0, 0:3], view[0, 1, 1:3], view[0, 3, 5] = [1.0, 2.0, 0.0], [4.0, np.nan], 9.0
    view[1, 1, 2:4], view[1, 2, 3:5] = [3.0, 0.5], [1e9, -1.0]
    return ids, table, view


def test_reference_on_a_hand_made_event():
    ids, table, view = _hand_made()
    r = R.match(ids, table, 3, 8, view, 2, 2, 1, (0, 0), 64)
    assert r["ncand"] == 2 and r["status"] == [0, 0] and r["profile"].shape == (64, 4) and r["profile"].dtype == np.uint32
    assert r["profile"][:3].tolist() == [[6, 8, 0, 0], [0, 7, 65535, 0], [0, 0, 0, 0]]
    assert r["candidates"][:3].tolist() == [[0, 0, 14, 2, 0, 1], [2, 1, 65542, 2, 1, 2], [0] * 6]
    assert r["pairs"][0, 1].tolist() == [1, 7, 8, 7] and (r["pairs"][1, 0] == R.SENTINEL).all() and (r["pairs"][0, 2] == R.SENTINEL).all()
    # min_pixels 1: the one-pixel cluster is candidate 1, of the same plane as candidate 0 (four zeros), and shares no bin with 2
    r = R.match(ids, table, 3, 8, view, 2, 1, 1, (0, 0), 64)
    assert r["ncand"] == 3 and r["candidates"][:3, :2].tolist() == [[0, 0], [1, 0], [2, 1]]
    assert r["pairs"][0, 1].tolist() == [0] * 4 and r["pairs"][1, 2].tolist() == [0] * 4 and r["pairs"][0, 2].tolist() == [1, 7, 8, 7]
    # time_bin 2 folds rows 0..1 and 2..3; a shift of plane 1 by -2 drops its row 1 and moves row 2 to row 0
    r = R.match(ids, table, 3, 8, view, 2, 2, 2, (0, -2), 64)
    assert r["status"] == [0, 2] and r["profile"][:2].tolist() == [[14, 0], [65535, 0]] and r["candidates"][1].tolist() == [2, 1, 65535, 1, 0, 0]
    assert r["pairs"][0, 1].tolist() == [1, 14, 14, 65535]
    # the weight-0 pixel of a NaN still occupies its bin: cluster 0 has a pixel in row 1 whatever its charge
    gone = view.copy()
    gone[0, 1] = np.nan
    assert R.match(ids, table, 3, 8, gone, 2, 2, 1, (0, 0), 64)["pairs"][0, 1].tolist() == [1, 0, 0, 7]
    # the count and the capacity bound the clusters that are read
    assert R.match(ids, table, 2, 8, view, 2, 2, 1, (0, 0), 64)["ncand"] == 1 and R.match(ids, table, 3, 1, view, 2, 1, 1, (0, 0), 64)["ncand"] == 1


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_match.h"\n'
                     'int main(void) {\n'
                     '  int (*m)(const int32_t*, const long long*, int, const unsigned long long*, int64_t, const float*, float, int, int, int,\n'
                     '           int64_t, int, const int*, int64_t, uint32_t*, long long*, long long*, unsigned long long*, unsigned long long*,\n'
                     '           void*, void*) = ubu_match;\n'
                     '  int64_t (*s)(int, int, int, int, int64_t, int64_t) = ubu_scratch_bytes;\n'
                     '  const char* (*e)(void) = ubu_last_error;\n'
                     '  int (*v)(void) = ubu_version;\n'
                     '  return m == 0 || s == 0 || e == 0 || v == 0 || UBU_OK != 0 || UBU_EINVAL != -1 || UBU_ELAUNCH != -2\n'
                     '         || UBU_CAND_COLUMNS != 6 || UBU_PAIR_COLUMNS != 4 || UBU_MAX_SLOTS % UBU_TILE;\n}\n')
    r = subprocess.run([H.cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_plan_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(ubu_[a-z_0-9]+)\s*\(", text)
    assert declared == M.SYMBOLS == ["ubu_scratch_bytes", "ubu_match", "ubu_last_error", "ubu_version"]
    constants = {k: int(v) for k, v in re.findall(r"#define\s+UBU_(%s)\s+(\d+)" % NAMES, text)}
    assert constants == {k: getattr(M, k) for k in NAMES.split("|")}
    assert (R.TILE, R.CHUNK_BINS, R.CAND_COLUMNS, R.PAIR_COLUMNS, R.CLUSTER_FIXED, R.MIN_SLOTS, R.MAX_SLOTS, R.MAX_TIME_BIN, R.MAX_SHIFT, R.MAX_WEIGHT,
            R.CAND_NAMES, R.PAIR_NAMES) == (M.TILE, M.CHUNK_BINS, M.CAND_COLUMNS, M.PAIR_COLUMNS, M.CLUSTER_FIXED, M.MIN_SLOTS, M.MAX_SLOTS,
                                            M.MAX_TIME_BIN, M.MAX_SHIFT, M.MAX_WEIGHT, M.CAND_NAMES, M.PAIR_NAMES)
    assert "{%s}" % ", ".join(M.CAND_NAMES) in raw and "{%s}" % ", ".join(M.PAIR_NAMES) in raw
    assert len(M.CAND_NAMES) == M.CAND_COLUMNS and len(M.PAIR_NAMES) == M.PAIR_COLUMNS
    from ubresnet_amd import _cluster, _moment
    assert M.CLUSTER_FIXED == _cluster.TABLE_FIXED and M.MAX_CLASSES == _cluster.MAX_CLASSES
    assert (M.MAX_ROWS, M.MAX_COLS, M.MAX_PLANE_PIXELS, M.MAX_WEIGHT, M.MAX_SCALE) == \
        (_moment.MAX_ROWS, _moment.MAX_COLS, _moment.MAX_PLANE_PIXELS, _moment.MAX_WEIGHT, _moment.MAX_SCALE), "the limits of ubresnet_moment.h"
    plan = open(PLAN).read()
    # the bound of a bin is stated in the plan header and holds
    assert "time_bin * cols * 65535" in plan and "below 2^32" in plan and "MAX_BIN_PIXELS = 65536" in plan
    assert M.MAX_BIN_PIXELS * M.MAX_WEIGHT < 2 ** 32 <= (M.MAX_BIN_PIXELS + 1) * M.MAX_WEIGHT + M.MAX_WEIGHT
    for phrase in ("STORED", "ADDED to", "are not touched", "ties to even", "no spinning", "Five launches", "on the HOST", "there are no atomics",
                   "returns after one read of ncand", "same bytes on every run", "A pair from one plane is four zeros"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", raw), phrase
    H.need_lib(LIB)
    assert M.lib().ubu_version() == M.BINDING.version() == 1
    assert M.scratch_bytes(3, 1008, 3456, 1, 512, 65536) == 8 * 512 * 16 + 4 * 512 * 1008 + 4 * 65536
    assert M.scratch_bytes(2, 5, 12, 4, 64, 4096) == 8 * 64 + 4 * 64 * 2 + 4 * 120 and M.time_bins(37, 4) == 10 == R.time_bins(37, 4)
    assert M.lib().ubu_scratch_bytes(1, 8, 8, 1, 64, 8) == 0 and "P must be 2..4" in M.lib().ubu_last_error().decode()
    with pytest.raises(RuntimeError, match="ubu_scratch_bytes refused.*multiple of 64"):
        M.scratch_bytes(2, 4, 4, 1, 100, 8)


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


def test_library_stands_alone_and_exports_exactly_its_bindings_symbols():
    bd = M.BINDING
    assert bd.prefix == "ubu" and bd.path == LIB and os.path.basename(LIB) == "libubresnet_match.so" and os.path.dirname(LIB) == PKG
    assert (M.LIB_PATH, M.SYMBOLS, M.lib, M.check) == (bd.path, bd.symbols, bd.lib, bd.check)
    H.need_lib(LIB)
    assert "libubresnet_" not in H.readelf("-d", LIB).replace("libubresnet_match", "")
    assert sorted(n for n in H.defined_symbols(LIB) if re.match(r"ub[a-z]_", n)) == sorted(bd.symbols)
    others = [importlib.import_module("ubresnet_amd." + lib.binding).BINDING.prefix for t in (B.LIBS, B.EXTRAS, B.ADDONS)
              for n, lib in t.items() if n != "match"]
    assert "ubu" not in others and len(set(others)) == len(others), "the ubu prefix is the library's alone"
    tree = open(os.path.join(PKG, "_match.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy)", tree, flags=re.M) and "from ._binding import Binding" in tree
    assert 'Binding("UBU_LIB", "libubresnet_match.so", "ubu"' in tree
    src = open(os.path.join(B.CSRC, B.ADDONS["match"].sources[0])).read()
    assert '#include "../ubr_sat.h"' in src and '#include "../ubr_match_plan.h"' in src and "SAT_EXPORTS(ubu, UBU_VERSION)" in src
    assert '#include "../ubr_walk.h"' in src and '#include "../ubr_adc_rule.h"' in src and "weight_of(float" not in src
    assert "walk::trip_loop" in src and "walk::wave_round" in src and "walk::load_ids" in src and "wv::block_scan" in src
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "Malloc" not in src and "hipFree" not in src and "Synchronize" not in src, "no allocation, free or sync"
    assert "cooperative" not in code.lower() and "while (true)" not in code and "__threadfence" not in code
    assert len(re.findall(r"<<<", code)) == 5, "five launches"
    match_kernel = code[code.index("void match_kernel"):code.index("int check_geometry")]
    assert "atomic" not in match_kernel, "the match launch writes each pair once, without atomics"
    after_profile = code[code.index("void summary_kernel"):code.index("int check_geometry")]
    assert not re.search(r"\b(float|double)\b", after_profile), "integers only past the weight of a pixel"
    # the plan compiles without HIP: it reaches the shared scan plan and walk plan and nothing else
    shared, walk = os.path.join(B.CSRC, "ubr_scan_plan.h"), os.path.join(B.CSRC, "ubr_walk_plan.h")
    assert _include_closure([PLAN]) == {os.path.realpath(shared), os.path.realpath(walk)}
    assert re.findall(r"#\s*include\s*<([^>]+)>", open(PLAN).read()) == []
    host = os.path.join(REPO, "tests", "match_host.cpp")
    assert re.findall(r'#\s*include\s*"([^"]+)"', open(host).read()) == ["ubr_match_plan.h"]


def test_a_missing_library_is_a_runtime_error(monkeypatch):
    import importlib.util
    nowhere = os.path.join(REPO, "no_such_dir", "libubresnet_match.so")
    monkeypatch.setenv("UBU_LIB", nowhere)
    spec = importlib.util.spec_from_file_location("ubresnet_amd._match_missing", os.path.join(PKG, "_match.py"))
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert fresh.LIB_PATH == nowhere
    with pytest.raises(RuntimeError, match="is missing; build it with") as e:
        fresh.match(0x1000, 0x2000, 12, 0x3000, 8, 0x4000, 16.0, 2, 2, 2, 1, 1, (0, 0), 64, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000, 0xA000)
    assert nowhere in str(e.value) and "There is no CPU fallback" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------
# the build table
# ------------------------------------------------------------------------------------------------------------------------
def test_the_addons_entry_is_last_and_lists_the_true_include_closure():
    lib = B.ADDONS["match"]
    assert isinstance(lib, B.Lib) and lib.sources == [os.path.join("extra", "ubr_match.hip")] and lib.binding == "_match"
    assert "match" not in B.LIBS and "match" not in B.EXTRAS
    assert list(B.ADDONS)[:8] == ["blend", "sparse", "crop", "calib", "cluster", "moment", "overlap", "match"]
    listed = [os.path.realpath(os.path.join(B.CSRC, h)) for h in lib.headers]
    assert len(listed) == len(set(listed)) and set(listed) == _include_closure([os.path.join(B.CSRC, s) for s in lib.sources])
    assert os.path.realpath(HEADER) in listed and os.path.realpath(PLAN) in listed
    for shared in ("ubr_walk.h", "ubr_walk_plan.h", "ubr_adc_rule.h", "ubr_wave.h", "ubr_scan_plan.h"):
        assert os.path.realpath(os.path.join(B.CSRC, shared)) in listed
    for foreign in ("ubr_moment_plan.h", "ubr_overlap_plan.h", "ubr_cluster_plan.h"):
        assert os.path.realpath(os.path.join(B.CSRC, foreign)) not in listed
    assert not set(B.SOURCES + B.HEADERS) & set(lib.sources + lib.headers), "source_hash() covers the network's library only"


def test_a_forced_build_of_match_is_one_compile_and_one_link(monkeypatch, capsys):
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    capsys.readouterr()
    built = B.build_addons(force=True, only=["match"])
    monkeypatch.undo()
    lib = B.ADDONS["match"]
    src, obj = os.path.join(B.CSRC, lib.sources[0]), os.path.join(B.CSRC, "extra", "ubr_match.o")
    assert built == [lib.out] and len(lines) == 2
    assert lines[0] == [B.HIPCC] + B.FLAGS + ["-c", src, "-o", obj]
    assert lines[1] == [B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib.out, obj]
    io = capsys.readouterr()
    assert io.out == "" and io.err.strip().split("\n") == [" ".join(c) for c in lines]


def test_entry_point_reports_match_on_stderr_after_overlap(monkeypatch, capsys):
    import __graft_entry__ as entry
    for lib in [l for t in (B.LIBS, B.ADDONS, B.EXTRAS) for l in t.values()]:
        H.need_lib(lib.out)
    for f in ("build", "build_addons", "build_extras"):
        monkeypatch.setattr(B, f, lambda *a, **kw: None)
    capsys.readouterr()
    entry.build()
    io = capsys.readouterr()
    err = io.err.strip().split("\n")
    assert "match" not in io.out and "built %s ABI version 1" % LIB in err
    assert err.index("built %s ABI version 1" % B.ADDONS["overlap"].out) < err.index("built %s ABI version 1" % LIB)


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals: every call below is refused on the host, before any HIP call; the addresses are never dereferenced
# ------------------------------------------------------------------------------------------------------------------------
_P = 0x100000
_GOOD = dict(ids=_P, clusters=_P + 0x1000, width=12, count=_P + 0x3000, capacity=16, view=_P + 0x4000, scale=16.0, P=2, rows=3, cols=5,
             min_pixels=2, time_bin=1, shift=(0, 0), slots=64, profile=_P + 0x10000, cand=_P + 0x20000, pairs=_P + 0x40000,
             ncand=_P + 0x30000, status=_P + 0x30100, scratch=_P + 0x80000)
_BAD = {
    "null ids": (dict(ids=None), "null pointer (ids, clusters, count, view)"),
    "null clusters": (dict(clusters=None), "null pointer (ids, clusters, count, view)"),
    "null count": (dict(count=None), "null pointer (ids, clusters, count, view)"),
    "null view": (dict(view=None), "null pointer (ids, clusters, count, view)"),
    "null profile": (dict(profile=None), "null pointer (profile, candidates, pairs, ncand, status, scratch)"),
    "null candidates": (dict(cand=None), "null pointer (profile, candidates, pairs, ncand, status, scratch)"),
    "null pairs": (dict(pairs=None), "null pointer (profile, candidates, pairs, ncand, status, scratch)"),
    "null ncand": (dict(ncand=None), "null pointer (profile, candidates, pairs, ncand, status, scratch)"),
    "null status": (dict(status=None), "null pointer (profile, candidates, pairs, ncand, status, scratch)"),
    "null scratch": (dict(scratch=None), "null pointer (profile, candidates, pairs, ncand, status, scratch)"),
    "null row_shift": (dict(shift=None), "null pointer (row_shift)"),
    "ids alignment": (dict(ids=_P + 8), "ids and view must be 16-byte aligned"),
    "view alignment": (dict(view=_P + 0x4004), "ids and view must be 16-byte aligned"),
    "clusters alignment": (dict(clusters=_P + 0x1004), "8-byte aligned"),
    "count alignment": (dict(count=_P + 0x3004), "8-byte aligned"),
    "candidates alignment": (dict(cand=_P + 0x20004), "8-byte aligned"),
    "ncand alignment": (dict(ncand=_P + 0x30004), "8-byte aligned"),
    "status alignment": (dict(status=_P + 0x30104), "8-byte aligned"),
    "profile alignment": (dict(profile=_P + 0x10002), "profile must be 4-byte"),
    "pairs alignment": (dict(pairs=_P + 0x40008), "pairs and scratch 16-byte aligned"),
    "scratch alignment": (dict(scratch=_P + 0x80008), "pairs and scratch 16-byte aligned"),
    "width 8": (dict(width=8), "cluster_width=8 must be 8 + C for 1..16 classes"),
    "width 25": (dict(width=25), "cluster_width=25 must be 8 + C"),
    "scale 0": (dict(scale=0.0), "adc_scale=0 must be a power of two in 1..256"),
    "scale 3": (dict(scale=3.0), "adc_scale=3 must be a power of two in 1..256"),
    "scale 512": (dict(scale=512.0), "adc_scale=512 must be a power of two in 1..256"),
    "scale nan": (dict(scale=float("nan")), "must be a power of two in 1..256"),
    "min_pixels 0": (dict(min_pixels=0), "min_pixels=0 must be >= 1"),
    "min_pixels negative": (dict(min_pixels=-4), "min_pixels=-4 must be >= 1"),
    "P 1": (dict(P=1, shift=(0,)), "P must be 2..4"),
    "P 5": (dict(P=5, shift=(0,) * 5), "P must be 2..4"),
    "rows 0": (dict(rows=0), "rows and cols positive"),
    "cols negative": (dict(cols=-2), "rows and cols positive"),
    "rows 4097": (dict(rows=4097), "rows must be at most 4096"),
    "plane of 2^23": (dict(rows=2048, cols=4096), "rows * cols must be at most 2^22"),
    "time_bin 0": (dict(time_bin=0), "time_bin must be a power of two in 1..64"),
    "time_bin 3": (dict(time_bin=3), "time_bin must be a power of two in 1..64"),
    "time_bin 128": (dict(time_bin=128), "time_bin must be a power of two in 1..64"),
    "a bin past 32 bits": (dict(rows=64, cols=4096, time_bin=32), "time_bin * cols must be at most 65536"),
    "slots 0": (dict(slots=0), "slots must be a multiple of 64 in 64..4096"),
    "slots 96": (dict(slots=96), "slots must be a multiple of 64 in 64..4096"),
    "slots 8192": (dict(slots=8192), "slots must be a multiple of 64 in 64..4096"),
    "slots negative": (dict(slots=-64), "slots must be a multiple of 64"),
    "capacity 0": (dict(capacity=0), "capacity must be >= 1"),
    "shift too far": (dict(shift=(0, 4097)), "row_shift[1]=4097 must be in -4096..4096"),
    "shift too far back": (dict(shift=(-5000, 0)), "row_shift[0]=-5000 must be in -4096..4096"),
    "profile is view": (dict(profile=_P + 0x4000), "overlaps an input"),
    "ncand inside ids": (dict(ncand=_P + 0x10), "overlaps an input"),
    "scratch over clusters": (dict(scratch=_P + 0x1000), "overlaps an input"),
    "status is ncand": (dict(status=_P + 0x30000), "overlap one another"),
    "candidates inside pairs": (dict(cand=_P + 0x40100), "overlap one another"),
    "scratch inside profile": (dict(scratch=_P + 0x10010), "overlap one another"),
}


def _call(a):
    return M.lib().ubu_match(a["ids"], a["clusters"], a["width"], a["count"], a["capacity"], a["view"], a["scale"], a["P"], a["rows"], a["cols"],
                             a["min_pixels"], a["time_bin"], M.shifts(a["shift"]), a["slots"], a["profile"], a["cand"], a["pairs"], a["ncand"],
                             a["status"], a["scratch"], None)


@pytest.mark.parametrize("name", sorted(_BAD))
def test_match_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD[name]
    rc = _call(dict(_GOOD, **change))
    msg = M.lib().ubu_last_error().decode()
    assert rc == -1 and msg.startswith("ubu_match:") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match="ubu_match"):
        M.check(rc, name)


def test_the_good_arguments_differ_from_every_refusal_in_one_place_only():
    """the buffers of _GOOD do not overlap, so each entry of _BAD is refused for its own reason: the plan's sizes place them"""
    a = _GOOD
    T, S = a["rows"], a["slots"]
    ranges = [(a["ids"], 4 * 30), (a["clusters"], 8 * 16 * 12), (a["count"], 8), (a["view"], 4 * 30), (a["profile"], 4 * S * T),
              (a["cand"], 8 * S * 6), (a["pairs"], 8 * S * S * 4), (a["ncand"], 8), (a["status"], 16), (a["scratch"], 8 * S + 4 * S * T + 4 * 16)]
    ranges.sort()
    assert all(lo + n <= nxt for (lo, n), (nxt, _) in zip(ranges, ranges[1:]))


# ------------------------------------------------------------------------------------------------------------------------
# the plan as a program
# ------------------------------------------------------------------------------------------------------------------------
GEOMETRIES = [(3, 1008, 3456, 1, 512, 65536), (2, 5, 12, 1, 64, 4096), (2, 5, 12, 4, 64, 4096), (3, 37, 260, 4, 64, 4096), (4, 130, 12, 1, 64, 4096),
              (3, 5, 13, 1, 64, 4096), (2, 130, 260, 1, 128, 4096), (2, 16, 4096, 16, 64, 4096), (3, 96, 160, 1, 64, 4096)]


def test_plan_tiles_trips_and_bounds_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/match_host.cpp has its own main and includes ubr_match_plan.h; built with -fsanitize=address,undefined and run as a
    process of its own over the geometries of the GPU cases and the full event"""
    exe = str(tmp_path / "match_host")
    r = subprocess.run([H.cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "match_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([exe] + [str(v) for g in GEOMETRIES for v in g], capture_output=True, text=True)
    assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
    lines = p.stdout.strip().split("\n")
    rows = [[int(v) for v in l.split()[1:]] for l in lines if l.startswith("I ")]
    assert [tuple(r[:6]) for r in rows] == GEOMETRIES
    H.need_lib(LIB)
    for P, rows_, cols, time_bin, slots, capacity, T, chunks, select_trips, clear, summary, match, scratch in rows:
        rows_max = min(capacity, P * rows_ * cols)
        assert T == R.time_bins(rows_, time_bin) == M.time_bins(rows_, time_bin) and chunks == -(-T // M.CHUNK_BINS)
        assert select_trips == -(-rows_max // M.LANES) and clear == min(M.MAX_GRID, -(-slots * T // M.LANES)) and summary == slots // 4
        tiles = slots // M.TILE
        assert match == tiles * (tiles + 1) // 2
        assert scratch == 8 * slots * chunks + -(-4 * slots * T // 16) * 16 + -(-4 * rows_max // 16) * 16
        assert M.scratch_bytes(P, rows_, cols, time_bin, slots, capacity) == scratch
    assert lines[-1].split() == ["G", str(M.LANES), str(M.TRIP_PIXELS), str(M.MAX_GRID), str(M.TILE), str(M.CHUNK_BINS), str(M.MIN_SLOTS),
                                 str(M.MAX_SLOTS), str(M.MAX_TIME_BIN), str(M.MAX_SHIFT), str(M.MAX_BIN_PIXELS)]


# ------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------------
def _table(cand, pairs, scale=16):
    n = len(cand)
    full = torch.zeros((n, n, 4), dtype=torch.int64)
    for (i, j), row in pairs.items():
        full[i, j] = torch.tensor(row)
    return planes.PlaneTable(torch.tensor(cand, dtype=torch.int64).reshape(n, 6), full, scale)


#         cluster plane Q  bins t_min t_max
_CAND = [[3, 0, 100, 10, 0, 9],      # 0
         [5, 0, 40, 4, 2, 5],        # 1
         [8, 1, 80, 8, 0, 7],        # 2
         [9, 1, 100, 10, 0, 9],      # 3
         [12, 1, 0, 3, 4, 6],        # 4: pixels without charge
         [20, 2, 90, 9, 1, 9],       # 5
         [21, 2, 40, 5, 2, 6]]       # 6
#                  both I  Qi_in Qj_in
_PAIRS = {(0, 2): [8, 80, 90, 80],   # containment 1.0: a tie with (0, 3) that goes to the smaller number
          (0, 3): [10, 100, 100, 100],
          (1, 2): [4, 20, 40, 30],
          (1, 4): [2, 0, 20, 0],     # a partner without charge: NaN
          (0, 5): [9, 81, 95, 90],
          (1, 6): [4, 40, 40, 36],
          (2, 5): [7, 60, 70, 75],
          (3, 5): [9, 90, 95, 90],
          (3, 6): [5, 10, 50, 40],
          (2, 6): [0, 0, 0, 0]}      # no shared bin: no pair


def test_plane_table_on_hand_made_tables():
    tab = _table(_CAND, _PAIRS)
    assert len(tab) == 7 and tab.cluster.tolist() == [3, 5, 8, 9, 12, 20, 21] and tab.plane.tolist() == [0, 0, 1, 1, 1, 2, 2]
    assert tab.charge().tolist() == [c[2] / 16 for c in _CAND] and tab.bins.tolist() == [c[3] for c in _CAND] and tab.span().tolist() == [c[4:] for c in _CAND]
    assert tab.pairs() == sorted(p for p in _PAIRS if _PAIRS[p][0] > 0) and (2, 6) not in tab.pairs()
    con, iou, tio = tab.containment(), tab.charge_iou(), tab.time_iou()
    assert con[(0, 2)] == 1.0 and con[(0, 3)] == 1.0 and con[(1, 2)] == 0.5 and np.isnan(con[(1, 4)]) and con[(0, 5)] == 81 / 90
    assert iou[(0, 2)] == 80 / 100 and iou[(0, 3)] == 1.0 and iou[(1, 4)] == 0.0 and iou[(3, 6)] == 10 / 130
    assert tio[(0, 2)] == 8 / 10 and tio[(1, 4)] == 2 / 5 and tio[(0, 3)] == 1.0
    # ties go to the smaller candidate number; NaN is never the best; a candidate without a partner has (-1, NaN)
    best = tab.best(0, 1)
    assert best[0] == (2, 1.0) and best[1] == (2, 0.5) and sorted(best) == [0, 1]
    back = tab.best(1, 0)
    assert back[2] == (0, 1.0) and back[3] == (0, 1.0) and back[4][0] == -1 and np.isnan(back[4][1])
    assert tab.best(0, 1, by="charge_iou")[0] == (3, 1.0) and tab.best(0, 1, by="time_iou")[0] == (3, 1.0)
    assert tab.best(2, 1)[6] == (3, 0.25) and tab.best(1, 2)[2] == (5, 0.75)
    # mutual best: 0 and 2 choose each other (3 loses the tie at 0), 1 and 6, 3 and 5
    m = tab.matched(0.0)
    assert [(i, j) for i, j, _ in m] == sorted((i, j) for i, j, _ in m) and (0, 2) in [(i, j) for i, j, _ in m] and (0, 3) not in [(i, j) for i, j, _ in m]
    assert (1, 6, 1.0) in m and all(v >= 0.95 for _, _, v in tab.matched(0.95))
    assert m == [(0, 2, 1.0), (0, 5, 0.9), (1, 6, 1.0), (3, 5, 1.0)] and tab.triples(0.0) == [], "2 is matched to 0 but not to 5"
    assert [p[:2] for p in tab.matched(0.0, by="charge_iou")] == [(0, 3), (0, 5), (1, 6), (3, 5)]
    assert tab.triples(0.0, by="charge_iou") == [(0, 3, 5)] and tab.triples(0.95, by="charge_iou") == []
    with pytest.raises(ValueError, match="by must be one of"):
        tab.best(0, 1, by="purity")
    with pytest.raises(ValueError, match="two different planes"):
        tab.best(1, 1)
    with pytest.raises(ValueError, match="int64 candidates of 6 columns"):
        planes.PlaneTable(torch.zeros((3, 5), dtype=torch.int64), torch.zeros((3, 3, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="pair table"):
        planes.PlaneTable(torch.zeros((3, 6), dtype=torch.int64), torch.zeros((3, 2, 4), dtype=torch.int64))


def test_triples_an_empty_table_and_a_missing_plane():
    cand = [[0, 0, 50, 5, 0, 4], [1, 1, 50, 5, 0, 4], [2, 2, 50, 5, 0, 4], [3, 2, 10, 1, 9, 9]]
    full = {(0, 1): [5, 50, 50, 50], (0, 2): [5, 45, 50, 50], (1, 2): [5, 40, 50, 50]}
    tab = _table(cand, full)
    assert tab.matched(0.5) == [(0, 1, 1.0), (0, 2, 0.9), (1, 2, 0.8)] and tab.triples(0.5) == [(0, 1, 2)] and tab.triples(0.85) == []
    assert tab.best(2, 0)[3][0] == -1
    empty = _table([], {})
    assert len(empty) == 0 and empty.pairs() == [] and empty.matched() == [] and empty.triples() == [] and empty.best(0, 1) == {}
    assert empty.containment() == {} and empty.charge().tolist() == []
    two = _table([c for c in cand if c[1] != 1], {(0, 1): [5, 45, 50, 50]})       # plane 1 is missing
    assert two.matched(0.5) == [(0, 1, 0.9)] and two.triples(0.0) == [] and list(two.best(0, 1)) == [0] and two.best(0, 1)[0][0] == -1
    dark = _table([[0, 0, 0, 2, 0, 1], [1, 1, 0, 2, 0, 1]], {(0, 1): [2, 0, 0, 0]})                # Q = 0 on both sides
    assert np.isnan(dark.containment()[(0, 1)]) and np.isnan(dark.charge_iou()[(0, 1)]) and dark.time_iou()[(0, 1)] == 1.0
    assert dark.matched(0.0) == [] and dark.matched(0.0, by="time_iou") == [(0, 1, 1.0)]


def test_matches_read_and_matcher_refusals_without_a_device():
    cand = torch.arange(64 * 6, dtype=torch.int64).reshape(64, 6)
    pairs = torch.arange(64 * 64 * 4, dtype=torch.int64).reshape(64, 64, 4)
    prof = torch.full((64, 5), -1, dtype=torch.int32)
    m = planes.Matches(prof, cand, pairs, torch.tensor([3]), torch.tensor([0, 7]), 16, 2)
    tab = m.read()
    assert len(tab) == 3 and tab.candidates.tolist() == cand[:3].tolist() and tab.pair_table.tolist() == pairs[:3, :3].tolist()
    assert (tab.adc_scale, tab.time_bin, tab.dropped, m.slots) == (16, 2, 7, 64) and m.profiles().tolist() == [[2 ** 32 - 1] * 5] * 3
    with pytest.raises(OverflowError, match=r"70 candidates, slots=64"):
        planes.Matches(prof, cand, pairs, torch.tensor([70]), torch.tensor([6, 0]), 16, 1).read()
    fake = types.SimpleNamespace(planes=3, rows=37, cols=260, num_classes=4, capacity=128, device="cpu")
    for kw, message in ((dict(slots=96), "multiple of 64"), (dict(slots=32), "slots"), (dict(slots=8192), "slots"), (dict(min_pixels=0), "min_pixels"),
                        (dict(time_bin=3), "power of two"), (dict(time_bin=128), "time_bin"), (dict(row_shift=(0, 0)), "one entry per plane"),
                        (dict(row_shift=(0, 0, 4097)), "row_shift"), (dict(row_shift=(0, 0, 1.5)), "row_shift"), (dict(adc_scale=3), "adc_scale")):
        with pytest.raises(ValueError, match=message):
            planes.PlaneMatcher(fake, **kw)
    for change, message in ((dict(planes=1), "needs 2..4 planes"), (dict(planes=5), "needs 2..4 planes"), (dict(rows=4097), "outside the limits"),
                            (dict(rows=2048, cols=4096), "outside the limits")):
        with pytest.raises(ValueError, match=message):
            planes.PlaneMatcher(types.SimpleNamespace(**dict(vars(fake), **change)))
    with pytest.raises(ValueError, match="32-bit bin could overflow"):
        planes.PlaneMatcher(types.SimpleNamespace(**dict(vars(fake), rows=64, cols=4096)), time_bin=32)
    H.need_lib(LIB)
    pm = planes.PlaneMatcher(fake, 64, 3, 4, None, 16)
    assert pm.row_shift == (0, 0, 0) and pm.T == 10 and pm.profile.shape == (64, 10) and pm.pairs.shape == (64, 64, 4)
    assert pm.scratch.numel() * 8 == M.scratch_bytes(3, 37, 260, 4, 64, 128)
    with pytest.raises(TypeError, match="must be the Clusters"):
        pm(torch.zeros(3), torch.zeros((3, 37, 260)))


# ------------------------------------------------------------------------------------------------------------------------
# matched events
# ------------------------------------------------------------------------------------------------------------------------
def test_make_matched_event_is_deterministic_and_every_object_shares_its_time_span():
    a, b = synthetic.make_matched_event(3, 96, 160, 4, objects=5), synthetic.make_matched_event(3, 96, 160, 4, objects=5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    image, label, instance = a
    assert (image.dtype, label.dtype, instance.dtype) == (np.float32, np.uint8, np.int32) and image.shape == label.shape == instance.shape == (3, 96, 160)
    assert synthetic.make_matched_event(3, 96, 160, 5, objects=5)[0].tobytes() != image.tobytes()
    lit = instance >= 0
    assert ((image > 0) == lit).all() and ((label > 0) == lit).all() and set(np.unique(label)) <= {0, 1, 2} and instance.max() >= 2
    for k in range(instance.max() + 1):
        spans = [np.flatnonzero((instance[p] == k).any(1)) for p in range(3)]
        assert all(len(s) and (s == spans[0]).all() for s in spans), "object %d covers the same rows in every plane" % k
        assert len({int(label[p][instance[p] == k].max()) for p in range(3)}) == 1
    # a cluster is an object: the objects keep OBJECT_GAP pixels apart, so 8-connected clustering never joins two
    ids, table, count = R.clustered(R.label_of(image, label))
    for k in range(count):
        assert len(np.unique(instance[ids == k])) == 1
    for planes_ in (1, 2, 4):
        assert synthetic.make_matched_event(planes_, 40, 64, 1, objects=2)[2].shape == (planes_, 40, 64)
    with pytest.raises(ValueError, match="planes must be 1..4"):
        synthetic.make_matched_event(5, 40, 64, 1)


MATCH_SEEDS = (0, 1, 2)            # chosen on the CPU: the reference recovers the pairing of each
MIN_PIXELS = 10


@pytest.mark.parametrize("seed", MATCH_SEEDS)
def test_the_reference_recovers_the_instance_pairing_of_a_matched_event(seed):
    """3 x 96 x 160, five objects: an instance counts where it has at least MIN_PIXELS pixels in two planes.  matched(0.5) of
    the numpy reference's tables must be exactly those pairs: none missed, none added."""
    image, label, instance = synthetic.make_matched_event(3, 96, 160, seed, objects=5)
    ids, table, count = R.clustered(R.label_of(image, label))
    ref = R.match(ids, table, count, 4096, image, 16, MIN_PIXELS, 1, (0, 0, 0), 64)
    n = ref["n"]
    assert ref["ncand"] == n >= 6
    tab = planes.PlaneTable(torch.from_numpy(ref["candidates"][:n]), torch.from_numpy(np.ascontiguousarray(ref["pairs"][:n, :n])), 16)
    truth, of = R.truth_pairs(ids, table, instance, MIN_PIXELS)
    counted = {k for k in range(instance.max() + 1) if sum(int((instance[p] == k).sum()) >= MIN_PIXELS for p in range(3)) >= 2}
    assert counted and {of[a] for a, _ in truth} == counted, "every instance with enough pixels in two planes is in the truth"
    got = {(int(tab.cluster[i]), int(tab.cluster[j])) for i, j, _ in tab.matched(0.5)}
    assert got == truth, "missed %s, added %s" % (sorted(truth - got), sorted(got - truth))
    whole = {k for k in counted if sum(int((instance[p] == k).sum()) >= MIN_PIXELS for p in range(3)) == 3}
    assert {of[int(tab.cluster[i])] for i, _, _ in tab.triples(0.5)} == whole and len(tab.triples(0.5)) == len(whole)
