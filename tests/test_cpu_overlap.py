"""ClusterOverlap without a GPU: libubresnet_overlap.so's header is C99, and header, binding, reference, plan and library agree on
entry points and constants; the library stands alone and exports its binding's symbols; the ADDONS entry, its include closure and
a forced build; every argument refusal returns UBH_EINVAL with a message before any HIP call; the plan, the key, the hash and the
insert-then-look-up model as a stand-alone program under the host sanitizers (tests/overlap_host.cpp); the numpy reference on a
hand-made image; OverlapTable on hand-made rows; and the condition that keeps the GPU tests honest: for the key set of every exact
GPU case the longest run of occupied slots in the reference model is below the probe limit, so no insertion order can drop a pair."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cluster_ref as CR
import overlap_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ubresnet_amd")
HEADER = os.path.join(REPO, "include", "ubresnet_overlap.h")
import cpu_helpers as H  # noqa: E402
from ubresnet_amd import _overlap as M  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd import overlap  # noqa: E402

LIB = B.ADDONS["overlap"].out
PLAN = os.path.join(B.CSRC, "ubr_overlap_plan.h")


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def test_reference_on_a_hand_made_image():
    a = np.array([[[0, 0, -1, 1], [-1, -3, 1, 1]]], np.int32)
    b = np.array([[[5, -1, -1, 5], [2, -1, 5, -9]]], np.int32)
    view = np.array([[[1.0, 2.5, 100.0, 0.0], [np.nan, 7.0, 0.03125, 5000.0]]], np.float32)
    assert R.table(a, b, view, 16).tolist() == [[0, 5, 0, 1, 1, 16], [0, -1, 1, 1, 1, 40], [1, 5, 3, 2, 0, 0], [-1, 2, 4, 1, 0, 0],
                                                [1, -1, 7, 1, 1, 65535]]
    assert R.table(a, b).tolist() == [[0, 5, 0, 1, 0, 0], [0, -1, 1, 1, 0, 0], [1, 5, 3, 2, 0, 0], [-1, 2, 4, 1, 0, 0], [1, -1, 7, 1, 0, 0]]
    assert R.keys_of(a, b).tolist() == [(1 << 32) | 6, 1 << 32, 0, (2 << 32) | 6, 3, 0, (2 << 32) | 6, 2 << 32]
    none = np.full((1, 2, 4), -1, np.int32)
    assert R.table(none, none, view).shape == (0, 6)


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_overlap.h"\n'
                     'int main(void) {\n'
                     '  int (*o)(const int32_t*, const int32_t*, const float*, float, long long*, int64_t, unsigned long long*,\n'
                     '           unsigned long long*, void*, int64_t, int, int, int, void*) = ubh_overlap;\n'
                     '  int64_t (*d)(int64_t) = ubh_default_slots;\n'
                     '  int64_t (*s)(int, int, int, int64_t) = ubh_scratch_bytes;\n'
                     '  const char* (*e)(void) = ubh_last_error;\n'
                     '  int (*v)(void) = ubh_version;\n'
                     '  return o == 0 || d == 0 || s == 0 || e == 0 || v == 0 || UBH_OK != 0 || UBH_EINVAL != -1 || UBH_ELAUNCH != -2\n'
                     '         || UBH_COLUMNS != 6 || UBH_MIN_SLOTS > UBH_MAX_PROBES;\n}\n')
    r = subprocess.run([H.cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_plan_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(ubh_[a-z_0-9]+)\s*\(", text)
    assert declared == M.SYMBOLS == ["ubh_default_slots", "ubh_scratch_bytes", "ubh_overlap", "ubh_last_error", "ubh_version"]
    names = "LANES|TRIP_PIXELS|MAX_GRID|LDS_SLOTS|COLUMNS|SLOT_WORDS|MAX_PROBES|MIN_SLOTS|MAX_SLOTS|MAX_WEIGHT|MAX_SCALE"
    constants = {k: int(v) for k, v in re.findall(r"#define\s+UBH_(%s)\s+(\d+)" % names, text)}
    assert constants == {k: getattr(M, k) for k in names.split("|")}
    assert (R.COLUMNS, R.MAX_PROBES, R.MIN_SLOTS, R.MAX_WEIGHT, R.TRIP_PIXELS, R.LDS_SLOTS, R.COLUMN_NAMES) == \
        (M.COLUMNS, M.MAX_PROBES, M.MIN_SLOTS, M.MAX_WEIGHT, M.TRIP_PIXELS, M.LDS_SLOTS, M.COLUMN_NAMES)
    assert "{%s}" % ", ".join(M.COLUMN_NAMES) in raw and len(M.COLUMN_NAMES) == M.COLUMNS and M.MAX_SLOTS == 2 ** 30
    plan = open(PLAN).read()
    assert "GOLDEN = 0x%Xull" % R.GOLDEN in plan and "0x%X" % R.GOLDEN in raw and "MAX_PROBES = %d;" % R.MAX_PROBES in plan
    assert "pixels < 2^31 and Q < 2^47" in raw and "Q is below 2^31 * 2^16 = 2^47" in plan
    for phrase in ("STORED", "ADDED to", "are not written", "ties to even", "no spinning", "goes to memory directly", "Zero columns are not sent",
                   "power of two", "never 0", "slots are never freed", "wholly in the table or wholly dropped", "is reserved and stays 0",
                   "same bytes on every run"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", raw), phrase          # (a phrase may run over a line of the comment)
    H.need_lib(LIB)
    assert M.lib().ubh_version() == M.BINDING.version() == 1
    for capacity in (1, 2, 511, 512, 513, 1000, 65536, 131072, 131073, 2 ** 29):
        s = M.default_slots(capacity)
        assert s == R.default_slots(capacity) and s & (s - 1) == 0 and s >= 1024 and capacity / s <= 0.5
    assert M.lib().ubh_default_slots(0) == 0 and M.lib().ubh_default_slots(2 ** 29 + 1) == 0
    assert M.scratch_bytes(3, 1008, 3456, 262144) == 262144 * 40 + 4 * 10208 and M.lib().ubh_scratch_bytes(3, 1008, 3456, 100) == 0
    with pytest.raises(RuntimeError, match="ubh_scratch_bytes refused"):
        M.scratch_bytes(0, 4, 4, 64)


def test_library_stands_alone_and_exports_exactly_its_bindings_symbols():
    bd = M.BINDING
    assert bd.prefix == "ubh" and bd.path == LIB and os.path.basename(LIB) == "libubresnet_overlap.so" and os.path.dirname(LIB) == PKG
    assert (M.LIB_PATH, M.SYMBOLS, M.lib, M.check) == (bd.path, bd.symbols, bd.lib, bd.check)
    H.need_lib(LIB)
    assert "libubresnet_" not in H.readelf("-d", LIB).replace("libubresnet_overlap", "")
    assert sorted(n for n in H.defined_symbols(LIB) if re.match(r"ub[a-z]_", n)) == sorted(bd.symbols)
    others = [importlib.import_module("ubresnet_amd." + lib.binding).BINDING.prefix for t in (B.LIBS, B.EXTRAS, B.ADDONS)
              for n, lib in t.items() if n != "overlap"]
    assert "ubh" not in others and len(set(others)) == len(others)
    tree = open(os.path.join(PKG, "_overlap.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy)", tree, flags=re.M) and "from ._binding import Binding" in tree
    src = open(os.path.join(B.CSRC, B.ADDONS["overlap"].sources[0])).read()
    assert '#include "../ubr_sat.h"' in src and '#include "../ubr_overlap_plan.h"' in src and "SAT_EXPORTS(ubh, UBH_VERSION)" in src
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "Malloc" not in src and "hipFree" not in src and "Synchronize" not in src, "no allocation, free or sync"
    assert "cooperative" not in code.lower() and "while (true)" not in code and "__threadfence" not in code
    assert len(re.findall(r"<<<", code)) == 5, "five launches"
    # the plan compiles without HIP: it reaches the shared scan plan and walk plan and nothing else, and names no HIP outside comments
    shared, walk = os.path.join(B.CSRC, "ubr_scan_plan.h"), os.path.join(B.CSRC, "ubr_walk_plan.h")
    assert _include_closure([PLAN]) == {os.path.realpath(shared), os.path.realpath(walk)}
    assert "hip" not in re.sub(r"//.*", "", open(PLAN).read()).lower()
    assert '#include "../ubr_walk.h"' in src and '#include "../ubr_adc_rule.h"' in src and "weight_of(float" not in src
    assert re.findall(r"#\s*include\s*<([^>]+)>", open(PLAN).read()) == []
    host = os.path.join(REPO, "tests", "overlap_host.cpp")
    assert re.findall(r'#\s*include\s*"([^"]+)"', open(host).read()) == ["ubr_overlap_plan.h", "ubr_scan_plan.h"]


def test_a_missing_library_is_a_runtime_error(monkeypatch):
    import importlib.util
    nowhere = os.path.join(REPO, "no_such_dir", "libubresnet_overlap.so")
    monkeypatch.setenv("UBH_LIB", nowhere)
    spec = importlib.util.spec_from_file_location("ubresnet_amd._overlap_missing", os.path.join(PKG, "_overlap.py"))
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert fresh.LIB_PATH == nowhere
    with pytest.raises(RuntimeError, match="is missing; build it with") as e:
        fresh.overlap(0x1000, 0x2000, None, 16.0, 0x4000, 8, 0x5000, 0x6000, 0x7000, 64, 1, 2, 2)
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
    lib = B.ADDONS["overlap"]
    assert isinstance(lib, B.Lib) and lib.sources == [os.path.join("extra", "ubr_overlap.hip")] and lib.binding == "_overlap"
    assert "overlap" not in B.LIBS and "overlap" not in B.EXTRAS
    assert list(B.ADDONS)[:7] == ["blend", "sparse", "crop", "calib", "cluster", "moment", "overlap"]
    listed = [os.path.realpath(os.path.join(B.CSRC, h)) for h in lib.headers]
    assert len(listed) == len(set(listed)) and set(listed) == _include_closure([os.path.join(B.CSRC, s) for s in lib.sources])
    assert os.path.realpath(HEADER) in listed and os.path.realpath(PLAN) in listed
    assert os.path.realpath(os.path.join(B.CSRC, "ubr_moment_plan.h")) not in listed
    assert not set(B.SOURCES + B.HEADERS) & set(lib.sources + lib.headers), "source_hash() covers the network's library only"


def test_a_forced_build_of_overlap_is_one_compile_and_one_link(monkeypatch, capsys):
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    capsys.readouterr()
    built = B.build_addons(force=True, only=["overlap"])
    monkeypatch.undo()
    lib = B.ADDONS["overlap"]
    src, obj = os.path.join(B.CSRC, lib.sources[0]), os.path.join(B.CSRC, "extra", "ubr_overlap.o")
    assert built == [lib.out] and len(lines) == 2
    assert lines[0] == [B.HIPCC] + B.FLAGS + ["-c", src, "-o", obj]
    assert lines[1] == [B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib.out, obj]
    io = capsys.readouterr()
    assert io.out == "" and io.err.strip().split("\n") == [" ".join(c) for c in lines]


def test_entry_point_reports_overlap_on_stderr_after_moment(monkeypatch, capsys):
    import __graft_entry__ as entry
    for lib in [l for t in (B.LIBS, B.ADDONS, B.EXTRAS) for l in t.values()]:
        H.need_lib(lib.out)
    for f in ("build", "build_addons", "build_extras"):
        monkeypatch.setattr(B, f, lambda *a, **kw: None)
    capsys.readouterr()
    entry.build()
    io = capsys.readouterr()
    err = io.err.strip().split("\n")
    assert "overlap" not in io.out and "built %s ABI version 1" % LIB in err
    assert err.index("built %s ABI version 1" % B.ADDONS["moment"].out) < err.index("built %s ABI version 1" % LIB) < len(err) - 1


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals: every call below is refused on the host, before any HIP call; the addresses are never dereferenced
# ------------------------------------------------------------------------------------------------------------------------
_P = 0x100000
_GOOD = dict(a=_P, b=_P + 0x1000, view=_P + 0x2000, scale=16.0, table=_P + 0x4000, capacity=30, count=_P + 0x8000, status=_P + 0x8100,
             scratch=_P + 0x10000, slots=64, P=2, rows=3, cols=5)
_BAD = {
    "null a": (dict(a=None), "null pointer (ids_a, ids_b)"),
    "null b": (dict(b=None), "null pointer (ids_a, ids_b)"),
    "null table": (dict(table=None), "null pointer (table, count, status, scratch)"),
    "null count": (dict(count=None), "null pointer (table, count, status, scratch)"),
    "null status": (dict(status=None), "null pointer (table, count, status, scratch)"),
    "null scratch": (dict(scratch=None), "null pointer (table, count, status, scratch)"),
    "a alignment": (dict(a=_P + 8), "must be 16-byte aligned"),
    "b alignment": (dict(b=_P + 0x1004), "must be 16-byte aligned"),
    "view alignment": (dict(view=_P + 0x2004), "must be 16-byte aligned"),
    "table alignment": (dict(table=_P + 0x4004), "8-byte aligned"),
    "count alignment": (dict(count=_P + 0x8004), "8-byte aligned"),
    "status alignment": (dict(status=_P + 0x8104), "8-byte aligned"),
    "scratch alignment": (dict(scratch=_P + 0x10008), "scratch must be 16-byte aligned"),
    "slots 0": (dict(slots=0), "slots=0 must be a power of two in 64..1073741824"),
    "slots 32": (dict(slots=32), "slots=32 must be a power of two in 64..1073741824"),
    "slots 96": (dict(slots=96), "slots=96 must be a power of two"),
    "slots negative": (dict(slots=-64), "slots=-64 must be a power of two"),
    "slots 2^31": (dict(slots=2 ** 31), "must be a power of two in 64..1073741824"),
    "capacity 0": (dict(capacity=0), "capacity=0 must be >= 1"),
    "capacity negative": (dict(capacity=-5), "capacity=-5 must be >= 1"),
    "scale 0": (dict(scale=0.0), "adc_scale=0 must be a power of two in 1..256"),
    "scale 3": (dict(scale=3.0), "adc_scale=3 must be a power of two in 1..256"),
    "scale half": (dict(scale=0.5), "adc_scale=0.5 must be a power of two in 1..256"),
    "scale 512": (dict(scale=512.0), "adc_scale=512 must be a power of two in 1..256"),
    "scale nan": (dict(scale=float("nan")), "must be a power of two in 1..256"),
    "scale 3 without a view": (dict(scale=3.0, view=None), "adc_scale=3 must be a power of two in 1..256"),
    "P 0": (dict(P=0), "must be positive"),
    "rows negative": (dict(rows=-3), "must be positive"),
    "cols 0": (dict(cols=0), "must be positive"),
    "2^31 pixels": (dict(P=512, rows=1024, cols=4096), "below 2^31 pixels"),
    "table is view": (dict(table=_P + 0x2000), "overlaps an input"),
    "table inside a": (dict(table=_P + 64), "overlaps an input"),
    "count inside table": (dict(count=_P + 0x4000 + 104), "overlaps an input"),
    "status is count": (dict(status=_P + 0x8000), "overlaps an input or one another"),
    "scratch over the table": (dict(scratch=_P + 0x4000 - 64 * 40), "scratch overlaps another buffer"),
    "scratch over b": (dict(scratch=_P + 0x1000), "scratch overlaps another buffer"),
}


@pytest.mark.parametrize("name", sorted(_BAD))
def test_overlap_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD[name]
    a = dict(_GOOD, **change)
    rc = M.lib().ubh_overlap(a["a"], a["b"], a["view"], a["scale"], a["table"], a["capacity"], a["count"], a["status"], a["scratch"], a["slots"],
                             a["P"], a["rows"], a["cols"], None)
    msg = M.lib().ubh_last_error().decode()
    assert rc == -1 and msg.startswith("ubh_overlap:") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match="ubh_overlap"):
        M.check(rc, name)


# ------------------------------------------------------------------------------------------------------------------------
# the plan, the hash and the insert as a program
# ------------------------------------------------------------------------------------------------------------------------
def _gpu_images():
    cases = R.clustered_cases()
    return sorted({(c[0].shape, R.default_slots(c[3])) for c in cases.values()} | {((2, 67, 133), 64)})


def test_plan_hash_and_insert_model_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/overlap_host.cpp has its own main and includes ubr_overlap_plan.h and ubr_scan_plan.h; built with
    -fsanitize=address,undefined and run as a process of its own over every image of the GPU cases"""
    exe = str(tmp_path / "overlap_host")
    r = subprocess.run([H.cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "overlap_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    images = _gpu_images()
    args = [str(v) for shape, slots in images for v in shape + (slots,)]
    p = subprocess.run([exe] + args, capture_output=True, text=True)
    assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
    lines = p.stdout.strip().split("\n")
    rows = [[int(v) for v in l.split()[1:]] for l in lines if l.startswith("I ")]
    assert [tuple(r[:3]) for r in rows] == [shape for shape, _ in images]
    for (shape, slots), (P, rows_, cols, pixels, trips, span, grid, clear, blocks, scratch) in zip(images, rows):
        assert pixels == P * rows_ * cols and trips == -(-pixels // M.TRIP_PIXELS) and blocks == -(-pixels // 1024)
        assert span == -(-trips // min(trips, M.MAX_GRID)) and grid == -(-trips // span) and clear == min(M.MAX_GRID, -(-slots // M.LANES))
        assert scratch == slots * M.SLOT_WORDS * 8 + 4 * (-(-blocks // 4) * 4)
        H.need_lib(LIB)
        assert M.scratch_bytes(P, rows_, cols, slots) == scratch
    by_shape = dict((tuple(r[:3]), r) for r in rows)
    assert by_shape[R.ALL_LIT][4] == 59 and by_shape[R.RAGGED][5] == 2, "the contended case spans 59 workgroups, the ragged one two trips each"
    assert lines[-1].split() == ["G", str(M.LANES), str(M.TRIP_PIXELS), str(M.MAX_GRID), str(M.LDS_SLOTS), "4", str(M.LDS_SLOTS // 2),
                                 str(M.COLUMNS), str(M.SLOT_WORDS), str(M.MAX_PROBES), str(M.MIN_SLOTS)]


def test_the_hash_model_is_the_plan_headers():
    """home slots of the Python model against constants worked out by hand from the multiplier, and the model's own laws"""
    assert R.home_slot(1, 64) == R.GOLDEN >> 58 == 39 and R.home_slot(1 << 32, 1024) == ((R.GOLDEN << 32) & R.MASK64) >> 54
    assert R.probes(64) == 64 and R.probes(128) == 128 and R.probes(1 << 20) == 128
    keys = [int(k) for k in np.random.default_rng(5).integers(1, 2 ** 62, 600)]
    first, dropped = R.occupied(keys, 1024)
    assert not dropped and len(first) == 600
    for seed in range(3):                                        # the occupied set does not depend on the order
        again, dropped = R.occupied(np.random.default_rng(seed).permutation(keys).tolist(), 1024)
        assert again == first and not dropped
    small, dropped = R.occupied(keys, 64)
    assert len(small) == 64 and len(dropped) == 600 - 64 and R.longest_run(small, 64) == 64
    assert R.longest_run({0, 1, 63}, 64) == 3 and R.longest_run({5}, 64) == 1 and R.longest_run(set(), 64) == 0
    t = dict(slots=64, held={})
    assert R.lookup(t, 77) == -1 and R.insert(t, 77) == R.lookup(t, 77) == R.home_slot(77, 64)


@pytest.mark.parametrize("name", sorted(R.clustered_cases()) + ["raw"])
def test_no_insertion_order_can_drop_a_pair_of_an_exact_gpu_case(name):
    """the longest cyclic run of occupied slots is below UBH_PROBES: a pair's probe sequence meets a free slot (or its own) before
    the limit whatever was inserted before it, so a nonzero status[0] on the device is a bug"""
    if name == "raw":
        a, b = R.raw_maps()
        capacity = a.size
    else:
        label, mode_a, mode_b, capacity = R.clustered_cases()[name]
        a, b = R.reference_ids(label, mode_a), R.reference_ids(label, mode_b)
    slots = R.default_slots(capacity)
    keys = np.unique(R.keys_of(a, b))
    keys = keys[keys != 0]
    taken, dropped = R.occupied(keys.tolist(), slots)
    assert not dropped and len(taken) == len(keys) <= slots // 2
    assert R.longest_run(taken, slots) < R.probes(slots), "a run of %d occupied slots" % R.longest_run(taken, slots)


# ------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------------
def _table(rows, scale=16):
    return overlap.OverlapTable(torch.tensor(rows, dtype=torch.int64).reshape(-1, 6), scale)


#        a   b  first pixels weighted Q
_ROWS = [[0, 0, 0, 6, 6, 60],
         [0, 1, 3, 2, 2, 100],
         [0, -1, 5, 2, 0, 0],
         [1, 1, 9, 3, 3, 30],
         [1, 2, 12, 3, 3, 90],           # a tie in pixels with (1, 1): the smaller first wins; in charge (1, 2) wins
         [2, -1, 20, 4, 4, 40],          # a cluster of a that nothing of b covers
         [-1, 2, 30, 5, 5, 50],
         [-1, 3, 40, 1, 1, 10],          # a cluster of b that nothing of a covers
         [3, 4, 50, 1, 0, 0]]            # a pair without charge


def test_overlap_table_on_hand_made_rows():
    tab = _table(_ROWS)
    assert len(tab) == 9 and tab.a.tolist() == [r[0] for r in _ROWS] and tab.first.tolist() == [r[2] for r in _ROWS]
    assert tab.pixels.tolist() == [r[3] for r in _ROWS] and tab.weighted.tolist() == [r[4] for r in _ROWS]
    assert tab.charge.tolist() == [r[5] / 16 for r in _ROWS] and tab.b.tolist() == [r[1] for r in _ROWS]
    assert tab.sizes_a() == {0: 10, 1: 6, 2: 4, 3: 1} and tab.sizes_b() == {0: 6, 1: 5, 2: 8, 3: 1, 4: 1}
    assert tab.sizes_a(weighted=True) == {0: 160, 1: 120, 2: 40, 3: 0} and tab.sizes_b(weighted=True) == {0: 60, 1: 130, 2: 140, 3: 10, 4: 0}
    pur = tab.purity()
    assert pur.cluster.tolist() == [0, 1, 2, 3] and pur.value.tolist() == [0.6, 0.5, 0.0, 1.0] and pur.best.tolist() == [0, 1, -1, 4]
    eff = tab.efficiency()
    assert eff.cluster.tolist() == [0, 1, 2, 3, 4] and eff.value.tolist() == [1.0, 0.6, 3 / 8, 0.0, 1.0] and eff.best.tolist() == [0, 1, 1, -1, 3]
    assert pur.value.dtype == torch.float64 and pur.best.dtype == torch.int64
    wp, we = tab.purity(weighted=True), tab.efficiency(weighted=True)
    assert wp.best.tolist() == [1, 2, -1, 4] and wp.value.tolist()[:3] == [100 / 160, 90 / 120, 0.0] and np.isnan(wp.value[3].item())
    assert we.best.tolist() == [0, 0, 1, -1, 3] and we.value.tolist()[:4] == [1.0, 100 / 130, 90 / 140, 0.0] and np.isnan(we.value[4].item())
    assert tab.matched() == [(0, 0, 0.6, 1.0), (1, 1, 0.5, 0.6), (3, 4, 1.0, 1.0)]
    assert tab.matched(0.55, 0.0) == [(0, 0, 0.6, 1.0), (3, 4, 1.0, 1.0)] and tab.matched(0.0, 0.7) == [(0, 0, 0.6, 1.0), (3, 4, 1.0, 1.0)]
    assert tab.matched(0.7, 0.7) == [(3, 4, 1.0, 1.0)]
    assert tab.unmatched_a() == [2] and tab.unmatched_b() == [2, 3] and tab.unmatched_a(0.7, 0.7) == [0, 1, 2]
    assert tab.unmatched_b(0.7, 0.7) == [0, 1, 2, 3]
    assert [(m[0], m[1]) for m in tab.matched(weighted=True)] == [(0, 1), (1, 2)], "(3, 4) has no charge: its purity is NaN and passes no threshold"
    with pytest.raises(ValueError, match="int64 rows of 6 columns"):
        overlap.OverlapTable(torch.zeros((3, 5), dtype=torch.int64))


def test_ari_against_a_brute_force_pair_count_and_its_edge_cases():
    rng = np.random.default_rng(6)
    for trial in range(4):
        a = rng.integers(-1, 4, (1, 6, 6)).astype(np.int32)
        b = rng.integers(-1, 3 + trial, (1, 6, 6)).astype(np.int32)
        got, want = _table(R.table(a, b).tolist()).ari(), R.ari_brute_force(a, b)
        assert abs(got - want) < 1e-12 and -1 <= got < 1, (got, want)
    a = rng.integers(0, 5, (1, 6, 6)).astype(np.int32)
    assert _table(R.table(a, a).tolist()).ari() == 1.0 == R.ari_brute_force(a, a)
    relabelled = (4 - a).astype(np.int32)
    assert _table(R.table(a, relabelled).tolist()).ari() == 1.0
    # below two pixels where both sides are >= 0: NaN
    assert np.isnan(_table([]).ari()) and np.isnan(_table([[0, 0, 0, 1, 0, 0], [1, -1, 1, 30, 0, 0], [-1, 2, 40, 30, 0, 0]]).ari())
    # a denominator of zero: both sides one cluster, and every pixel its own cluster on both sides
    assert _table([[0, 0, 0, 36, 0, 0]]).ari() == 1.0 and R.ari_brute_force(np.zeros((1, 6, 6), np.int32), np.zeros((1, 6, 6), np.int32)) == 1.0
    ident = np.arange(36, dtype=np.int32).reshape(1, 6, 6)
    assert _table(R.table(ident, ident).tolist()).ari() == 1.0 == R.ari_brute_force(ident, ident)
    # big counts stay exact: the binomial sums are Python integers (2^31 pixels squared pass 2^64)
    big = _table([[0, 0, 0, 2 ** 30, 0, 0], [0, 1, 1, 2 ** 30, 0, 0], [1, 1, 2, 2 ** 30, 0, 0]])
    n = 2 ** 30
    pairs = lambda m: m * (m - 1) // 2
    s_ab, s_a, s_b, s_n = 3 * pairs(n), pairs(2 * n) + pairs(n), pairs(n) + pairs(2 * n), pairs(3 * n)
    assert big.ari() == 2 * (s_ab * s_n - s_a * s_b) / ((s_a + s_b) * s_n - 2 * s_a * s_b)


def test_cluster_overlap_and_read_refusals_without_a_device():
    for bad in (0, 3, 512, 16.0, True):
        with pytest.raises(ValueError, match="adc_scale must be a power of two in 1..256"):
            overlap.ClusterOverlap(1, 4, 4, 8, 64, bad, "cpu")
    for kw in (dict(planes=0), dict(rows=-1), dict(cols=0), dict(capacity=0), dict(slots=32), dict(slots=96), dict(slots=2 ** 31),
               dict(planes=512, rows=1024, cols=4096)):
        with pytest.raises(ValueError):
            overlap.ClusterOverlap(**dict(dict(planes=1, rows=4, cols=4, capacity=8, slots=64, device="cpu"), **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        overlap.ClusterOverlap(1, 4, 4, 8, 64, 16, "cpu")
    assert overlap.Overlap._fields[:3] == ("table", "count", "status")
    table = torch.arange(4 * 6, dtype=torch.int64).reshape(4, 6)
    ov = overlap.Overlap(table, torch.tensor([3]), torch.tensor([0, 0]), 16, 1024)
    tab = ov.read()
    assert isinstance(tab, overlap.OverlapTable) and tab.rows.tolist() == table[:3].tolist() and tab.adc_scale == 16 and ov.capacity == 4
    with pytest.raises(OverflowError, match=r"9 pairs, capacity 4 \(slots=1024\)"):
        overlap.Overlap(table, torch.tensor([9]), torch.tensor([0, 0]), 16, 1024).read()
    with pytest.raises(OverflowError, match=r"7 pixels found no slot among slots=64"):
        overlap.Overlap(table, torch.tensor([2]), torch.tensor([7, 0]), 16, 64).read()


def test_truth_products_without_a_device():
    truth = torch.tensor([[[0, 1, 2], [2, -100, 1]]])
    view = torch.tensor([[[50.0, 10.0, 10.5], [float("nan"), 99.0, 11.0]]])
    label, conf = overlap.truth_products(truth, view)
    assert label.dtype == torch.uint8 and label.tolist() == [[[0, 255, 2], [255, 255, 1]]]
    assert conf.dtype == torch.float16 and conf.tolist() == [[[1.0] * 3] * 2]
    label, _ = overlap.truth_products(truth.to(torch.uint8), view[:, None], adc_threshold=60.0, fill_label=9, ignore_index=156)
    assert label.tolist() == [[[9, 9, 9], [9, 9, 9]]]
    label, _ = overlap.truth_products(truth, view[:, None], adc_threshold=0.0, ignore_index=2)
    assert label.tolist() == [[[0, 1, 255], [255, 255, 1]]]
    for bad, error in (((truth.float(), view), TypeError), ((truth, view.double()), TypeError), ((truth, view[:, :1]), ValueError)):
        with pytest.raises(error):
            overlap.truth_products(*bad)
