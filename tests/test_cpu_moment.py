"""ClusterMoments without a GPU: the numpy reference of tests/moment_ref.py against cases written out by hand and a brute-force
double loop; the weight rule on its edge values; libubresnet_moment.so's header is C99, and header, binding, reference, plan and
library agree on entry points and constants; the library stands alone and exports its binding's symbols; the ADDONS entry, its
include closure and a forced build; a missing library is a RuntimeError; every argument refusal returns UBM_EINVAL with a message
before any HIP call; the overflow bound and the launch plan as a stand-alone program under the host sanitizers
(tests/moment_host.cpp), and the pixel walk and the weight rule it shares with ClusterOverlap as another (tests/walk_host.cpp);
ShapeTable and the refusals of the Python surface that need no device."""
import importlib
import importlib.util
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import cluster_ref as CR
import moment_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ubresnet_amd")
HEADER = os.path.join(REPO, "include", "ubresnet_moment.h")
import cpu_helpers as H  # noqa: E402
from ubresnet_amd import _moment as M  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd import clusters, shapes  # noqa: E402

LIB = B.ADDONS["moment"].out
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def _one_cluster(shape, pixels, adc, label=1, C=4, scale=16):
    """the table row of one cluster made of `pixels` [(row, col)] of plane 0 with the ADC values `adc`"""
    ids, lab, view = np.full(shape, -1, np.int32), np.full(shape, 255, np.uint8), np.zeros(shape, f32)
    for (r, c), a in zip(pixels, adc):
        ids[0, r, c], lab[0, r, c], view[0, r, c] = 0, label, a
    return R.table(ids, lab, view, C, scale, 8, 1)[0]


def test_reference_single_pixel():
    row = _one_cluster((1, 9, 11), [(7, 5)], [2.5])
    assert row.tolist() == [1, 0, 0, 40, 280, 200, 1960, 1400, 1000, 0, 40, 0, 0]
    s = R.shape_of(row)
    assert s["centroid"] == (7.0, 5.0) and s["covariance"] == ((0.0, 0.0), (0.0, 0.0)) and s["extent"] == (0.0, 0.0)
    assert math.isnan(s["linearity"]) and s["axis"] == (0.0, 1.0)


@pytest.mark.parametrize("L", [2, 7, 64])
def test_reference_horizontal_line_far_from_the_origin(L):
    r0, c0 = 4000, 3900
    row = _one_cluster((1, 4001, 4000), [(r0, c0 + i) for i in range(L)], [3.0] * L)
    s = R.shape_of(row)
    assert s["covariance"][0] == (0.0, 0.0) and s["covariance"][1][0] == 0.0, "the variance across is exactly 0"
    assert s["covariance"][1][1] == (L * L - 1) / 12 and s["centroid"] == (float(r0), c0 + (L - 1) / 2)
    assert s["axis"] == (0.0, 1.0) and s["linearity"] == 1.0 and s["extent"] == (math.sqrt((L * L - 1) / 12), 0.0)


def test_reference_l_shape_against_a_double_loop():
    pixels = [(r, 3) for r in range(2, 9)] + [(8, c) for c in range(4, 8)]
    adc = [1.0 + 0.25 * i for i in range(len(pixels))]
    row = _one_cluster((1, 12, 12), pixels, adc, label=2)
    w = [int(np.rint(f32(a) * f32(16))) for a in adc]
    Q = sum(w)
    mr, mc = sum(wi * r for wi, (r, c) in zip(w, pixels)) / Q, sum(wi * c for wi, (r, c) in zip(w, pixels)) / Q
    cov = [[0.0, 0.0], [0.0, 0.0]]
    for wi, (r, c) in zip(w, pixels):
        for i, a in enumerate((r - mr, c - mc)):
            for j, b in enumerate((r - mr, c - mc)):
                cov[i][j] += wi * a * b / Q
    s = R.shape_of(row)
    assert row[0] == len(pixels) and row[3] == Q == row[R.TABLE_FIXED + 2] and row[1] == row[2] == 0
    assert abs(s["centroid"][0] - mr) < 1e-12 and abs(s["centroid"][1] - mc) < 1e-12
    assert np.allclose(np.array(s["covariance"]), np.array(cov), rtol=1e-12, atol=1e-12)
    evals, evecs = np.linalg.eigh(np.array(cov))
    assert np.allclose(np.array(s["extent"]) ** 2, evals[::-1], rtol=1e-10)
    v = evecs[:, 1] * (1 if evecs[1, 1] > 0 else -1)
    assert np.allclose(np.array(s["axis"]), v, atol=1e-10) and s["axis"][1] > 0
    assert abs(s["linearity"] - (1 - evals[0] / evals[1])) < 1e-10


def test_reference_uniform_square_has_linearity_zero():
    n = 6
    row = _one_cluster((1, 50, 50), [(20 + r, 30 + c) for r in range(n) for c in range(n)], [5.0] * (n * n))
    s = R.shape_of(row)
    assert s["covariance"] == (((n * n - 1) / 12, 0.0), (0.0, (n * n - 1) / 12)) and s["linearity"] == 0.0 and s["axis"] == (0.0, 1.0)
    assert s["extent"][0] == s["extent"][1] == math.sqrt((n * n - 1) / 12)


def test_the_weight_rule_on_its_edge_values():
    sub = np.float32(1e-45)
    assert sub > 0 and sub < np.finfo(f32).tiny
    v = np.array([0.0, -0.0, sub, 0.03125, 0.09375, 4095.9375, 4096.0, 1e30, np.inf, -1.0, -np.inf, np.nan], f32)
    w, clipped, odd = R.weight(v, 16)
    assert w.tolist() == [0, 0, 0, 0, 2, 65535, 65535, 65535, 65535, 0, 0, 0]
    assert clipped.tolist() == [False] * 6 + [True] * 3 + [False] * 3
    assert odd.tolist() == [False] * 9 + [True] * 3
    assert w.dtype == np.int64 and R.weight(np.array([0.15625, 1.5, 2.5, 65535.0, 65535.5], f32), 1)[0].tolist() == [0, 2, 2, 65535, 65535]
    assert R.weight(np.array([65535.0, 65536.0], f32), 1)[1].tolist() == [False, True]
    assert R.weight(np.array([255.99609375, 255.998046875, 256.0], f32), 256)[1].tolist() == [False, True, True]
    with pytest.raises(AssertionError):
        R.weight(v, 3)
    # the table counts them: weighted, clipped, odd
    row = _one_cluster((1, 1, 16), [(0, i) for i in range(len(v))], v.tolist())
    assert row[:4].tolist() == [5, 3, 3, 2 + 4 * 65535]
    # every edge value of the ADC maker lands on a lit pixel
    lit = np.zeros((2, 9, 40), bool)
    lit[:, ::2] = True
    field = R.adc(lit.shape, lit=lit)
    got = set(field[lit].view(np.uint32).tolist())
    assert field.dtype == f32 and set(R.EDGE_ADC.view(np.uint32).tolist()) <= got


def test_a_foreign_label_is_odd_and_nothing_else():
    ids, lab, view = np.zeros((1, 1, 3), np.int32), np.array([[[1, 4, 200]]], np.uint8), np.full((1, 1, 3), 2.0, f32)
    assert R.table(ids, lab, view, 4, 16, 2, 1).tolist() == [[1, 0, 2, 32, 0, 0, 0, 0, 0, 0, 32, 0, 0]]
    # rows at or past min(count, capacity) do not exist, and their pixels are skipped
    ids[0, 0, 2], lab[0, 0, 2] = 1, 0
    assert R.table(ids, lab, view, 4, 16, 1, 2).shape == (1, 13) and R.table(ids, lab, view, 4, 16, 5, 2)[1, 3] == 32


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_moment.h"\n'
                     'int main(void) {\n'
                     '  int (*m)(const int32_t*, const uint8_t*, const float*, int, float, long long*, int64_t, const unsigned long long*,\n'
                     '           int, int, int, void*) = ubm_moments;\n'
                     '  const char* (*e)(void) = ubm_last_error;\n'
                     '  int (*v)(void) = ubm_version;\n'
                     '  return m == 0 || e == 0 || v == 0 || UBM_OK != 0 || UBM_EINVAL != -1 || UBM_ELAUNCH != -2\n'
                     '         || UBM_MAX_ROWS * UBM_MAX_COLS < UBM_MAX_PLANE_PIXELS;\n}\n')
    r = subprocess.run([H.cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(ubm_[a-z_0-9]+)\s*\(", text)
    assert declared == M.SYMBOLS == ["ubm_moments", "ubm_last_error", "ubm_version"]
    names = "LANES|TRIP_PIXELS|MAX_GRID|SLOTS|MAX_CLASSES|TABLE_FIXED|MAX_ROWS|MAX_COLS|MAX_PLANE_PIXELS|MAX_WEIGHT|MAX_SCALE"
    constants = {k: int(v) for k, v in re.findall(r"#define\s+UBM_(%s)\s+(\d+)" % names, text)}
    assert constants == {k: getattr(M, k) for k in names.split("|")}
    assert (R.TABLE_FIXED, R.MAX_WEIGHT, R.MAX_ROWS, R.MAX_COLS, R.MAX_PLANE_PIXELS, R.MAX_SCALE, R.TRIP_PIXELS, R.SLOTS, R.MAX_GRID) == \
        (M.TABLE_FIXED, M.MAX_WEIGHT, M.MAX_ROWS, M.MAX_COLS, M.MAX_PLANE_PIXELS, M.MAX_SCALE, M.TRIP_PIXELS, M.SLOTS, M.MAX_GRID)
    assert M.MAX_CLASSES == 16 and M.MAX_PLANE_PIXELS == 2 ** 22 and M.COLUMNS == R.COLUMNS and len(M.COLUMNS) == M.TABLE_FIXED
    assert "{%s, Q_0 .. Q_{C-1}}" % ", ".join(M.COLUMNS) in raw
    for phrase in ("STORED", "are not touched", "are skipped", "ties to even", "no spinning", "goes to memory directly",
                   "Zero columns are not sent", "power of two", "below 2^62"):
        assert phrase in raw, phrase
    H.need_lib(LIB)
    assert M.lib().ubm_version() == M.BINDING.version() == 1


def test_library_stands_alone_and_exports_exactly_its_bindings_symbols():
    bd = M.BINDING
    assert bd.prefix == "ubm" and bd.path == LIB and os.path.basename(LIB) == "libubresnet_moment.so" and os.path.dirname(LIB) == PKG
    assert (M.LIB_PATH, M.SYMBOLS, M.lib, M.check) == (bd.path, bd.symbols, bd.lib, bd.check)
    H.need_lib(LIB)
    assert "libubresnet_" not in H.readelf("-d", LIB).replace("libubresnet_moment", "")
    assert sorted(n for n in H.defined_symbols(LIB) if re.match(r"ub[a-z]_", n)) == sorted(bd.symbols)
    others = [importlib.import_module("ubresnet_amd." + lib.binding).BINDING.prefix for t in (B.LIBS, B.EXTRAS, B.ADDONS)
              for n, lib in t.items() if n != "moment"]
    assert "ubm" not in others and len(set(others)) == len(others)
    tree = open(os.path.join(PKG, "_moment.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy)", tree, flags=re.M) and "from ._binding import Binding" in tree
    src = open(os.path.join(B.CSRC, B.ADDONS["moment"].sources[0])).read()
    assert '#include "../ubr_sat.h"' in src and '#include "../ubr_moment_plan.h"' in src and "SAT_EXPORTS(ubm, UBM_VERSION)" in src
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "Malloc" not in src and "hipFree" not in src and "Synchronize" not in src, "no allocation, free or sync"
    assert "cooperative" not in code.lower() and "while (true)" not in code and "__threadfence" not in code
    # the plan compiles without HIP: it reaches the shared scan plan and walk plan and nothing else, and none of the files names HIP
    # outside comments
    plan, shared, walk = (os.path.join(B.CSRC, f) for f in ("ubr_moment_plan.h", "ubr_scan_plan.h", "ubr_walk_plan.h"))
    assert _include_closure([plan]) == {os.path.realpath(shared), os.path.realpath(walk)}
    assert _include_closure([shared]) == set() and _include_closure([walk]) == set()
    for f in (plan, shared, walk):
        assert "hip" not in re.sub(r"//.*", "", open(f).read()).lower(), f
    assert re.findall(r"#\s*include\s*<([^>]+)>", open(plan).read() + open(shared).read() + open(walk).read()) == ["stdint.h"] * 2
    # the weight rule is host and device code: it reaches the walk plan alone, and HIP only behind its __HIPCC__ guard
    rule = os.path.join(B.CSRC, "ubr_adc_rule.h")
    assert _include_closure([rule]) == {os.path.realpath(walk)} and re.findall(r"#\s*include\s*<([^>]+)>", open(rule).read()) == ["stdint.h", "string.h"]
    assert '#include "../ubr_walk.h"' in src and '#include "../ubr_adc_rule.h"' in src and "weight_of(float" not in src


def test_a_missing_library_is_a_runtime_error(monkeypatch):
    nowhere = os.path.join(REPO, "no_such_dir", "libubresnet_moment.so")
    monkeypatch.setenv("UBM_LIB", nowhere)
    spec = importlib.util.spec_from_file_location("ubresnet_amd._moment_missing", os.path.join(PKG, "_moment.py"))
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert fresh.LIB_PATH == nowhere
    with pytest.raises(RuntimeError, match="is missing; build it with") as e:
        fresh.moments(0x1000, 0x2000, 0x3000, 4, 16.0, 0x4000, 8, 0x5000, 1, 2, 2)
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
    lib = B.ADDONS["moment"]
    assert isinstance(lib, B.Lib) and lib.sources == [os.path.join("extra", "ubr_moment.hip")] and lib.binding == "_moment"
    assert "moment" not in B.LIBS and "moment" not in B.EXTRAS and list(B.ADDONS)[:6] == ["blend", "sparse", "crop", "calib", "cluster", "moment"]
    listed = [os.path.realpath(os.path.join(B.CSRC, h)) for h in lib.headers]
    assert len(listed) == len(set(listed)) and set(listed) == _include_closure([os.path.join(B.CSRC, s) for s in lib.sources])
    assert os.path.realpath(HEADER) in listed and os.path.realpath(os.path.join(B.CSRC, "ubr_moment_plan.h")) in listed
    assert os.path.realpath(os.path.join(B.CSRC, "ubr_cluster_plan.h")) not in listed
    assert not set(B.SOURCES + B.HEADERS) & set(lib.sources + lib.headers), "source_hash() covers the network's library only"


def test_a_forced_build_of_moment_is_one_compile_and_one_link(monkeypatch, capsys):
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    capsys.readouterr()
    built = B.build_addons(force=True, only=["moment"])
    monkeypatch.undo()
    lib = B.ADDONS["moment"]
    src, obj = os.path.join(B.CSRC, lib.sources[0]), os.path.join(B.CSRC, "extra", "ubr_moment.o")
    assert built == [lib.out] and len(lines) == 2
    assert "-ffp-contract=off" in B.FLAGS and lines[0] == [B.HIPCC] + B.FLAGS + ["-c", src, "-o", obj]
    assert lines[1] == [B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib.out, obj]
    io = capsys.readouterr()
    assert io.out == "" and io.err.strip().split("\n") == [" ".join(c) for c in lines]


def test_entry_point_reports_moment_on_stderr_before_the_score_line(monkeypatch, capsys):
    import __graft_entry__ as entry
    for lib in [l for t in (B.LIBS, B.ADDONS, B.EXTRAS) for l in t.values()]:
        H.need_lib(lib.out)
    for f in ("build", "build_addons", "build_extras"):
        monkeypatch.setattr(B, f, lambda *a, **kw: None)
    capsys.readouterr()
    entry.build()
    io = capsys.readouterr()
    err = io.err.strip().split("\n")
    assert "moment" not in io.out and "built %s ABI version 1" % LIB in err
    assert err.index("built %s ABI version 1" % B.ADDONS["cluster"].out) < err.index("built %s ABI version 1" % LIB) < len(err) - 1
    assert err[-1] == "built %s ABI version 1" % B.EXTRAS["score"].out


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals: every call below is refused on the host, before any HIP call; the addresses are never dereferenced
# ------------------------------------------------------------------------------------------------------------------------
_P = 0x100000
_GOOD = dict(ids=_P, label=_P + 0x1000, view=_P + 0x2000, C=4, scale=16.0, table=_P + 0x4000, capacity=30, count=_P + 0x8000, P=2, rows=3,
             cols=5)
_BAD = {
    "null ids": (dict(ids=None), "null pointer (ids, label, view)"),
    "null label": (dict(label=None), "null pointer (ids, label, view)"),
    "null view": (dict(view=None), "null pointer (ids, label, view)"),
    "null table": (dict(table=None), "null pointer (table, count)"),
    "null count": (dict(count=None), "null pointer (table, count)"),
    "table alignment": (dict(table=_P + 0x4004), "8-byte aligned"),
    "count alignment": (dict(count=_P + 0x8004), "8-byte aligned"),
    "ids alignment": (dict(ids=_P + 8), "ids and view must be 16-byte"),
    "view alignment": (dict(view=_P + 0x2004), "ids and view must be 16-byte"),
    "label alignment": (dict(label=_P + 0x1001), "label 4-byte aligned"),
    "C 0": (dict(C=0), "C=0 must be 1..16"),
    "C 17": (dict(C=17), "C=17 must be 1..16"),
    "scale 0": (dict(scale=0.0), "adc_scale=0 must be a power of two in 1..256"),
    "scale 3": (dict(scale=3.0), "adc_scale=3 must be a power of two in 1..256"),
    "scale half": (dict(scale=0.5), "adc_scale=0.5 must be a power of two in 1..256"),
    "scale 512": (dict(scale=512.0), "adc_scale=512 must be a power of two in 1..256"),
    "scale negative": (dict(scale=-16.0), "must be a power of two in 1..256"),
    "scale nan": (dict(scale=float("nan")), "must be a power of two in 1..256"),
    "capacity 0": (dict(capacity=0), "capacity=0 must be >= 1"),
    "capacity negative": (dict(capacity=-5), "capacity=-5 must be >= 1"),
    "P 0": (dict(P=0), "must be positive"),
    "rows negative": (dict(rows=-3), "must be positive"),
    "cols 0": (dict(cols=0), "must be positive"),
    "rows 4097": (dict(rows=4097, cols=4), "rows must be at most 4096"),
    "cols 4097": (dict(rows=4, cols=4097), "cols at most 4096"),
    "plane above 2^22": (dict(rows=2048, cols=2049), "rows * cols must be at most 2^22"),
    "2^31 pixels": (dict(P=512, rows=1024, cols=4096), "below 2^31 pixels"),
    "table is view": (dict(table=_P + 0x2000), "table overlaps an input"),
    "table inside ids": (dict(table=_P + 64), "table overlaps an input"),
    "count inside table": (dict(count=_P + 0x4000 + 104), "table overlaps an input"),
}


@pytest.mark.parametrize("name", sorted(_BAD))
def test_moments_refusals_precede_any_hip_call(name):
    H.need_lib(LIB)
    change, message = _BAD[name]
    a = dict(_GOOD, **change)
    rc = M.lib().ubm_moments(a["ids"], a["label"], a["view"], a["C"], a["scale"], a["table"], a["capacity"], a["count"], a["P"], a["rows"],
                             a["cols"], None)
    msg = M.lib().ubm_last_error().decode()
    assert rc == -1 and msg.startswith("ubm_moments:") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match="ubm_moments"):
        M.check(rc, name)


# ------------------------------------------------------------------------------------------------------------------------
# the plan and the overflow bound as a program
# ------------------------------------------------------------------------------------------------------------------------
def test_plan_and_overflow_bound_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/moment_host.cpp has its own main and includes ubr_moment_plan.h; built with -fsanitize=address,undefined and run as a
    process of its own over every view of the GPU tests: the plan's walk is the shared walk plan's (which the next test holds), the
    clear grid, what the plan refuses, and the overflow bound at the largest accepted shape"""
    exe = str(tmp_path / "moment_host")
    r = subprocess.run([H.cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "moment_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    images = sorted(CR.VIEWS.values()) + [(2, 200, 300), (3, 200, 700)]
    args = [str(v) for im in images for v in im + (im[0] * im[1] * im[2], 4)]
    p = subprocess.run([exe] + args, capture_output=True, text=True)
    assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
    lines = p.stdout.strip().split("\n")
    rows = [[int(v) for v in l.split()[1:]] for l in lines if l.startswith("I ")]
    assert [tuple(r[:3]) for r in rows] == images
    for P, rows_, cols, pixels, trips, span, grid, clear in rows:
        assert pixels == P * rows_ * cols and trips == -(-pixels // M.TRIP_PIXELS)
        assert span == -(-trips // min(trips, M.MAX_GRID)) and grid == -(-trips // span) and clear == min(M.MAX_GRID, -(-pixels * 13 // M.LANES))
    assert dict((tuple(r[:3]), r[4]) for r in rows)[(2, 200, 300)] == 59, "the all-lit test spans many workgroups"
    bound = int(lines[-2].split()[1])
    # the overflow bound of the plan, at the largest accepted shape, is below 2^63 -- and below 2^62, as the header says
    assert lines[-2].startswith("B ") and bound == 65535 * 2 ** 22 * 4095 ** 2 and bound < 2 ** 62 < 2 ** 63
    # the closed form of the GPU test's largest plane stays inside it
    assert 65535 * 1024 * (4095 * 4096 * 8191 // 6) <= bound
    assert lines[-1].split() == ["G", str(M.LANES), str(M.TRIP_PIXELS), str(M.MAX_GRID), str(M.SLOTS), "4", str(M.SLOTS // 2)]


def test_shared_walk_and_weight_rule_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/walk_host.cpp has its own main and includes ubr_walk_plan.h and ubr_adc_rule.h, the walk and the weight rule that the
    moment and overlap libraries share; built with -fsanitize=address,undefined and -ffp-contract=off and run as a process of its
    own.  (a) the spans tile the trips and the lane slots tile the pixels in a buffer of exactly the pixels, from 1 pixel to a few
    trips past MAX_GRID * TRIP_PIXELS and at the full event; (b) the weight and its class of every edge ADC value and of every
    65521st float bit pattern, at every valid scale, bit for bit against moment_ref.weight"""
    exe = str(tmp_path / "walk_host")
    r = subprocess.run([H.cc(plus=True), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wall", "-Werror", "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "walk_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    stride, edge = 65521, R.EDGE_ADC.view(np.uint32)
    p = subprocess.run([exe, str(stride)] + ["%08x" % b for b in edge.tolist()], capture_output=True, text=True)
    assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
    lines = p.stdout.strip().split("\n")
    # (a)
    walks = {int(l.split()[1]): [int(v) for v in l.split()[2:]] for l in lines if l.startswith("W ")}
    full = M.MAX_GRID * M.TRIP_PIXELS
    assert set(walks) >= {1, 3 * M.TRIP_PIXELS + 1, full - 1, full, full + 1, full + 3 * M.TRIP_PIXELS + 5, 3 * 1008 * 3456}
    for n, (trips, span, grid) in walks.items():
        assert trips == -(-n // M.TRIP_PIXELS) and span == -(-trips // min(trips, M.MAX_GRID)) and grid == -(-trips // span) <= M.MAX_GRID
    assert walks[full] == [1024, 1, 1024] and walks[full + 1] == [1025, 2, 513] and walks[3 * 1008 * 3456] == [5103, 5, 1021]
    # (b)
    def classes(values, scale):
        w, clipped, odd = R.weight(values, scale)
        return w, np.where(odd, 2, np.where(clipped, 1, 0))
    scales = [1, 2, 4, 8, 16, 32, 64, 128, 256]
    sweep = np.arange(0, 2 ** 32, stride, dtype=np.uint64).astype(np.uint32)
    assert [int(l.split()[1]) for l in lines if l.startswith("S ")] == scales and len(sweep) > 65000
    for scale in scales:
        got = [[int(t, 16) if i == 0 else int(t) for i, t in enumerate(l.split()[2:])] for l in lines if l.startswith("E %d " % scale)]
        w, cls = classes(R.EDGE_ADC, scale)
        assert got == [[int(b), int(x), int(c)] for b, x, c in zip(edge, w, cls)], scale
        at = lines.index("S %d %d" % (scale, stride))
        packed = np.array([int(t, 16) for t in lines[at + 1].split()], np.int64)
        w, cls = classes(sweep.view(f32), scale)
        assert len(packed) == len(sweep) and np.array_equal(packed >> 2, w) and np.array_equal(packed & 3, cls), scale
        assert set(cls.tolist()) == {0, 1, 2} and (w[cls == 0] > 0).any()


# ------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------------
def _cluster_rows(n, C=4):
    rows = torch.zeros((n, 8 + C), dtype=torch.int64)
    rows[:, 1] = torch.arange(n, 0, -1) * 3
    return rows


def test_shape_table_against_the_reference():
    ids = np.full((1, 4001, 4000), -1, np.int32)
    lab, view = np.full(ids.shape, 255, np.uint8), np.zeros(ids.shape, f32)
    ids[0, 4000, 3900:3907], lab[0, 4000, 3900:3907], view[0, 4000, 3900:3907] = 0, 1, 3.0           # a line, far out
    for i in range(9):                                                                                  # a diagonal blob
        ids[0, 10 + i, 20 + 2 * i:23 + 2 * i], lab[0, 10 + i, 20 + 2 * i:23 + 2 * i] = 1, [0, 2, 2]
        view[0, 10 + i, 20 + 2 * i:23 + 2 * i] = [1.0 + i, 2.5, 0.125 * i]
    ids[0, 50, 50], lab[0, 50, 50], view[0, 50, 50] = 2, 3, 7.0                                         # one pixel
    ids[0, 60, 60:62], lab[0, 60, 60:62], view[0, 60, 60:62] = 3, 1, [-1.0, np.nan]                      # no charge at all
    for r in range(5):                                                                                  # a column: axis (1, 0)
        ids[0, 100 + r, 7], lab[0, 100 + r, 7], view[0, 100 + r, 7] = 4, 0, 4.0
    ids[0, 200:203, 9], lab[0, 200:203, 9], view[0, 200:203, 9] = 5, 2, [1e9, 1.0, 1.0]                  # clipped
    t = R.table(ids, lab, view, 4, 16, 8, 6)
    tab = shapes.ShapeTable(torch.from_numpy(t), clusters.ClusterTable(_cluster_rows(6), 4, ids.shape, 6), 16)
    assert len(tab) == 6 and tab.weighted.tolist() == [7, 26, 1, 0, 5, 3] and tab.clipped.tolist() == [0, 0, 0, 0, 0, 1]
    assert tab.odd.tolist() == [0, 0, 0, 2, 0, 0]
    assert tab.charge().tolist() == (t[:, 3] / 16).tolist() and tab.charge()[0] == 21.0 and tab.class_charge()[2].tolist() == [0, 0, 0, 7.0]
    frac = tab.charge_fractions()
    assert frac[0].tolist() == [0, 1, 0, 0] and bool(torch.isnan(frac[3]).all()) and abs(float(frac[1].sum()) - 1) < 1e-15
    want = [R.shape_of(row) for row in t]
    for name, got in (("centroid", tab.centroid()), ("extent", tab.extent()), ("axis", tab.axis())):
        ref = np.array([w[name] for w in want])
        assert got.dtype == torch.float64 and np.allclose(got.numpy(), ref, rtol=1e-13, atol=1e-13, equal_nan=True), name
    assert np.array_equal(tab.covariance().numpy(), np.array([w["covariance"] for w in want]), equal_nan=True), "formed exactly, rounded once"
    assert np.allclose(tab.linearity().numpy(), np.array([w["linearity"] for w in want]), rtol=1e-13, atol=1e-13, equal_nan=True)
    # by hand
    assert tab.covariance()[0].tolist() == [[0.0, 0.0], [0.0, 4.0]] and tab.extent()[0].tolist() == [2.0, 0.0]
    assert tab.axis()[0].tolist() == [0.0, 1.0] and float(tab.linearity()[0]) == 1.0 and tab.centroid()[0].tolist() == [4000.0, 3903.0]
    assert abs(float(tab.length()[0]) - math.sqrt(48)) < 1e-14 and float(tab.width()[0]) == 0.0
    assert tab.axis()[4].tolist() == [1.0, 0.0] and abs(float(tab.extent()[4][0]) - math.sqrt(2.0)) < 1e-15 and float(tab.extent()[4][1]) == 0.0
    assert tab.extent()[2].tolist() == [0.0, 0.0] and bool(torch.isnan(tab.linearity()[2])) and tab.axis()[2].tolist() == [0.0, 1.0]
    for q in (tab.centroid()[3], tab.covariance()[3], tab.extent()[3], tab.axis()[3], tab.linearity()[3]):
        assert bool(torch.isnan(q).all())
    assert 0 < float(tab.axis()[1][0]) < float(tab.axis()[1][1]) and 0.5 < float(tab.linearity()[1]) < 1
    with pytest.raises(ValueError, match="do not belong"):
        shapes.ShapeTable(torch.from_numpy(t[:5]), tab.clusters, 16)


def _fake_clusterer(rows=3, cols=5, planes=2, C=4, capacity=4):
    shape = (planes, rows, cols)
    cl = types.SimpleNamespace(planes=planes, rows=rows, cols=cols, num_classes=C, capacity=capacity, device="cpu",
                               ids=torch.full(shape, -1, dtype=torch.int32), root=torch.full(shape, -1, dtype=torch.int32),
                               table=torch.zeros((capacity, 8 + C), dtype=torch.int64), count=torch.zeros(1, dtype=torch.int64),
                               status=torch.zeros(1, dtype=torch.int64), label=None)
    return cl, clusters.Clusters(cl.ids, cl.root, cl.table, cl.count, cl.status)


def test_cluster_moments_refusals_without_a_device():
    cl, found = _fake_clusterer()
    for bad in (0, 3, 512, 16.0, True, -16, None):
        with pytest.raises(ValueError, match="adc_scale must be a power of two in 1..256"):
            shapes.ClusterMoments(cl, adc_scale=bad)
    for rows, cols in ((4097, 4), (4, 4097), (2048, 2049)):
        with pytest.raises(ValueError, match="outside the overflow limits"):
            shapes.ClusterMoments(types.SimpleNamespace(planes=1, rows=rows, cols=cols, num_classes=4, capacity=2, device="cpu"))
    cm = shapes.ClusterMoments(cl, adc_scale=16)
    assert cm.table.shape == (4, 13) and cm.table.dtype == torch.int64
    view = torch.zeros((2, 1, 3, 5))
    with pytest.raises(TypeError, match="must be the Clusters"):
        cm((cl.ids, cl.table), view)
    _, other = _fake_clusterer()
    with pytest.raises(ValueError, match="not the buffers of the clusterer"):
        cm(other, view)
    with pytest.raises(RuntimeError, match="holds no class map"):
        cm(found, view)
    cl.label = torch.zeros((2, 3, 5), dtype=torch.uint8)
    for bad, error, match in ((torch.zeros((2, 3, 6)), ValueError, "expected a view of"), (torch.zeros((3, 5)), ValueError, "expected a view of"),
                              (torch.zeros((2, 3, 5), dtype=torch.float16), TypeError, "must be float32"),
                              (np.zeros((2, 3, 5), f32), TypeError, "torch tensor or a sparse.SparseEvent")):
        with pytest.raises(error, match=match):
            cm(found, bad)
    from ubresnet_amd import sparse
    with pytest.raises(ValueError, match="sparse event is of a 2 x 3 x 6 image"):
        cm(found, sparse.SparseEvent(torch.zeros(1, dtype=torch.int32), torch.zeros(1), 2, 3, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cm(found, view)                                          # every argument is fine: the view is on the host
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cm(found, sparse.SparseEvent(torch.zeros(1, dtype=torch.int32), torch.zeros(1), 2, 3, 5))


def test_moments_read_without_a_device():
    cl, found = _fake_clusterer()
    cl.table[:3, 1] = torch.tensor([5, 1, 2])
    mine = torch.arange(4 * 13, dtype=torch.int64).reshape(4, 13)
    mom = shapes.Moments(mine, found, 16)
    assert shapes.Moments._fields == ("table", "clusters", "adc_scale")
    cl.count[0] = 9
    with pytest.raises(OverflowError, match="9 clusters, capacity 4"):
        mom.read()
    cl.count[0] = 3
    tab = mom.read()
    assert isinstance(tab, shapes.ShapeTable) and isinstance(tab.clusters, clusters.ClusterTable) and len(tab) == len(tab.clusters) == 3
    assert tab.rows.tolist() == mine[:3].tolist() and tab.clusters.total == 3 and tab.clusters.image == (2, 3, 5) and tab.adc_scale == 16
    big = mom.read(min_pixels=2)                                 # the filter comes from the cluster table, for both tables alike
    assert big.clusters.pixels.tolist() == [5, 2] and big.rows.tolist() == mine[[0, 2]].tolist() and big.clusters.total == 3
    with pytest.raises(ValueError, match="min_pixels"):
        mom.read(min_pixels=-1)
