"""The scoring library without a GPU: libubresnet_score.so's header is C99; header, binding and library agree on the entry points
and constants; the library stands alone; the compiled kernels are exactly those the GPU module's case table runs; the second
build table and its commands; every argument refusal returns UBQ_EINVAL with a message before any launch; the numpy reference
against a brute-force computation; the inputs of the GPU cases reach every part of the table; EventScorer's argument errors."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import score_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ubresnet_amd")
HEADER = os.path.join(REPO, "include", "ubresnet_score.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
import cpu_helpers as H  # noqa: E402
from ubresnet_amd import _score as S  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd import scoring  # noqa: E402

LIB = B.EXTRAS["score"].out


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ubresnet_score.h"\n'
                   'int main(void) {\n'
                   '  int (*w)(int, int, int) = ubq_table_words;\n'
                   '  int (*f)(const uint8_t*, const uint16_t*, const void*, int, int, int, int, int, const uint16_t*, int,\n'
                   '           unsigned long long*, int, int, int, void*) = ubq_score_event;\n'
                   '  const char* (*e)(void) = ubq_last_error;\n'
                   '  int (*v)(void) = ubq_version;\n'
                   '  return w == 0 || f == 0 || e == 0 || v == 0 || UBQ_OK != 0 || UBQ_EINVAL != -1 || UBQ_ELAUNCH != -2\n'
                   '         || UBQ_MAX_CLASSES != 16 || UBQ_MAX_BINS != 32 || UBQ_MAX_RADIUS != 8 || UBQ_TRUTH_U8 != 0 || UBQ_TRUTH_I64 != 1;\n}\n')
    r = subprocess.run([H.cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(ubq_[a-z_0-9]+)\s*\(", text)
    assert declared == S.SYMBOLS == ["ubq_table_words", "ubq_score_event", "ubq_last_error", "ubq_version"]
    consts = {k: int(v) for k, v in re.findall(r"#define\s+UBQ_(MAX_CLASSES|MAX_BINS|MAX_RADIUS|TRUTH_U8|TRUTH_I64|TILE_H|TILE_W)\s+(\d+)", text)}
    assert consts == dict(MAX_CLASSES=S.MAX_CLASSES, MAX_BINS=S.MAX_BINS, MAX_RADIUS=S.MAX_RADIUS, TRUTH_U8=S.TRUTH_U8,
                          TRUTH_I64=S.TRUTH_I64, TILE_H=S.TILE_H, TILE_W=S.TILE_W)
    assert consts == dict(MAX_CLASSES=R.MAX_CLASSES, MAX_BINS=R.MAX_BINS, MAX_RADIUS=R.MAX_RADIUS, TRUTH_U8=R.U8, TRUTH_I64=R.I64,
                          TILE_H=R.TILE_H, TILE_W=R.TILE_W)
    for phrase in ("ADDED to", "HOST pointer", "modulo 2^64", "2^23 pixels", "0x8000 counts as zero", "(1024 + m) << (e - 1)"):
        assert phrase in raw, phrase
    H.need_lib(LIB)
    assert S.lib().ubq_version() == S.BINDING.version() == 1


def test_library_stands_alone_and_exports_exactly_its_bindings_symbols():
    bd = S.BINDING
    assert bd.prefix == "ubq" and bd.path == LIB and os.path.basename(LIB) == "libubresnet_score.so" and os.path.dirname(LIB) == PKG
    assert bd.symbols[-2:] == ["ubq_last_error", "ubq_version"]
    assert (S.LIB_PATH, S.SYMBOLS, S.lib, S.check) == (bd.path, bd.symbols, bd.lib, bd.check)
    H.need_lib(LIB)
    assert "libubresnet_" not in H.readelf("-d", LIB).replace("libubresnet_score", "")
    assert sorted(n for n in H.defined_symbols(LIB) if re.match(r"ub[a-z]_", n)) == sorted(bd.symbols)
    others = [importlib.import_module("ubresnet_amd." + lib.binding).BINDING.prefix for lib in B.LIBS.values()]
    assert "ubq" not in others
    tree = open(os.path.join(PKG, "_score.py")).read()
    assert not re.search(r"^\s*(import|from)\s+torch", tree, flags=re.M) and "from ._binding import Binding" in tree


def test_a_missing_library_is_a_runtime_error(monkeypatch):
    nowhere = os.path.join(REPO, "no_such_dir", "libubresnet_score.so")
    monkeypatch.setenv("UBQ_LIB", nowhere)
    spec = importlib.util.spec_from_file_location("ubresnet_amd._score_missing", os.path.join(PKG, "_score.py"))
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert fresh.LIB_PATH == nowhere
    with pytest.raises(RuntimeError, match="is missing; build it with") as e:
        fresh.lib()
    assert nowhere in str(e.value) and "There is no CPU fallback" in str(e.value)
    with pytest.raises(RuntimeError, match="is missing"):
        fresh.table_words(1, 1, 1)


def test_the_compiled_kernels_are_the_case_table():
    H.need_lib(LIB)
    assert kernel_symbols.kernels(LIB) == sorted(R.KERNEL_CASES)
    ids = [i for v in R.KERNEL_CASES.values() for i in v]
    assert all(R.KERNEL_CASES.values()) and len(ids) == len(set(ids))
    assert H.case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_score_exact.py")) == set(ids)


# ------------------------------------------------------------------------------------------------------------------------
# the second build table
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


def test_the_extras_table():
    assert list(B.EXTRAS) == ["score"] and not set(B.EXTRAS) & set(B.LIBS)
    lib = B.EXTRAS["score"]
    assert isinstance(lib, B.Lib) and lib.sources == [os.path.join("extra", "ubr_score.hip")] and lib.binding == "_score"
    assert os.path.exists(os.path.join(B.CSRC, lib.sources[0])) and os.path.exists(os.path.join(PKG, "_score.py"))
    listed = [os.path.realpath(os.path.join(B.CSRC, h)) for h in lib.headers]
    assert len(listed) == len(set(listed)) and set(listed) == _include_closure([os.path.join(B.CSRC, lib.sources[0])])
    assert os.path.realpath(HEADER) in listed
    # source_hash() still covers the network's library only
    assert not set(B.SOURCES + B.HEADERS) & set(lib.sources + lib.headers)


def test_a_forced_build_of_the_extras_is_one_compile_and_one_link(monkeypatch, capsys):
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    capsys.readouterr()
    built = B.build_extras(force=True)
    monkeypatch.undo()
    lib = B.EXTRAS["score"]
    src, obj = os.path.join(B.CSRC, lib.sources[0]), os.path.join(B.CSRC, "extra", "ubr_score.o")
    assert built == [lib.out] and len(lines) == 2
    assert lines[0] == [B.HIPCC] + B.FLAGS + ["-c", src, "-o", obj]
    assert lines[1] == [B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib.out, obj]
    io = capsys.readouterr()
    assert io.out == "" and io.err.strip().split("\n") == [" ".join(c) for c in lines]        # the echo goes to stderr
    with pytest.raises(ValueError, match="no library named"):
        B.build_extras(only=["hip"])


def test_the_command_line_builds_the_extras_after_the_table(monkeypatch, capsys):
    import runpy
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    monkeypatch.setattr("sys.argv", ["build.py", "--force", "--extras"])
    capsys.readouterr()
    runpy.run_module("ubresnet_amd.build", run_name="__main__")
    monkeypatch.undo()
    io = capsys.readouterr()
    out = io.out.strip().split("\n")
    assert len(lines) == 35 and lines[-1][lines[-1].index("-o") + 1] == LIB
    assert out[33:] == [lib.out for lib in B.LIBS.values()] + [LIB]
    err = io.err.strip().split("\n")
    assert all(" ".join(c) in err and " ".join(c) not in out for c in lines[33:]), "the extras' echo goes to stderr"


def test_entry_point_reports_the_extras_on_stderr(monkeypatch, capsys):
    import __graft_entry__ as entry
    for lib in list(B.LIBS.values()) + [B.EXTRAS["score"]]:
        H.need_lib(lib.out)
    calls = []
    monkeypatch.setattr(B, "build", lambda *a, **kw: calls.append(("build", a, kw)))
    monkeypatch.setattr(B, "build_extras", lambda *a, **kw: calls.append(("extras", a, kw)))
    capsys.readouterr()
    entry.build()
    io = capsys.readouterr()
    assert [c[0] for c in calls] == ["build", "extras"] and not calls[1][1] and not calls[1][2].get("only")
    out = io.out.strip().split("\n")
    assert len(out) == 14 and all(l.startswith("built ") for l in out) and "score" not in io.out
    assert io.err.strip().split("\n")[-1] == "built %s ABI version 1" % LIB


def test_entry_point_refuses_a_score_library_that_lacks_a_symbol(monkeypatch):
    import __graft_entry__ as entry
    H.need_lib(LIB)
    monkeypatch.setattr(B, "build", lambda *a, **kw: None)
    monkeypatch.setattr(B, "build_extras", lambda *a, **kw: None)
    monkeypatch.setitem(S.BINDING.table, "ubq_no_such_call", (C.c_int, []))
    monkeypatch.setattr(S.BINDING, "_lib", None)
    with pytest.raises(RuntimeError, match="lacks symbols") as e:
        entry.build()
    assert "libubresnet_score.so" in str(e.value) and "ubq_no_such_call" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals: null device pointers throughout, so nothing below can launch
# ------------------------------------------------------------------------------------------------------------------------
def test_table_words():
    H.need_lib(LIB)
    lib = S.lib()
    for P, Cn, bins in ((1, 1, 1), (3, 4, 10), (2, 16, 32), (65535, 16, 32)):
        assert lib.ubq_table_words(P, Cn, bins) == R.words(P, Cn, bins) == S.table_words(P, Cn, bins)
    for P, Cn, bins, msg in ((0, 4, 10, "P=0"), (-1, 4, 10, "P=-1"), (1, 0, 10, "C=0"), (1, 17, 10, "C=17"), (1, 4, 0, "bins=0"),
                             (1, 4, 33, "bins=33"), (1 << 22, 16, 32, "do not fit an int")):
        assert lib.ubq_table_words(P, Cn, bins) == -1
        assert lib.ubq_last_error().decode().startswith("ubq_table_words:") and msg in lib.ubq_last_error().decode()
        with pytest.raises(RuntimeError, match="ubq_table_words"):
            S.table_words(P, Cn, bins)


_HALF = lambda x: int(np.float16(x).view(np.uint16))  # noqa: E731
_GOOD = dict(kind=0, C=4, fill=255, radius=2, lo=1, edges=[_HALF(0.25), _HALF(0.5), _HALF(0.75)], bins=4, P=2, rows=8, cols=8)
_BAD = {
    "truth_kind 2": (dict(kind=2), "truth_kind=2"),
    "truth_kind negative": (dict(kind=-1), "truth_kind=-1"),
    "C 0": (dict(C=0), "C=0 must be 1..16"),
    "C 17": (dict(C=17), "C=17 must be 1..16"),
    "fill_label 256": (dict(fill=256), "fill_label=256"),
    "fill_label negative": (dict(fill=-1), "fill_label=-1"),
    "radius 9": (dict(radius=9), "radius=9 must be 0..8"),
    "radius negative": (dict(radius=-1), "radius=-1 must be 0..8"),
    "interface_from above C": (dict(lo=5), "interface_from=5 must be 0..C=4"),
    "interface_from negative": (dict(lo=-1), "interface_from=-1"),
    "bins 0": (dict(bins=0, edges=[]), "bins=0 must be 1..32"),
    "bins 33": (dict(bins=33, edges=list(range(1, 33))), "bins=33 must be 1..32"),
    "P 0": (dict(P=0), "P=0"),
    "P 65536": (dict(P=65536), "P=65536"),
    "rows 0": (dict(rows=0), "rows=0"),
    "cols negative": (dict(cols=-3), "cols=-3"),
    "edges null": (dict(edges=None), "edges_host is null"),
    "edges equal": (dict(edges=[_HALF(0.25), _HALF(0.5), _HALF(0.5)]), "not strictly ascending at 2"),
    "edges descending": (dict(edges=[_HALF(0.5), _HALF(0.25), _HALF(0.75)]), "not strictly ascending at 1"),
    "edge zero": (dict(edges=[0x0000, _HALF(0.5), _HALF(0.75)]), "edge 0 (0x0000) is not a positive finite half"),
    "edge negative": (dict(edges=[_HALF(0.25), _HALF(-0.5), _HALF(0.75)]), "edge 1 (0xB800) is not a positive finite half"),
    "edge negative zero": (dict(edges=[0x8000, _HALF(0.5), _HALF(0.75)]), "edge 0 (0x8000)"),
    "edge inf": (dict(edges=[_HALF(0.25), _HALF(0.5), 0x7C00]), "edge 2 (0x7C00) is not a positive finite half"),
    "edge nan": (dict(edges=[_HALF(0.25), _HALF(0.5), 0x7E00]), "edge 2 (0x7E00) is not a positive finite half"),
    "null pointers": (dict(), "null pointer"),
}


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    H.need_lib(LIB)
    change, message = _BAD[name]
    a = dict(_GOOD)
    a.update(change)
    edges = None if a["edges"] is None else (C.c_uint16 * max(len(a["edges"]), 1))(*a["edges"])
    lib = S.lib()
    rc = lib.ubq_score_event(None, None, None, a["kind"], a["C"], a["fill"], a["radius"], a["lo"], edges, a["bins"], None,
                             a["P"], a["rows"], a["cols"], None)
    msg = lib.ubq_last_error().decode()
    assert rc == -1 and msg.startswith("ubq_score_event:") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match="ubq_score_event"):
        S.check(rc, name)


def test_one_bin_needs_no_edges():
    """bins == 1 with a null edges_host passes the edge checks: the refusal is the null device pointers'"""
    H.need_lib(LIB)
    lib = S.lib()
    assert lib.ubq_score_event(None, None, None, 0, 4, 255, 2, 1, None, 1, None, 2, 8, 8, None) == -1
    assert "null pointer" in lib.ubq_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def test_fix_is_the_half_times_two_to_the_24_for_every_non_negative_finite_pattern():
    """31 744 patterns 0x0000..0x7BFF; with the sign bit set the magnitudes are the same 31 744, 63 488 finite patterns in all"""
    bits = np.arange(0x0000, 0x7C00, dtype=np.uint16)
    negative = bits | np.uint16(0x8000)
    assert bits.size + negative.size == 63488 and np.isfinite(negative.view(np.float16)).all()
    assert np.array_equal(R.fix(negative & np.uint16(0x7FFF)), (-negative.view(np.float16).astype(np.float64) * 2.0 ** 24).astype(np.uint64))
    value = bits.view(np.float16).astype(np.float64) * 2.0 ** 24
    assert np.array_equal(value, np.floor(value)) and value.max() < 2.0 ** 41
    assert np.array_equal(R.fix(bits), value.astype(np.uint64))
    assert R.fix(0x0001) == 1 and R.fix(0x03FF) == 1023 and R.fix(0x0400) == 1024 and R.fix(0x3C00) == 1 << 24 and R.fix(0x7BFF) == 65504 << 24


def _brute(label, conf, truth, Cn, fill, radius, lo, edges):
    """bincount for the confusion, an explicit double loop for the window, per-pixel Python for the bins"""
    P, rows, cols = label.shape
    bins = len(edges) + 1
    t = torch.from_numpy(truth.astype(np.int64)) if truth.dtype != np.int64 else torch.from_numpy(truth)
    valid = (t >= 0) & (t < Cn)
    lab = torch.from_numpy(label.astype(np.int64))
    lit = lab != fill
    scored = lit & valid & (lab < Cn)
    s = torch.zeros(label.shape, dtype=torch.int64)
    for p in range(P):
        for y in range(rows):
            for x in range(cols):
                if radius > 0 and valid[p, y, x] and t[p, y, x] >= lo:
                    w = t[p, max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1]
                    wv = valid[p, max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1]
                    s[p, y, x] = int(bool((wv & (w >= lo) & (w != t[p, y, x])).any()))
    cf = torch.stack([torch.stack([torch.bincount((t[p] * Cn + lab[p])[scored[p] & (s[p] == k)], minlength=Cn * Cn).view(Cn, Cn)
                                   for k in (0, 1)]) for p in range(P)])
    half = conf.view(np.float16).astype(np.float64)
    rel = np.zeros((P, 2, bins, 3), dtype=object)
    nonfinite = np.zeros(P, np.int64)
    edge_values = [float(np.array(e, np.uint16).view(np.float16)) for e in edges]
    for p, y, x in zip(*np.nonzero(scored.numpy())):
        v = half[p, y, x]
        if not np.isfinite(v) or v < 0:
            nonfinite[p] += 1
            continue
        b = sum(1 for e in edge_values if e <= v)
        rel[p, int(s[p, y, x]), b] += np.array([1, int(lab[p, y, x] == t[p, y, x]), int(v * 2.0 ** 24)], dtype=object)
    tally = np.stack([scored.sum((1, 2)).numpy(), (lit & ~scored).sum((1, 2)).numpy(), (~lit & valid & (t >= 1)).sum((1, 2)).numpy(), nonfinite], 1)
    return cf.numpy(), rel, tally


@pytest.mark.parametrize("kind", [R.U8, R.I64], ids=["u8", "i64"])
def test_reference_against_brute_force(kind):
    P, rows, cols, Cn, radius, lo, bins = 2, 23, 31, 4, 2, 1, 10
    edges = R.equal_edges(bins)
    label, conf, truth = R.make_event(3, P, rows, cols, Cn, kind, edges=edges)
    table = R.reference(label, conf, truth, Cn, 255, radius, lo, edges, np.zeros(R.words(P, Cn, bins), np.uint64))
    cf, rel, tally = R.unpack(table, P, Cn, bins)
    bcf, brel, btally = _brute(label, conf, truth, Cn, 255, radius, lo, edges)
    assert np.array_equal(cf.astype(np.int64), bcf) and np.array_equal(tally.astype(np.int64), btally)
    assert np.array_equal(rel.astype(object), brel)
    assert (cf.sum((0, 2, 3)) > 0).all() and (tally > 0).all()
    # the same table through Score: the float64 ECE by hand, the metrics of the summed confusion
    from ubresnet_amd import metrics
    sc = scoring.Score(table[None], P, Cn, edges)
    n, c, f = (brel.sum((0, 1))[:, i].astype(np.float64) for i in range(3))
    keep = n > 0
    ece = float((n[keep] / n.sum() * np.abs(c[keep] / n[keep] - f[keep] / (2.0 ** 24 * n[keep]))).sum())
    assert abs(sc.ece() - ece) <= 1e-15 * ece and ece > 0.0        # (the inputs hold confidences up to 65504)
    cm = torch.from_numpy(bcf.sum((0, 1)))
    assert torch.equal(sc.confusion(), cm) and torch.equal(sc.confusion("interface", 1), torch.from_numpy(bcf[1, 1]))
    assert sc.accuracy() == metrics.accuracy_from_confusion(cm, track_shower=True) and sc.iou() == metrics.iou(cm)
    assert sc.tallies() == dict(zip(("scored", "ignored", "dark", "nonfinite"), btally.sum(0).tolist()))
    assert sc.reliability()["pixels"] == [int(v) for v in n] and "interface" in str(sc) and "ECE" in str(sc)
    # summing events in Python ints does not wrap
    big = np.full((2, table.size), np.uint64(1) << np.uint64(63))
    assert int(scoring.Score(big, P, Cn, edges).total[0]) == 1 << 64


def test_reference_rules_by_hand():
    """one row of five pixels, C = 3, lo = 1, radius 1: classes 1 2 0 1 1"""
    truth = np.array([[[1, 2, 0, 1, 1]]], np.uint8)
    label = np.array([[[1, 1, 255, 255, 7]]], np.uint8)
    conf = np.array([[[0x3C00, 0x3800, 0x7E00, 0, 0x3C00]]], np.uint16)
    edges = [0x3800]                                                        # one edge at 0.5: 0.5 itself is in the upper bin
    t = R.reference(label, conf, truth, 3, 255, 1, 1, edges, np.zeros(R.words(1, 3, 2), np.uint64))
    cf, rel, tally = R.unpack(t, 1, 3, 2)
    assert tally.tolist() == [[2, 1, 1, 0]]                                 # pixel 4: label 7 is ignored; pixel 3: dark; pixel 2: background, not lit
    assert cf[0, 1, 1, 1] == 1 and cf[0, 1, 2, 1] == 1 and cf.sum() == 2    # both scored pixels touch the other class
    assert rel[0, 1, 1].tolist() == [2, 1, (1 << 24) + (1 << 23)] and rel[0, 0].sum() == 0
    assert not R.interface(R.classes(truth, 3), 1, 0).any()
    assert R.interface(R.classes(truth, 3), 0, 1).tolist() == [[[True, True, True, True, False]]]
    assert R.classes(np.array([2 ** 40 + 1, -1, 3, 2], np.int64), 3).tolist() == [-1, -1, -1, 2]


def test_the_inputs_of_the_gpu_cases_reach_every_part_of_the_table():
    """the reference alone, on the inputs the GPU grid uses: both strata, at least three bins and all four tallies move"""
    for kind in (R.U8, R.I64):
        for Cn in (3, 16):
            edges = R.equal_edges(10)
            for shape in R.BASE_SHAPES:
                label, conf, truth = R.make_event(100 + Cn, *shape, Cn, kind, edges=edges)
                t = R.reference(label, conf, truth, Cn, 255, 2, 1, edges, np.zeros(R.words(shape[0], Cn, 10), np.uint64))
                cf, rel, tally = R.unpack(t, shape[0], Cn, 10)
                assert (cf.sum((2, 3)) > 0).all(), "both strata of both planes"
                assert ((rel[:, :, :, 0] > 0).sum(2) >= 3).all(), "three bins or more in each stratum"
                assert (tally > 0).all(), "scored, ignored, dark and non-finite"
                assert int(tally[:, :2].sum()) == int((label != 255).sum())
    # the view spans two tiles and a ragged one in each direction
    for P, rows, cols in R.BASE_SHAPES:
        assert R.TILE_H < rows < 2 * R.TILE_H and R.TILE_W < cols < 2 * R.TILE_W and rows % R.TILE_H and cols % R.TILE_W
    assert [s[2] % 4 for s in R.BASE_SHAPES] == [2, 0]
    src = open(os.path.join(B.CSRC, B.EXTRAS["score"].sources[0])).read()
    assert int(re.search(r"constexpr int GRID_X = (\d+);", src).group(1)) == R.GRID_X


# ------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------------
def test_event_scorer_argument_errors():
    ES = scoring.EventScorer
    ok = ES(num_classes=4, planes=3, bins=10, radius=2, interface_from=1, fill_label=255, capacity=64, device="cuda")
    assert ok.edges == R.equal_edges(10) and ok.bins == 10 and ok.words == R.words(3, 4, 10) and ok.events == 0
    assert ES(bins=[0.5, 0.9]).edges == [0x3800, _HALF(0.9)] and ES(bins=1).edges == [] and ES(bins=[]).bins == 1
    assert len(ES(bins=32).edges) == 31
    for kw, msg in ((dict(num_classes=0), "num_classes must be 1..16"), (dict(num_classes=17), "num_classes must be 1..16"),
                    (dict(num_classes=4.0), "num_classes must be an int"), (dict(planes=0), "planes must be"),
                    (dict(bins=0), "bins must be 1..32"), (dict(bins=33), "bins must be 1..32"), (dict(bins=True), "bins must be"),
                    (dict(bins=[0.5, 0.5]), "strictly ascending"), (dict(bins=[0.5, 0.25]), "strictly ascending"),
                    (dict(bins=[0.5, 0.50001]), "strictly ascending"), (dict(bins=[0.0, 0.5]), "positive and finite"),
                    (dict(bins=[-0.5]), "positive and finite"), (dict(bins=[float("inf")]), "positive and finite"),
                    (dict(bins=[float("nan")]), "positive and finite"), (dict(bins=[1e-9]), "not a positive finite half"),
                    (dict(bins=[1e6]), "not a positive finite half"), (dict(bins=[0.01 * i for i in range(1, 33)]), "more than 32 bins"),
                    (dict(bins="ten"), "bins must be"), (dict(radius=9), "radius must be 0..8"), (dict(radius=-1), "radius must be 0..8"),
                    (dict(interface_from=5), "interface_from must be 0..4"), (dict(interface_from=-1), "interface_from must be"),
                    (dict(fill_label=256), "fill_label must be 0..255"), (dict(capacity=0), "capacity must be"),
                    (dict(radius=True), "radius must be an int")):
        with pytest.raises(ValueError, match=msg):
            ES(**kw)
    with pytest.raises(ValueError, match="duplicate edges"):
        scoring.equal_width_edges(4096)
    # add(): everything but the launch is checked on the host
    lab, cf, tr = torch.zeros((3, 8, 8), dtype=torch.uint8), torch.zeros((3, 8, 8), dtype=torch.float16), torch.zeros((3, 8, 8), dtype=torch.int64)
    for products, truth, msg in (((lab, cf), tr, "one CUDA device"), ((lab.int(), cf), tr, "label must be uint8"),
                                 ((lab, cf.float()), tr, "confidence float16"), ((lab, cf), tr.int(), "truth must be uint8 or int64"),
                                 ((lab[:2], cf[:2]), tr[:2], r"label must be \[3, rows, cols\]"), ((lab, cf[:, :4]), tr, "differ in shape"),
                                 ((lab, cf), tr[:, :, :4], "differ in shape"), (lab, tr, "label must be uint8"),
                                 (None, tr, "products must be"), ((lab, cf), None, "truth must be a tensor")):
        with pytest.raises(ValueError, match=msg):
            ok.add(products, truth)
    assert ok.events == 0 and ok._table is None
    empty = ok.read()
    assert empty.events == 0 and empty.tallies() == dict(scored=0, ignored=0, dark=0, nonfinite=0) and np.isnan(empty.ece())
    ok.reset()
