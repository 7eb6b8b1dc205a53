"""Overlap-tile inference without a GPU: margin_tiling against regular_tiling, the margin guarantee and the partition of the keep
windows; the blend weights of ubresnet_amd/_blend.py against tests/blend_ref.py and their sums; libubresnet_blend.so's header is
C99, header, binding, reference and library agree on entry points and geometry, the compiled kernels are exactly those the GPU
module's case table runs, every argument refusal returns UBV_EINVAL with a message before any launch; the third build table
and the entry point; the refusals of WholeViewSegmenter that need no device.  (No rule of the library lives in a header of
csrc/ that host code could run: the weights are Python, the kernel is device code, so there is no stand-alone host program.)"""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import blend_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ubresnet_amd")
HEADER = os.path.join(REPO, "include", "ubresnet_blend.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
import cpu_helpers as H  # noqa: E402
from ubresnet_amd import _blend as V  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd import deploy  # noqa: E402

LIB = B.ADDONS["blend"].out
U = 2.0 ** -24

# rows x cols, tile: the event, a view one tile covers, one axis covered by one tile, odd sizes, the small views of the GPU tests
SIZES = [((1008, 3456), (512, 832)), ((512, 832), (512, 832)), ((300, 500), (512, 832)), ((512, 3456), (512, 832)),
         ((1009, 3457), (512, 832)), ((96, 160), (64, 96)), ((80, 144), (64, 96)), ((2048, 2048), (256, 256)), ((65, 97), (64, 96))]


# ------------------------------------------------------------------------------------------------------------------------
# tiling
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,tile", SIZES)
def test_margin_zero_is_the_regular_tiling(size, tile):
    assert deploy.margin_tiling(*size, *tile, 0) == deploy.regular_tiling(*size, *tile) == tuple(R.margin_tiling(*size, *tile, 0))
    assert deploy.view_tiles(*size, 3, *tile, False, 0) == deploy.view_tiles(*size, 3, *tile, False)
    if size == (1008, 3456):
        assert deploy.margin_tiling(*size, *tile, 0) == ([0, 496], [0, 656, 1312, 1968, 2624])


@pytest.mark.parametrize("size,tile", SIZES)
def test_margin_guarantee_and_partition(size, tile):
    for margin in (0, 8, 64, min(tile) // 4):
        if 4 * margin > min(tile):
            continue
        origins = deploy.margin_tiling(*size, *tile, margin)
        assert origins == tuple(R.margin_tiling(*size, *tile, margin))
        for o, t, n in zip(origins, tile, size):
            assert o[0] == 0 and (o[-1] == n - t if n > t else o == [0]) and o == sorted(set(o))
            assert all(b - a <= t - 2 * margin for a, b in zip(o, o[1:])), "an overlap below 2 * margin"
            keep = deploy._keep_windows(o, t, n)
            assert keep == R.keep_windows(o, t, n)
            assert keep[0][0] == 0 and keep[-1][1] == n and all(a[1] == b[0] for a, b in zip(keep, keep[1:])), "not a partition"
            for oi, (lo, hi) in zip(o, keep):
                assert lo < hi and oi <= lo and hi <= oi + t
                assert oi == 0 or lo - oi >= margin, "a kept pixel within margin of the tile's low edge"
                assert oi + t >= n or oi + t - hi >= margin, "a kept pixel within margin of the tile's high edge"
    with pytest.raises(ValueError, match="margin"):
        deploy.margin_tiling(*size, *tile, min(tile) // 4 + 1)
    with pytest.raises(ValueError, match="margin"):
        deploy.margin_tiling(*size, *tile, -1)


def test_the_event_with_margin_64():
    ro, co = deploy.margin_tiling(1008, 3456, 512, 832, 64)
    assert ro == [0, 248, 496] and co == [0, 656, 1312, 1968, 2624]
    assert len(deploy.view_tiles(1008, 3456, 3, 512, 832, False, 64)) == 45 and len(deploy.view_tiles(1008, 3456, 3, 512, 832, False)) == 30


# ------------------------------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("size,tile", SIZES)
def test_weights(size, tile, kind):
    for margin in (0, 8, min(tile) // 4):
        origins = R.margin_tiling(*size, *tile, margin)
        axes = []
        for o, t, n in zip(origins, tile, size):
            w = R.axis_weights(o, t, n, margin, kind)
            lw = np.array(V.axis_log_weights(o, t, n, margin, kind))                   # the package's, in float64
            with np.errstate(divide="ignore"):
                assert np.allclose(lw, np.log(w), rtol=1e-14, atol=1e-15), "the package's weights are not the reference's"
            tab = R.log_table(w)
            total, total32, covering = np.zeros(n), np.zeros(n), np.zeros(n, int)
            for i, oi in enumerate(o):
                m = min(t, n - oi)
                total[oi:oi + m] += w[i, :m]
                total32[oi:oi + m] += np.exp(tab[i, :m].astype(np.float64))
                covering[oi:oi + m] += w[i, :m] > 0
                u = np.arange(m)
                d = np.minimum(u if oi > 0 else np.inf, t - 1 - u if oi + t < n else np.inf)
                assert (w[i, :m][d < margin] == 0).all() and np.isneginf(tab[i, :m][d < margin]).all(), "weight inside the margin"
                assert (w[i, :m][d >= margin] > 0).all()
                lo, hi = R.keep_windows(o, t, n)[i]
                assert (w[i, lo - oi:hi - oi] > 0).all() and np.isfinite(lw[i, lo - oi:hi - oi]).all(), "the keeping tile has no weight"
                assert (lw[i][np.isneginf(tab[i])] == -np.inf).all() and (lw[i][oi + np.arange(t) >= n] == 0).all()
            assert np.abs(total - 1.0).max() <= 4 * 2.0 ** -53, "float64 weights do not sum to one"
            assert np.abs(total32 - 1.0).max() <= 4 * U, "the fp32 log-weights do not sum to one within 4u"
            assert (covering >= 1).all()
            for i, oi in enumerate(o):                                                  # one tile alone: exactly +0
                m = min(t, n - oi)
                alone = (covering[oi:oi + m] == 1) & (w[i, :m] > 0)
                assert (tab[i, :m][alone].view(np.uint32) == 0).all() and (np.array(lw[i][:m])[alone] == 0).all()
                assert not np.signbit(np.array(lw[i][:m])[alone]).any()
            axes.append((o, w, tab))
        # separable: the 2-D weights of the tiles covering a pixel sum to one, also from the fp32 tables
        (ro, wr, tr), (co, wc, tc) = axes
        s2, s2f = np.zeros(size), np.zeros(size)
        for i, r0 in enumerate(ro):
            for j, c0 in enumerate(co):
                hh, ww = min(tile[0], size[0] - r0), min(tile[1], size[1] - c0)
                s2[r0:r0 + hh, c0:c0 + ww] += wr[i, :hh, None] * wc[j, None, :ww]
                with np.errstate(invalid="ignore"):
                    s2f[r0:r0 + hh, c0:c0 + ww] += np.exp((tr[i, :hh, None] + tc[j, None, :ww]).astype(np.float64))
        assert np.abs(s2 - 1.0).max() <= 8 * 2.0 ** -53 and np.abs(s2f - 1.0).max() <= 8 * U


def test_weight_refusals_and_kinds():
    assert V.KINDS == R.KINDS == ("linear", "hann") and V.check_kind(None) is None and V.check_kind("hann") == "hann"
    for bad in ("cosine", "", 1, ("linear",), True):
        with pytest.raises(ValueError, match="blend must be None or one of"):
            V.check_kind(bad)
    with pytest.raises(ValueError, match="has no weight"):
        V.axis_log_weights([0, 60], 64, 124, 8, "linear")                              # an overlap of 4 below 2 * margin
    g = V.axis_gains([0, 32], 64, 96, 8, "linear")
    assert g[0][:33] == [1.0] * 33 and g[0][33] == 23 / 24 and g[0][56:] == [0.0] * 8 and g[0][55] == 1 / 24 and g[1][8] == 1 / 24 and g[1][7] == 0.0
    h = V.axis_gains([0, 32], 64, 96, 8, "hann")
    assert abs(h[0][55] - np.sin(np.pi / 48) ** 2) < 1e-17 and h[0][0] == 1.0 and h[1][63] == 1.0 and h[0][56] == 0.0


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_blend.h"\n'
                     'int main(void) {\n'
                     '  int (*b)(float*, int64_t, void*) = ubv_blend_begin;\n'
                     '  int (*t)(const float*, int, int, int, const int32_t*, int, const float*, const float*, float*, int, int, int,\n'
                     '           void*) = ubv_blend_tiles;\n'
                     '  const char* (*e)(void) = ubv_last_error;\n'
                     '  int (*v)(void) = ubv_version;\n'
                     '  return b == 0 || t == 0 || e == 0 || v == 0 || UBV_OK != 0 || UBV_EINVAL != -1 || UBV_ELAUNCH != -2\n'
                     '         || UBV_MAX_TILES != 64 || UBV_MAX_CLASSES != 16 || UBV_BLOCK != 256 || UBV_MAX_GRID < 1;\n}\n')
    r = subprocess.run([H.cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(ubv_[a-z_0-9]+)\s*\(", text)
    assert declared == V.SYMBOLS == ["ubv_blend_begin", "ubv_blend_tiles", "ubv_last_error", "ubv_version"]
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBV_(BLOCK|MAX_GRID|MAX_TILES|MAX_CLASSES)\s+(\d+)", text)}
    assert geometry == dict(BLOCK=V.BLOCK, MAX_GRID=V.MAX_GRID, MAX_TILES=V.MAX_TILES, MAX_CLASSES=V.MAX_CLASSES)
    assert geometry == dict(BLOCK=R.BLOCK, MAX_GRID=R.MAX_GRID, MAX_TILES=R.MAX_TILES, MAX_CLASSES=R.MAX_CLASSES)
    for phrase in ("lae(a, b)", "log1pf(expf(lo - hi))", "(float)M_LN2", "contracted", "subnormals kept", "payload", "gather-form",
                   "ascending descriptor order", "no\n * atomic", "fl(x + fl(lwr + lwc))"):
        assert phrase in raw, phrase
    # lae is the rule written in ubresnet_tta.h, word for word
    rule = re.search(r"lae\(a, b\):.*?subnormals kept\.", raw, flags=re.S).group(0)
    assert rule in open(os.path.join(REPO, "include", "ubresnet_tta.h")).read()
    H.need_lib(LIB)
    assert V.lib().ubv_version() == V.BINDING.version() == 1


def test_library_stands_alone_and_exports_exactly_its_bindings_symbols():
    bd = V.BINDING
    assert bd.prefix == "ubv" and bd.path == LIB and os.path.basename(LIB) == "libubresnet_blend.so" and os.path.dirname(LIB) == PKG
    assert bd.symbols[-2:] == ["ubv_last_error", "ubv_version"]
    assert (V.LIB_PATH, V.SYMBOLS, V.lib, V.check) == (bd.path, bd.symbols, bd.lib, bd.check)
    H.need_lib(LIB)
    assert "libubresnet_" not in H.readelf("-d", LIB).replace("libubresnet_blend", "")
    assert sorted(n for n in H.defined_symbols(LIB) if re.match(r"ub[a-z]_", n)) == sorted(bd.symbols)
    others = [importlib.import_module("ubresnet_amd." + lib.binding).BINDING.prefix for lib in list(B.LIBS.values()) + list(B.EXTRAS.values())]
    assert "ubv" not in others
    tree = open(os.path.join(PKG, "_blend.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy)", tree, flags=re.M) and "from ._binding import Binding" in tree
    src = open(os.path.join(B.CSRC, B.ADDONS["blend"].sources[0])).read()
    assert '#include "../ubr_sat.h"' in src and "atomic" not in src.lower()


def test_a_missing_library_is_a_runtime_error(monkeypatch):
    import importlib.util
    nowhere = os.path.join(REPO, "no_such_dir", "libubresnet_blend.so")
    monkeypatch.setenv("UBV_LIB", nowhere)
    spec = importlib.util.spec_from_file_location("ubresnet_amd._blend_missing", os.path.join(PKG, "_blend.py"))
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert fresh.LIB_PATH == nowhere
    with pytest.raises(RuntimeError, match="is missing; build it with") as e:
        fresh.blend_begin(0x1000, 4)
    assert nowhere in str(e.value) and "There is no CPU fallback" in str(e.value)


def test_the_compiled_kernels_are_the_case_table():
    """no allow-list: every compiled kernel is launched by a case of test_gpu_blend_exact.py, and the table names nothing else"""
    H.need_lib(LIB)
    compiled = kernel_symbols.kernels(LIB)
    assert compiled == sorted(R.KERNEL_CASES), (compiled, sorted(R.KERNEL_CASES))
    assert all(R.KERNEL_CASES.values())
    ran = H.case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_blend_exact.py"))
    assert ran == set(R.CASES) == set(i for v in R.KERNEL_CASES.values() for i in v)
    for k, ids in R.KERNEL_CASES.items():
        assert set(ids) & ran, k


def test_the_cases_cover_the_paths_of_the_launch():
    assert [R.vector_path(n) for n in R.CASES] == [False, False, False, True, True, True, False, False, True]
    assert R.CASES["offset-C3"]["offset"] == 1 and R.CASES["offset-C3"]["tile"][1] % 4 == 0
    assert any(c0 % 4 for _, _, c0 in R.CASES["odd-origin-C3"]["calls"][0]) and R.CASES["odd-origin-C3"]["offset"] == 0
    assert sorted(set(c["C"] for c in R.CASES.values())) == [1, 3, 16]
    assert set(c["tile"] for n, c in R.CASES.items() if n != "second-trip") == {(5, 7), (8, 12)}
    for name, c in R.CASES.items():
        P, rows, cols = c["view"]
        calls = R.case_inputs(name)
        ref, lim, count = R.blend(np.full((P, c["C"], rows, cols), -np.inf, np.float32), calls)
        want = {0, 1, 2} if name == "second-trip" else {0, 1, 2, 4}
        assert want <= set(count.ravel().tolist()), name                                # pixels under no, one, two and four tiles
        th, tw = c["tile"]
        assert any(r0 + th > rows or c0 + tw > cols for call in c["calls"] for _, r0, c0 in call) or name == "second-trip", "no tile hangs over"
        assert all(0 <= r0 < rows and 0 <= c0 < cols and 0 <= p < P for call in c["calls"] for p, r0, c0 in call)
        covered = np.broadcast_to(count[:, None] > 0, ref.shape)
        assert np.isneginf(ref[~covered]).all() and not np.isnan(ref).any()
        assert np.isfinite(ref[covered]).mean() > 0.9 and (lim >= 0).all() and (lim[covered & np.isfinite(ref)] > 0).mean() > 0.9
        if len(c["calls"]) == 2:                                                        # overlaps inside a call and across the two
            one = [R.blend(np.full((P, c["C"], rows, cols), -np.inf, np.float32), [k])[2] for k in calls]
            assert (one[0] >= 2).any() and (one[1] >= 2).any() and ((one[0] >= 1) & (one[1] >= 1)).any()
        with np.errstate(invalid="ignore"):
            far = [np.abs(k[0][a].astype(np.float64) - k[0][b].astype(np.float64)).max() for k in calls for a in range(1) for b in range(1, len(k[1]))]
        assert max(far) > 90, name + ": no operands 100 nat apart"
    big = R.CASES["second-trip"]
    assert big["tile"] == (1, V.MAX_GRID * V.BLOCK * 2 + 8) and R.vector_path("second-trip") and R.begin_vector_path("second-trip")
    for nunits in (R.units("second-trip", 0), R.begin_units("second-trip")):
        trips = -(-nunits // R.BLOCK)
        assert R.grid(nunits) == V.MAX_GRID and V.MAX_GRID < trips < 2 * V.MAX_GRID and nunits % R.BLOCK != 0, "a second, partial trip"
    assert all(R.grid(R.units(n, k)) < V.MAX_GRID for n in R.CASES if n != "second-trip" for k in range(len(R.CASES[n]["calls"])))


def test_reference_blend_by_hand():
    """one row, two tiles of three pixels overlapping in one: weights 1/4 and 3/4 there"""
    lp = np.log(np.array([[[[0.5, 0.25, 0.125]]], [[[0.5, 0.5, 0.5]]]])).astype(np.float32)            # [2, 1, 1, 3]
    lwr = np.zeros((2, 1), np.float32)
    lwc = np.array([[0.0, 0.0, np.log(0.25)], [np.log(0.75), 0.0, -np.inf]], np.float32)
    ref, lim, count = R.blend(np.full((1, 1, 1, 6), -np.inf, np.float32), [(lp, [(0, 0, 0), (0, 0, 2)], lwr, lwc)])
    assert count.tolist() == [[[1, 1, 2, 1, 1, 0]]]
    want = [0.5, 0.25, 0.25 * 0.125 + 0.75 * 0.5, 0.5, 0.0]
    assert np.allclose(np.exp(ref[0, 0, 0, :5]), want, rtol=1e-7, atol=0) and ref[0, 0, 0, 5] == -np.inf and ref[0, 0, 0, 4] == -np.inf
    assert lim[0, 0, 0, 5] == 0 and lim[0, 0, 0, 4] == 0 and 0 < lim[0, 0, 0, 2] < 1e-6
    assert np.array_equal(R.operand32(lp[0], lwr[0], lwc[0])[0, 0, :2].view(np.uint32), lp[0, 0, 0, :2].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------------------------------
# addresses that are never dereferenced: every call below is refused on the host, before any launch
_P = 0x100000
_GOOD = dict(logp=_P, C=3, th=4, tw=8, desc=[0, 0, 0, 1, 2, 4], n=2, lwr=_P + 0x10000, lwc=_P + 0x20000, out=_P + 0x30000, P=2, rows=6, cols=12)
_BAD = {
    "null logp": (dict(logp=None), "null pointer"),
    "null lw_rows": (dict(lwr=None), "null pointer"),
    "null lw_cols": (dict(lwc=None), "null pointer"),
    "null out": (dict(out=None), "null pointer"),
    "null desc": (dict(desc=None), "desc_host is null"),
    "n 0": (dict(n=0), "n=0 must be 1..64"),
    "n 65": (dict(n=65), "n=65 must be 1..64"),
    "n negative": (dict(n=-1), "n=-1 must be 1..64"),
    "C 0": (dict(C=0), "C=0 must be 1..16"),
    "C 17": (dict(C=17), "C=17 must be 1..16"),
    "th 0": (dict(th=0), "must be positive"),
    "tw negative": (dict(tw=-8), "must be positive"),
    "tile too large": (dict(th=1 << 13, tw=(1 << 11) + 1), "exceeds 2^24 pixels"),
    "P 0": (dict(P=0), "must be positive"),
    "rows 0": (dict(rows=0), "must be positive"),
    "cols negative": (dict(cols=-12), "must be positive"),
    "view too large": (dict(P=1 << 20, rows=1 << 20, cols=1 << 20), "exceeds 2^40 elements"),
    "plane negative": (dict(desc=[-1, 0, 0, 1, 2, 4]), "tile 0: plane=-1"),
    "plane P": (dict(desc=[0, 0, 0, 2, 2, 4]), "tile 1: plane=2"),
    "row0 negative": (dict(desc=[0, -1, 0, 1, 2, 4]), "tile 0: origin (-1, 0) is outside"),
    "row0 at rows": (dict(desc=[0, 0, 0, 1, 6, 4]), "tile 1: origin (6, 4) is outside"),
    "col0 at cols": (dict(desc=[0, 0, 12, 1, 2, 4]), "tile 0: origin (0, 12) is outside"),
    "col0 negative": (dict(desc=[0, 0, 0, 1, 2, -4]), "tile 1: origin (2, -4) is outside"),
    "logp alignment": (dict(logp=_P + 2), "4-byte aligned"),
    "out alignment": (dict(out=_P + 0x30001), "4-byte aligned"),
    "out is logp": (dict(out=_P), "logp overlaps out"),
    "out inside logp": (dict(out=_P + 4 * 2 * 3 * 4 * 8 - 4), "logp overlaps out"),
    "lw_rows inside out": (dict(lwr=_P + 0x30000 + 4 * 2 * 3 * 6 * 12 - 4), "lw_rows overlaps out"),
    "lw_cols is out": (dict(lwc=_P + 0x30000), "lw_cols overlaps out"),
}
_BAD_BEGIN = {
    "null out": ((None, 16), "null pointer"),
    "nelem 0": ((_P, 0), "nelem=0 must be in 1..2^40"),
    "nelem negative": ((_P, -4), "nelem=-4 must be in 1..2^40"),
    "nelem too large": ((_P, (1 << 40) + 1), "must be in 1..2^40"),
    "alignment": ((_P + 1, 16), "4-byte aligned"),
}


@pytest.mark.parametrize("name", sorted(_BAD))
def test_blend_tiles_refusals_precede_any_launch(name):
    H.need_lib(LIB)
    change, message = _BAD[name]
    a = dict(_GOOD)
    a.update(change)
    desc = None if a["desc"] is None else (C.c_int32 * len(a["desc"]))(*a["desc"])
    lib = V.lib()
    rc = lib.ubv_blend_tiles(a["logp"], a["C"], a["th"], a["tw"], desc, a["n"], a["lwr"], a["lwc"], a["out"], a["P"], a["rows"], a["cols"], None)
    msg = lib.ubv_last_error().decode()
    assert rc == -1 and msg.startswith("ubv_blend_tiles:") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match="ubv_blend_tiles"):
        V.check(rc, name)


@pytest.mark.parametrize("name", sorted(_BAD_BEGIN))
def test_blend_begin_refusals_precede_any_launch(name):
    H.need_lib(LIB)
    (out, nelem), message = _BAD_BEGIN[name]
    lib = V.lib()
    rc = lib.ubv_blend_begin(out, nelem, None)
    msg = lib.ubv_last_error().decode()
    assert rc == -1 and msg.startswith("ubv_blend_begin:") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match="ubv_blend_begin"):
        V.blend_begin(out, nelem)


def test_desc3_takes_the_first_three_fields():
    d = V.desc3([(2, 5, 7, 0, 64, 0, 96), (0, 1, 3)])
    assert list(d) == [2, 5, 7, 0, 1, 3] and isinstance(d, C.Array) and d._type_ is C.c_int32


# ------------------------------------------------------------------------------------------------------------------------
# the third build table and the entry point
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


def test_the_addons_table():
    assert "blend" in B.ADDONS and not set(B.ADDONS) & set(B.LIBS) and not set(B.ADDONS) & set(B.EXTRAS)
    lib = B.ADDONS["blend"]
    assert isinstance(lib, B.Lib) and lib.sources == [os.path.join("extra", "ubr_blend.hip")] and lib.binding == "_blend"
    assert os.path.exists(os.path.join(B.CSRC, lib.sources[0])) and os.path.exists(os.path.join(PKG, "_blend.py"))
    outs = [l.out for t in (B.LIBS, B.EXTRAS, B.ADDONS) for l in t.values()]
    srcs = [s for t in (B.LIBS, B.EXTRAS, B.ADDONS) for l in t.values() for s in l.sources]
    assert len(outs) == len(set(outs)) and len(srcs) == len(set(srcs))
    for name, entry in B.ADDONS.items():
        listed = [os.path.realpath(os.path.join(B.CSRC, h)) for h in entry.headers]
        assert len(listed) == len(set(listed)) and set(listed) == _include_closure([os.path.join(B.CSRC, s) for s in entry.sources]), name
        assert not set(B.SOURCES + B.HEADERS) & set(entry.sources + entry.headers), "source_hash() covers the network's library only"
    assert os.path.realpath(HEADER) in [os.path.realpath(os.path.join(B.CSRC, h)) for h in lib.headers]
    every = sorted(os.path.join("extra", f) for f in os.listdir(os.path.join(B.CSRC, "extra")) if f.endswith(".hip"))
    assert every == sorted(s for t in (B.EXTRAS, B.ADDONS) for l in t.values() for s in l.sources), "a .hip under csrc/extra/ that no table builds"


def test_a_forced_build_of_blend_is_one_compile_and_one_link(monkeypatch, capsys):
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    capsys.readouterr()
    built = B.build_addons(force=True, only=["blend"])
    monkeypatch.undo()
    lib = B.ADDONS["blend"]
    src, obj = os.path.join(B.CSRC, lib.sources[0]), os.path.join(B.CSRC, "extra", "ubr_blend.o")
    assert built == [lib.out] and len(lines) == 2
    assert lines[0] == [B.HIPCC] + B.FLAGS + ["-c", src, "-o", obj]
    assert lines[1] == [B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib.out, obj]
    io = capsys.readouterr()
    assert io.out == "" and io.err.strip().split("\n") == [" ".join(c) for c in lines]        # the echo goes to stderr
    with pytest.raises(ValueError, match="no library named"):
        B.build_addons(only=["score"])


def test_the_command_line_builds_the_addons_between_the_table_and_the_extras(monkeypatch, capsys):
    import runpy
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    monkeypatch.setattr("sys.argv", ["build.py", "--force", "--addons", "--extras"])
    capsys.readouterr()
    runpy.run_module("ubresnet_amd.build", run_name="__main__")
    monkeypatch.undo()
    io = capsys.readouterr()
    paths = io.out.strip().split("\n")[33:]
    assert paths == [l.out for t in (B.LIBS, B.ADDONS, B.EXTRAS) for l in t.values()]
    links = [c[c.index("-o") + 1] for c in lines if "-shared" in c]
    assert links == paths
    err = io.err.strip().split("\n")
    assert all(" ".join(c) in err for c in lines[33:]), "the addons' and extras' echo goes to stderr"


def test_entry_point_reports_blend_on_stderr_before_the_score_line(monkeypatch, capsys):
    import __graft_entry__ as entry
    for lib in [l for t in (B.LIBS, B.ADDONS, B.EXTRAS) for l in t.values()]:
        H.need_lib(lib.out)
    calls = []
    monkeypatch.setattr(B, "build", lambda *a, **kw: calls.append(("build", a, kw)))
    monkeypatch.setattr(B, "build_addons", lambda *a, **kw: calls.append(("addons", a, kw)))
    monkeypatch.setattr(B, "build_extras", lambda *a, **kw: calls.append(("extras", a, kw)))
    capsys.readouterr()
    entry.build()
    io = capsys.readouterr()
    assert [c[0] for c in calls] == ["build", "addons", "extras"] and not calls[1][1] and not calls[1][2].get("only")
    out = io.out.strip().split("\n")
    assert len(out) == 14 and all(l.startswith("built ") for l in out) and "blend" not in io.out
    err = io.err.strip().split("\n")
    assert "built %s ABI version 1" % LIB in err
    assert err[-1] == "built %s ABI version 1" % B.EXTRAS["score"].out and err.index("built %s ABI version 1" % LIB) < len(err) - 1


def test_entry_point_refuses_a_blend_library_that_lacks_a_symbol(monkeypatch):
    import __graft_entry__ as entry
    H.need_lib(LIB)
    for f in ("build", "build_addons", "build_extras"):
        monkeypatch.setattr(B, f, lambda *a, **kw: None)
    monkeypatch.setitem(V.BINDING.table, "ubv_no_such_call", (C.c_int, []))
    monkeypatch.setattr(V.BINDING, "_lib", None)
    with pytest.raises(RuntimeError, match="lacks symbols") as e:
        entry.build()
    assert "libubresnet_blend.so" in str(e.value) and "ubv_no_such_call" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------------
class _Conv:
    in_channels, out_channels = 1, 3


class _Model:
    conv1 = conv11 = _Conv()

    def eval(self):
        raise AssertionError("the arguments are checked before the model is touched")


def test_segmenter_refusals_and_defaults_without_a_device():
    kw = dict(planes=3, tile=(64, 96), batch=4)
    for bad in ("cosine", 1, ("linear",)):
        with pytest.raises(ValueError, match="blend must be None or one of"):
            deploy.WholeViewSegmenter(_Model(), 96, 160, blend=bad, **kw)
    for bad in (17, -1, 1.5, True, "8"):
        with pytest.raises(ValueError, match="margin must be an int"):
            deploy.WholeViewSegmenter(_Model(), 96, 160, margin=bad, **kw)
        with pytest.raises(ValueError, match="margin must be an int"):
            deploy.WholeViewSegmenter(_Model(), 96, 160, margin=bad, blend="linear", **kw)
    sig = inspect.signature(deploy.WholeViewSegmenter.__init__).parameters
    assert sig["margin"].default == 0 and sig["blend"].default is None
    assert inspect.signature(deploy.view_tiles).parameters["margin"].default == 0
    base = deploy.WholeViewSegmenter(_Model(), 96, 160, **kw)
    same = deploy.WholeViewSegmenter(_Model(), 96, 160, margin=0, blend=None, **kw)
    assert same.tiles == base.tiles and same.blend is None and same._blend_lw is None and same._blend_out is None
    dense = deploy.WholeViewSegmenter(_Model(), 112, 176, margin=16, **kw)
    assert dense.tiles_per_event == 3 * 3 * 3 and deploy.WholeViewSegmenter(_Model(), 112, 176, **kw).tiles_per_event == 3 * 2 * 2
    assert dense.tiles == deploy.view_tiles(112, 176, 3, 64, 96, False, 16) and dense.blend is None and dense.margin == 16
    on = deploy.WholeViewSegmenter(_Model(), 96, 160, margin=8, blend="hann", output="products", **kw)
    lr, lc = on._blend_host
    assert tuple(lr.shape) == (on.tiles_per_event, 64) and tuple(lc.shape) == (on.tiles_per_event, 96) and str(lr.dtype) == "torch.float64"
    ro, co = R.margin_tiling(96, 160, 64, 96, 8)
    tr, tc = R.view_tables(3, ro, co, 64, 96, 96, 160, 8, "hann")
    assert [t[:3] for t in on.tiles] == R.view_desc(3, ro, co)
    for mine, ref in ((lr, tr), (lc, tc)):
        got = mine.float().numpy()
        assert np.array_equal(np.isneginf(got), np.isneginf(ref)) and np.array_equal(got == 0, ref == 0)
        fin = np.isfinite(ref)
        assert np.abs(got[fin].astype(np.float64) - ref[fin]).max() <= 2.0 ** -23 * np.abs(ref[fin]).max()
    assert "dense" in deploy.WholeViewSegmenter.__doc__ and "blend" in deploy.WholeViewSegmenter.__doc__
