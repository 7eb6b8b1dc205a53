"""The test-time-augmentation library without a GPU: libubresnet_tta.so's header is C99; header, binding, reference and library agree
on the entry points and the geometry; the compiled kernels are exactly those the GPU module's case table runs; every argument
refusal returns UBT_EINVAL with a message before any launch; the numpy reference against numpy.logaddexp and torch.logsumexp, and
its edge rules; the refusals of WholeViewSegmenter and segment_crops that need no device."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import tta_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_tta.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib  # noqa: E402
from ubresnet_amd import _tta as T  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402

LIB = B.LIBS["tta"].out
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_tta.h"\n'
                     'int main(void) {\n'
                     '  int (*f)(const float*, float*, int64_t, int, int, int, void*) = ubt_flip_planes;\n'
                     '  int (*m)(const float*, float*, int64_t, int, int, int, int, int, float, void*) = ubt_merge_view;\n'
                     '  const char* (*e)(void) = ubt_last_error;\n'
                     '  int (*v)(void) = ubt_version;\n'
                     '  return f == 0 || m == 0 || e == 0 || v == 0 || UBT_OK != 0 || UBT_EINVAL != -1 || UBT_ELAUNCH != -2\n'
                     '         || UBT_MAX_VIEWS != 4 || UBT_FLIP_ROWS != 1 || UBT_FLIP_COLS != 2;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ubt_[a-z_0-9]+)\s*\(", text))
    need_lib(LIB)
    assert declared == set(T.SYMBOLS) and len(T.SYMBOLS) == len(set(T.SYMBOLS)) == 4
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBT_(BLOCK|UNROLL|MAX_GRID|MAX_VIEWS|FLIP_ROWS|FLIP_COLS)\s+(\d+)", text)}
    assert geometry == dict(BLOCK=T.BLOCK, UNROLL=T.UNROLL, MAX_GRID=T.MAX_GRID, MAX_VIEWS=T.MAX_VIEWS, FLIP_ROWS=T.FLIP_ROWS, FLIP_COLS=T.FLIP_COLS)
    assert geometry == dict(BLOCK=R.BLOCK, UNROLL=R.UNROLL, MAX_GRID=R.MAX_GRID, MAX_VIEWS=R.MAX_VIEWS, FLIP_ROWS=R.FLIP_ROWS, FLIP_COLS=R.FLIP_COLS)
    assert T.FLIPS == dict(rows=1, cols=2, both=3)
    # the arithmetic rules are stated in the header
    for phrase in ("32-bit patterns", "lae(a, b)", "log1pf(expf(lo - hi))", "(float)M_LN2", "symmetric", "contracted", "subnormals kept", "payload"):
        assert phrase in raw, phrase


def test_the_compiled_kernels_are_the_case_table():
    """no allow-list: every compiled instantiation is launched by a case of test_gpu_tta_exact.py, and the table names nothing else"""
    need_lib(LIB)
    compiled = kernel_symbols.kernels(LIB)
    assert compiled == sorted(R.KERNEL_CASES), (compiled, sorted(R.KERNEL_CASES))
    assert len(compiled) == 16                                       # flip in 0..3 x {scalar, vector} x {copy, merge}
    assert all(R.KERNEL_CASES[k] for k in compiled), [k for k in compiled if not R.KERNEL_CASES[k]]
    # the ids the table names are the ids the GPU module is parametrised with
    ids = set("flip[%s-%d]" % (n, f) for n in R.SHAPES for f in range(4))
    ids |= set("merge[%s-%d-%d]" % (n, K, first) for n in R.SHAPES for K, first in R.merge_cases(n))
    assert set(c for v in R.KERNEL_CASES.values() for c in v) == ids
    src = open(os.path.join(REPO, "tests", "test_gpu_tta_exact.py")).read()
    assert "R.SHAPES" in src and "R.merge_cases" in src and "R.view_flips" in src


def test_the_shapes_cover_the_paths_of_the_launch():
    assert [R.SHAPES[n]["shape"] for n in ("one", "odd", "vec8", "vec20", "misaligned")] == [(1, 1, 1), (3, 3, 7), (2, 5, 8), (6, 4, 20), (2, 32, 64)]
    assert [R.vector_path(n) for n in R.SHAPES] == [False, False, True, True, False, True]
    big = R.SHAPES["second-trip"]["shape"]
    assert big == (1, 3, T.MAX_GRID * T.BLOCK * 4 + 12)
    trips = -(-R.units("second-trip") // R.TRIP)
    assert R.grid(R.units("second-trip")) == T.MAX_GRID and T.MAX_GRID < trips < 2 * T.MAX_GRID, "a second, partial trip"
    assert R.units("second-trip") % R.TRIP != 0, "whose last workgroup is partly filled"
    assert all(R.grid(R.units(n)) == 1 for n in ("one", "odd", "vec8", "vec20")) and R.grid(R.units("misaligned")) == 8
    for K, first in R.MERGE_CASES:
        fl = R.view_flips(K, first)
        assert len(set(fl)) == K and fl[0] == first                                    # a different flip per view
    assert sorted(set(K for K, _ in R.MERGE_CASES)) == [1, 2, 3, 4] == sorted(K for K, _ in R.merge_cases("second-trip"))


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------------------------------
# addresses that are never dereferenced: every call below is refused on the host, before any launch.  2 x 4 x 8 floats (256 bytes)
_P = 0x100000
_A = dict(src=_P, dst=_P + 0x1000, nplanes=2, H=4, W=8, flip=3, k=1, K=2, log_k=float(f32(np.log(2.0))))
_PLANES = {
    "null src": (dict(src=None), "null pointer"),
    "null dst": (dict(dst=None), "null pointer"),
    "nplanes 0": (dict(nplanes=0), "must be positive"),
    "nplanes negative": (dict(nplanes=-1), "must be positive"),
    "H 0": (dict(H=0), "must be positive"),
    "H negative": (dict(H=-4), "must be positive"),
    "W 0": (dict(W=0), "must be positive"),
    "W negative": (dict(W=-8), "must be positive"),
    "too many elements": (dict(nplanes=1 << 40), "exceeds 2^40 elements"),
    "flip negative": (dict(flip=-1), "flip=-1 must be a mask"),
    "flip 4": (dict(flip=4), "flip=4 must be a mask"),
    "src alignment": (dict(src=_P + 2), "4-byte aligned"),
    "src is dst": (dict(dst=_P), "overlaps"),
    "dst starts inside src": (dict(dst=_P + 252), "overlaps"),
    "src starts inside dst": (dict(src=_P + 0x1000 + 252), "overlaps"),
}
_VIEWS = {
    "K 0": (dict(K=0, k=0), "K=0 must be in 1..4"),
    "K 5": (dict(K=5), "K=5 must be in 1..4"),
    "K negative": (dict(K=-2), "K=-2 must be in 1..4"),
    "k == K": (dict(k=2), "k=2 must be in 0..K-1"),
    "k > K": (dict(k=3, K=3), "k=3 must be in 0..K-1"),
    "k negative": (dict(k=-1), "k=-1 must be in 0..K-1"),
    "log_k NaN": (dict(log_k=float("nan")), "log_k"),
    "log_k inf": (dict(log_k=float("inf")), "log_k"),
    "log_k zero": (dict(log_k=0.0), "log_k"),
}
_BAD = {"%s: %s" % (w, k): (w, c, m) for w in ("flip", "merge") for k, (c, m) in _PLANES.items()}
_BAD.update({"merge: %s" % k: ("merge", c, m) for k, (c, m) in _VIEWS.items()})
_ENTRY = dict(flip="ubt_flip_planes", merge="ubt_merge_view")


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    which, change, message = _BAD[name]
    a = dict(_A)
    a.update(change)
    lib = T.lib()
    if which == "flip":
        rc = lib.ubt_flip_planes(a["src"], a["dst"], a["nplanes"], a["H"], a["W"], a["flip"], None)
    else:
        rc = lib.ubt_merge_view(a["src"], a["dst"], a["nplanes"], a["H"], a["W"], a["flip"], a["k"], a["K"], a["log_k"], None)
    msg = lib.ubt_last_error().decode()
    assert rc == -1 and msg.startswith(_ENTRY[which] + ":") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=_ENTRY[which]):
        T.check(rc, name)


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def test_reference_flip_by_hand():
    a = np.arange(2 * 2 * 3, dtype=np.int32).reshape(2, 2, 3)
    assert R.flip_planes(a, 0).tolist() == a.tolist()
    assert R.flip_planes(a, 1).tolist() == [[[3, 4, 5], [0, 1, 2]], [[9, 10, 11], [6, 7, 8]]]
    assert R.flip_planes(a, 2).tolist() == [[[2, 1, 0], [5, 4, 3]], [[8, 7, 6], [11, 10, 9]]]
    assert R.flip_planes(a, 3).tolist() == [[[5, 4, 3], [2, 1, 0]], [[11, 10, 9], [8, 7, 6]]]
    for f in range(4):
        assert R.flip_planes(R.flip_planes(a, f), f).tolist() == a.tolist()            # a flip is its own inverse


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_reference_merge_is_the_log_of_the_mean_probability(K):
    rs = np.random.RandomState(K)
    views = [R.logsoftmax_rows(rs, (6, 5, 13)) for _ in range(K)]
    flips = R.view_flips(K, 1)
    got, lim = R.merge(views, flips)
    un = np.stack([R.flip_planes(v, f).astype(np.float64) for v, f in zip(views, flips)])
    want = np.logaddexp.reduce(un, axis=0) - np.log(K)
    assert np.abs(got - want).max() <= 4 * 2.0 ** -53 * np.abs(want).max()
    tl = torch.logsumexp(torch.from_numpy(un), 0).numpy() - np.log(K)
    assert np.abs(got - tl).max() <= 4 * 2.0 ** -53 * np.abs(want).max()
    # rows of probabilities again: the classes of a pixel still sum to one
    assert np.abs(np.exp(got).reshape(2, 3, 5, 13).sum(1) - 1.0).max() < 1e-6
    if K == 1:
        assert not lim.any() and np.array_equal(got, views[0][:, ::-1, :].astype(np.float64))
    else:
        # the bound is a few ulps of the largest partial merge (none is below view 0), and some pixels are 100 nat apart
        assert (lim > 0).all() and (lim <= (4.0 * K + 4.0) * 1.03 * R.U32 * np.maximum(np.abs(un[0]) + np.log(K), 1.0)).all()
        assert (np.abs(un[0] - un[1]) > 90).any()


def test_reference_edge_rules():
    inf, nan = f32(np.inf), f32(np.nan)
    x = f32(-1.25)
    a = np.array([-inf, -inf, x, x, inf, x, nan, x, nan, inf, -inf, inf], dtype=f32)
    b = np.array([-inf, x, -inf, x, x, inf, x, nan, nan, inf, inf, -inf], dtype=f32)
    out, general = R.lae32(a, b)
    assert not general.any()
    xx = f32(x + R.LN2_F32)
    assert out[:6].view(np.uint32).tolist() == np.array([-inf, x, x, xx, inf, inf], dtype=f32).view(np.uint32).tolist()
    assert np.isnan(out[6:9]).all() and out[9] == inf and out[10] == inf and out[11] == inf
    o2, g2 = R.lae32(b, a)
    assert np.array_equal(out.view(np.uint32)[~np.isnan(out)], o2.view(np.uint32)[~np.isnan(o2)]) and not g2.any()   # symmetric
    assert R.lae32(f32(-1.0), f32(-2.0))[1].all()                                                                      # needs the library calls
    # the fp64 rules agree where both are defined
    with np.errstate(all="ignore"):
        o64 = R.lae64(a, b)
    assert o64[0] == -np.inf and o64[1] == x and o64[2] == x and abs(o64[3] - (x + np.log(2.0))) < 1e-15
    assert o64[4] == np.inf and o64[5] == np.inf and np.isnan(o64[6:9]).all() and (o64[9:] == np.inf).all()
    # and the merge of such views is finite wherever every input is, -inf where every view is
    views = [np.array([[[-inf, -inf, x, -200.0]]], dtype=f32), np.array([[[-inf, x, x, -0.0]]], dtype=f32)]
    got, lim = R.merge(views)
    assert got[0, 0, 0] == -np.inf and lim[0, 0, 0] == 0
    assert got[0, 0, 1] == x - np.log(2.0) and abs(got[0, 0, 2] - x) < 1e-15 and abs(got[0, 0, 3] + np.log(2.0)) < 1e-15
    assert float(R.log_views(2)) == float(f32(np.log(2.0))) and T.log_views(3) == np.log(3.0)


# ------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------------
def test_parse_views():
    assert T.parse_views(None) == () and T.parse_views(()) == () and T.parse_views([]) == ()
    assert T.parse_views(("cols",)) == (0, 2) and T.parse_views(("rows", "cols", "both")) == (0, 1, 2, 3)
    assert T.parse_views(["both", "rows"]) == (0, 3, 1)                                # the order given, the identity first
    for bad, msg in ((("cols", "cols"), "named twice"), (("diag",), "unknown view"), ("cols", "must be None or a tuple"),
                     ((2,), "unknown view"), (("identity",), "unknown view"), (3, "must be None or a tuple")):
        with pytest.raises(ValueError, match=msg):
            T.parse_views(bad)


def test_segmenters_reject_bad_tta_without_a_device():
    from ubresnet_amd import deploy

    class Conv:
        in_channels, out_channels = 1, 3

    class Model:
        conv1 = conv11 = Conv()

        def eval(self):
            raise AssertionError("the tta argument is checked before the model is touched")

    for bad, msg in ((("cols", "cols"), "named twice"), (("columns",), "unknown view"), ("rows", "must be None or a tuple")):
        with pytest.raises(ValueError, match=msg):
            deploy.WholeViewSegmenter(Model(), 80, 144, planes=3, tile=(64, 96), batch=4, tta=bad)
        with pytest.raises(ValueError, match=msg):
            deploy.segment_crops(Model(), torch.zeros(1, 1, 8, 8), tta=bad)
    for off in (None, ()):
        seg = deploy.WholeViewSegmenter(Model(), 80, 144, planes=3, tile=(64, 96), batch=4, tta=off)
        assert seg._flips == () and seg._tta_side is None and seg._tta_merged is None
    on = deploy.WholeViewSegmenter(Model(), 80, 144, planes=3, tile=(64, 96), batch=4, tta=("rows", "cols"))
    assert on._flips == (0, 1, 2) and on.tiles_per_event == 12
    assert inspect.signature(deploy.segment_crops).parameters["tta"].default is None
    assert inspect.signature(deploy.WholeViewSegmenter.__init__).parameters["tta"].default is None
