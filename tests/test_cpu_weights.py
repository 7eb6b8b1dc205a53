"""libubresnet_weight.so without a GPU: its header is C99, the header / binding / library agree on the entry points, the
kernels compiled into it are exactly the ones the case table of tests/test_gpu_weights_exact.py claims, the numpy reference
those GPU tests compare against follows the rule of include/ubresnet_weight.h on hand-worked examples, every argument refusal
returns its error before any launch, and PixelWeights / BatchStager refuse bad arguments before any library call."""
import ctypes as C
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import weights_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_weight.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib, case_ids_run_by_the_gpu_module  # noqa: E402
from ubresnet_amd import _weight  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd.pixel_weights import PixelWeights  # noqa: E402

LIB = B.LIBS["weight"].out
INF = float("inf")


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ubresnet_weight.h"\nint main(void) { int (*f)(const int64_t*, float*, int64_t*, int, int, int, int, float, int, float, int, void*) = ubw_pixel_weights; return f == 0 || UBW_MAX_CLASSES != 16 || UBW_OK != 0; }\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ubw_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_weight.SYMBOLS) and len(_weight.SYMBOLS) == len(set(_weight.SYMBOLS))
    tile = open(os.path.join(REPO, "ubresnet_amd", "csrc", "ubr_weight_tile.h")).read()       # the launch geometry is not in the ABI
    assert "UBW_TILE" not in text and "UBW_BLOCK" not in text
    consts = {k: int(v) for k, v in re.findall(r"#define\s+UBW_(MAX_CLASSES|MAX_RADIUS)\s+(\d+)", text)
              + re.findall(r"#define\s+UBW_(LANE_PIXELS|BLOCK|MAX_GRID|TILE_W|TILE_H)\s+(\d+)", tile)}
    assert consts == dict(MAX_CLASSES=_weight.MAX_CLASSES, MAX_RADIUS=_weight.MAX_RADIUS, LANE_PIXELS=_weight.LANE_PIXELS,
                          BLOCK=_weight.BLOCK, MAX_GRID=_weight.MAX_GRID, TILE_W=_weight.TILE_W, TILE_H=_weight.TILE_H)
    assert consts == dict(MAX_CLASSES=R.MAX_CLASSES, MAX_RADIUS=R.MAX_RADIUS, LANE_PIXELS=R.LANE_PIXELS, BLOCK=R.BLOCK,
                          MAX_GRID=R.MAX_GRID, TILE_W=R.TILE_W, TILE_H=R.TILE_H)
    need_lib(LIB)


def test_case_table_equals_the_compiled_kernels():
    need_lib(LIB)
    have = set(kernel_symbols.kernels(LIB))
    claimed = set(R.KERNEL_CASES)
    assert have - claimed == set(), "compiled kernels without a case in tests/test_gpu_weights_exact.py: %s" % sorted(have - claimed)
    assert claimed - have == set(), "cases for kernels that are not compiled: %s" % sorted(claimed - have)
    assert case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_weights_exact.py")) == set(i for ids in R.KERNEL_CASES.values() for i in ids)
    assert all(ids for ids in R.KERNEL_CASES.values())
    assert set(R.KERNEL_CASES) == {"count_kernel"} | {"apply_kernel<%d>" % r for r in range(R.MAX_RADIUS + 1)}
    assert set(R.KERNEL_CASES["count_kernel"]) == set(i for ids in R.KERNEL_CASES.values() for i in ids)     # every call counts


def test_geometry_shapes_cover_the_tile():
    shapes = R.GEOMETRY
    assert (1, 1, 1) in shapes
    assert any(h < R.MAX_RADIUS for _, h, _ in shapes) and any(w < R.MAX_RADIUS for _, _, w in shapes)
    assert any(w % R.LANE_PIXELS for _, _, w in shapes) and any(w % R.LANE_PIXELS == 0 for _, _, w in shapes)
    assert any(w > R.TILE_W and w % R.TILE_W and h > R.TILE_H and h % R.TILE_H for _, h, w in shapes)       # ragged, several tiles
    assert any(b > 1 and (h * w) % 2 for b, h, w in shapes)                                                 # image 1 starts unaligned


def test_a_missing_library_is_a_clear_error(tmp_path):
    code = "from ubresnet_amd import _weight\ntry:\n    _weight.lib()\nexcept RuntimeError as e:\n    print('ERR', e)\n"
    env = dict(os.environ, UBW_LIB=str(tmp_path / "nowhere" / "libubresnet_weight.so"), PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=REPO)
    assert r.returncode == 0 and "ERR" in r.stdout and "is missing" in r.stdout and "nowhere" in r.stdout, r.stdout + r.stderr
    assert "no CPU fallback" in r.stdout


# ------------------------------------------------------------------------------------------------------------------------
# the reference against the rule, by hand
# ------------------------------------------------------------------------------------------------------------------------
def test_reference_on_a_hand_worked_example():
    X = -100
    label = np.array([[[0, 0, 0, 0],
                       [0, 1, 2, 0],
                       [0, 1, X, 0],
                       [0, 0, 0, 2]]], np.int64)
    # n = (11, 2, 2), K = 3, V = 15: w = 15/33, 15/6, 15/6
    w0, w1 = np.float32(15.0 / 33.0), np.float32(2.5)
    w, counts = R.reference(label, 3, INF, 1, 3.0, 1)
    assert counts[0].tolist() == [11, 2, 2] + [0] * 13
    g = np.float32(7.5)                                       # 2.5 * 3
    want = np.array([[w0, w0, w0, w0],
                     [w0, g, g, w0],                          # (1,1) touches the 2 at (1,2); (1,2) touches both 1s
                     [w0, g, 0.0, w0],                        # (2,1) touches (1,2) diagonally; the invalid pixel weighs nothing
                     [w0, w0, w0, w1]], np.float32)           # (3,3): its only neighbours of interest are invalid or background
    assert np.array_equal(w[0].view(np.int32), want.view(np.int32))
    # lo = 0: background takes part, every pixel next to another class is marked
    w, _ = R.reference(label, 3, INF, 1, 3.0, 0)
    m = np.array([[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 0, 1], [1, 1, 1, 1]], bool)
    plain = np.where(label[0] == 0, w0, w1).astype(np.float32)
    plain[2, 2] = 0.0
    assert np.array_equal(w[0].view(np.int32), np.where(m, plain * np.float32(3.0), plain).astype(np.float32).view(np.int32))
    # a cap that binds classes 1 and 2 alone; r = 0 turns the gain off
    w, _ = R.reference(label, 3, 2.0, 0, 3.0, 1)
    assert sorted(set(w[0].reshape(-1).tolist())) == [0.0, float(w0), 2.0]


def test_reference_mean_is_one_without_a_cap():
    rs = np.random.RandomState(5)
    label = R.sprinkle_invalid(rs, R.noise(rs, 4, 13, 29, 5), 5)
    _, counts = R.reference(label, 5)
    for b in range(4):
        n = counts[b, :5].astype(np.float64)
        K, V = (n > 0).sum(), n.sum()
        present = n > 0
        total = sum(Fraction(int(V), int(K) * int(c)) * int(c) for c in n[present])          # the rule before any rounding
        assert total == int(V)
        wc = V / (K * n[present])                                                          # in float64, before the fp32 rounding
        assert abs((wc * n[present]).sum() / V - 1.0) <= 4 * np.finfo(np.float64).eps
    w, _ = R.reference(label, 5)
    valid = (label >= 0) & (label < 5)
    for b in range(4):
        assert abs(w[b][valid[b]].astype(np.float64).mean() - 1.0) < 1e-6


def test_reference_background_only_and_all_invalid():
    w, counts = R.reference(np.zeros((2, 3, 5), np.int64), 3, INF, 2, 4.0, 0)
    assert np.array_equal(w.view(np.int32), np.ones((2, 3, 5), np.float32).view(np.int32)) and counts[:, 0].tolist() == [15, 15]
    bad = np.resize(np.array(R.invalid_values(3), np.int64), 15).reshape(1, 3, 5)
    w, counts = R.reference(bad, 3, INF, 2, 4.0, 0)
    assert not w.view(np.int32).any() and not counts.any()                                  # all +0.0
    assert 2 ** 32 + 1 in R.invalid_values(3) and (2 ** 32 + 1) % 2 ** 32 == 1 and (2 ** 40 + 2) % 2 ** 32 == 2


def test_reference_marks_both_sides_and_stays_inside_rows_and_images():
    label = np.zeros((2, 4, 6), np.int64)
    label[0, 1, 2], label[0, 1, 3] = 1, 2
    w, _ = R.reference(label, 3, INF, 1, 2.0, 1)
    plain, _ = R.reference(label, 3)
    assert ((w != plain) == ((label == 1) | (label == 2))).all()                            # both sides, nothing else
    # the last pixel of a row against the first of the next; the last pixel of an image against the first of the next
    label = np.zeros((2, 4, 6), np.int64)
    label[0, 1, 5], label[0, 2, 0] = 1, 2
    label[0, 3, 5], label[1, 0, 0] = 1, 2
    for r in (1, 2, 3, 4):                                # five columns apart in the image, neighbours in memory
        w, _ = R.reference(label, 3, INF, r, 2.0, 1)
        assert np.array_equal(w.view(np.int32), R.reference(label, 3)[0].view(np.int32)), r
    label[0, 2, 1] = 2                                      # now (1,5) is 4 columns from a 2: r = 4 alone marks it
    for r in (3, 4):
        marked = R.reference(label, 3, INF, r, 2.0, 1)[0] != R.reference(label, 3)[0]
        assert marked[0, 1, 5] == (r == 4) and not marked[1].any()


# ------------------------------------------------------------------------------------------------------------------------
# the apply pass on the host
# ------------------------------------------------------------------------------------------------------------------------
def test_the_apply_phases_run_on_the_host_give_the_reference(tmp_path):
    """ubr_weight_tile.h is plain C++: tests/weights_tile_host.cpp runs its three phases lane by lane; every shape of the
    geometry table at every radius, element and 16-byte accesses, bit for bit"""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = "c++"
    so = str(tmp_path / "libtile.so")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "weights_tile_host.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    host = C.CDLL(so)
    host.host_apply.restype = C.c_int
    host.host_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_float, C.c_int, C.c_float, C.c_int, C.c_int]
    rs = np.random.RandomState(8)
    took_vectors = 0
    for shape in R.GEOMETRY + [(2, 20, 72)]:
        for Cn, lo in ((3, 1), (16, 0), (1, 1)):
            label = R.sprinkle_invalid(rs, R.blobs(rs, *shape, Cn) if Cn == 3 else R.noise(rs, *shape, Cn), Cn)
            for r_ in range(R.MAX_RADIUS + 1):
                for cap, gain in ((INF, 2.5), (3.0, 1.1)):
                    want, counts = R.reference(label, Cn, cap, r_, gain, lo)
                    for vector in (0, 1):
                        lab = np.ascontiguousarray(label)
                        got = np.full(label.shape, -7.0, np.float32)
                        took = host.host_apply(lab.ctypes.data, got.ctypes.data, counts.ctypes.data, *shape, Cn, cap, r_, gain, lo, vector)
                        took_vectors += took == 3
                        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (shape, Cn, lo, r_, cap, gain, vector)
    assert took_vectors > 0


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
# a pointer that is never dereferenced: every call below is refused on the host, before any launch
_P = 0x10000
_GOOD = dict(label=_P, weight=_P, counts=_P, B=2, H=8, W=16, C=3, max_weight=INF, r=1, gain=2.0, lo=1)
_BAD = {
    "B 0": dict(B=0),
    "H 0": dict(H=0),
    "W negative": dict(W=-3),
    "B*H*W 2^31": dict(B=2 ** 15, H=2 ** 8, W=2 ** 8),
    "H*W overflows int32": dict(H=2 ** 16, W=2 ** 16),
    "B*H*W overflows int64": dict(B=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1),
    "C 0": dict(C=0),
    "C 17": dict(C=17),
    "radius -1": dict(r=-1),
    "radius 5": dict(r=5),
    "lo -1": dict(lo=-1),
    "lo above C": dict(lo=4),
    "max_weight nan": dict(max_weight=float("nan")),
    "max_weight 0": dict(max_weight=0.0),
    "max_weight negative": dict(max_weight=-1.0),
    "max_weight -inf": dict(max_weight=-INF),
    "gain nan": dict(gain=float("nan")),
    "gain negative": dict(gain=-0.5),
    "gain inf": dict(gain=INF),
    "null label": dict(label=None),
    "null weight": dict(weight=None),
    "null counts": dict(counts=None),
    "label not 8-byte aligned": dict(label=_P + 4),
    "weight not 4-byte aligned": dict(weight=_P + 2),
}


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    a = dict(_GOOD)
    a.update(_BAD[name])
    lib = _weight.lib()
    rc = lib.ubw_pixel_weights(a["label"], a["weight"], a["counts"], a["B"], a["H"], a["W"], a["C"], a["max_weight"], a["r"], a["gain"],
                               a["lo"], None)
    msg = lib.ubw_last_error().decode()
    assert rc == -1 and msg.startswith("ubw_pixel_weights"), (rc, msg)
    with pytest.raises(RuntimeError, match="ubw_pixel_weights"):
        _weight.check(rc, name)
    assert C.sizeof(C.c_void_p) == 8


@pytest.mark.parametrize("kw", [dict(num_classes=0), dict(num_classes=17), dict(num_classes=3.0), dict(radius=-1), dict(radius=5),
                                dict(radius=True), dict(interface_from=-1), dict(interface_from=4), dict(max_weight=0.0),
                                dict(max_weight=float("nan")), dict(max_weight=-2.0), dict(gain=-1.0), dict(gain=float("nan")),
                                dict(gain=INF), dict(when="never")], ids=lambda kw: "%s=%r" % next(iter(kw.items())))
def test_pixel_weights_refuses_bad_arguments_in_the_constructor(kw, monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_weight, "lib", no_library)
    with pytest.raises(ValueError, match="PixelWeights"):
        PixelWeights(**kw)


def test_pixel_weights_defaults_and_the_host_half_takes_none():
    pw = PixelWeights()
    assert (pw.num_classes, pw.max_weight, pw.radius, pw.gain, pw.interface_from, pw.when) == (3, INF, 0, 1.0, 1, "missing")
    assert pw.counts is None
    pw = PixelWeights(num_classes=16, max_weight=20, radius=4, gain=0, interface_from=16, when="always")
    assert (pw.max_weight, pw.gain) == (20.0, 0.0)
    from ubresnet_amd.staging import BatchStager
    with pytest.raises(ValueError, match="weights"):
        BatchStager(object(), 2, 8, 8, device=None, pin=False, weights=pw)
    st = BatchStager(object(), 2, 8, 8, device=None, pin=False)
    assert st.weights is None and st.counts is None
    st.close()
