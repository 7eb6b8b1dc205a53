"""The gradient-accumulation library without a GPU: libubresnet_accum.so's header is C99; header, binding, reference and library
agree on the entry points and the geometry; every argument refusal returns UBC_EINVAL with a message before any launch; the numpy
reference against an fp64 sum; GradAccumulator's and epoch.train's refusals that need no device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import accum_ref as R
import kref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_accum.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib  # noqa: E402
from ubresnet_amd import _accum as A  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402

LIB = B.LIBS["accum"].out
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_accum.h"\n'
                     'int main(void) {\n'
                     '  int (*s)(float*, const float*, int64_t, void*) = ubc_set;\n'
                     '  int (*a)(float*, const float*, int64_t, void*) = ubc_add;\n'
                     '  int (*f)(float*, const float*, int64_t, float, void*) = ubc_finish;\n'
                     '  const char* (*e)(void) = ubc_last_error;\n'
                     '  int (*v)(void) = ubc_version;\n'
                     '  return s == 0 || a == 0 || f == 0 || e == 0 || v == 0 || UBC_OK != 0 || UBC_EINVAL != -1 || UBC_ELAUNCH != -2;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ubc_[a-z_0-9]+)\s*\(", text))
    need_lib(LIB)
    assert declared == set(A.SYMBOLS) and len(A.SYMBOLS) == len(set(A.SYMBOLS)) == 5
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBC_(BLOCK|UNROLL|MAX_GRID)\s+(\d+)", text)}
    assert geometry == dict(BLOCK=A.BLOCK, UNROLL=A.UNROLL, MAX_GRID=A.MAX_GRID)
    assert geometry == dict(BLOCK=R.BLOCK, UNROLL=R.UNROLL, MAX_GRID=R.MAX_GRID) and R.TRIP == R.BLOCK * R.UNROLL
    # the arithmetic rules are stated in the header
    for phrase in ("rounded to nearest even", "contracted", "Subnormal", "NaN", "payload"):
        assert phrase in raw, phrase
    # three kernels
    assert sorted(k.split("(")[0].split("::")[-1] for k in kernel_symbols.kernels(LIB)) == ["add_kernel", "finish_kernel", "set_kernel"]


def test_the_sizes_cover_the_paths_of_the_launch():
    t = R.TRIP
    sizes = R.flat_sizes()
    assert sizes == [4, 4 * (t - 1), 4 * t, 4 * (t + 1), 4 * (R.MAX_GRID * t + 1)]
    assert [R.grid(n) for n in sizes] == [1, 1, 1, 2, R.MAX_GRID]
    assert sizes[-1] // 4 == R.MAX_GRID * R.BLOCK * R.UNROLL + 1 and 15 << 20 < 4 * sizes[-1] < 17 << 20      # about 16 MB per buffer


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------------------------------
# addresses that are never dereferenced: every call below is refused on the host, before any launch.  n = 64 floats (256 bytes)
_P = 0x100000
_A = dict(acc=_P, grad=_P + 0x1000, n=64, scale=0.25)
_PAIR = {
    "null acc": (dict(acc=None), "null pointer"),
    "null grad": (dict(grad=None), "null pointer"),
    "n 0": (dict(n=0), "n=0 must be positive"),
    "n negative": (dict(n=-4), "n=-4 must be positive"),
    "n % 4": (dict(n=62), "multiple of 4"),
    "acc alignment": (dict(acc=_P + 4), "16-byte aligned"),
    "grad alignment": (dict(grad=_P + 0x1008), "16-byte aligned"),
    "acc is grad": (dict(grad=_P), "acc overlaps grad"),
    "grad starts inside acc": (dict(grad=_P + 240), "acc overlaps grad"),
    "acc starts inside grad": (dict(acc=_P + 0x1000 + 240), "acc overlaps grad"),
}
_SCALE = {
    "scale zero": (dict(scale=0.0), "finite and > 0"),
    "scale negative": (dict(scale=-0.5), "finite and > 0"),
    "scale negative zero": (dict(scale=-0.0), "finite and > 0"),
    "scale inf": (dict(scale=float("inf")), "finite and > 0"),
    "scale -inf": (dict(scale=float("-inf")), "finite and > 0"),
    "scale NaN": (dict(scale=float("nan")), "scale is NaN"),
}
_BAD = {"%s: %s" % (w, k): (w, c, m) for w in ("set", "add", "finish") for k, (c, m) in _PAIR.items()}
_BAD.update({"finish: %s" % k: ("finish", c, m) for k, (c, m) in _SCALE.items()})
_ENTRY = dict(set="ubc_set", add="ubc_add", finish="ubc_finish")


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    which, change, message = _BAD[name]
    a = dict(_A)
    a.update(change)
    lib = A.lib()
    if which == "set":
        rc = lib.ubc_set(a["acc"], a["grad"], a["n"], None)
    elif which == "add":
        rc = lib.ubc_add(a["acc"], a["grad"], a["n"], None)
    else:
        rc = lib.ubc_finish(a["grad"], a["acc"], a["n"], a["scale"], None)
    msg = lib.ubc_last_error().decode()
    assert rc == -1 and msg.startswith(_ENTRY[which] + ":") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=_ENTRY[which]):
        A.check(rc, name)


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def _rounded64(grads, scale):
    """(g1 + ... + gK) * scale in float64, rounded to fp32 once"""
    s = np.zeros(grads[0].shape, dtype=np.float64)
    for g in grads:
        s += g.astype(np.float64)
    return (s * float(f32(scale))).astype(f32)


def test_reference_by_hand():
    g = f32([1.0, -0.0, 1e-45, 3e38])
    s = R.set_(g)
    assert s.view(np.uint32).tolist() == g.view(np.uint32).tolist() and s is not g
    nan = np.array([0x7fc12345], dtype=np.uint32).view(f32)
    assert R.set_(nan).view(np.uint32).tolist() == [0x7fc12345]                        # a payload survives the copy
    a = R.add(f32([1.0, -0.0, 1e-45, 3e38]), f32([2.0, -0.0, 1e-45, 3e38]))
    assert a.dtype == f32 and a.view(np.uint32).tolist() == [0x40400000, 0x80000000, 2, 0x7f800000]
    fin = R.finish(f32([1.0, 3e38, 3e-45, np.inf]), f32([2.0, 3e38, 1e-45, -np.inf]), f32(0.5))
    assert fin.view(np.uint32).tolist()[:3] == [0x3fc00000, 0x7f800000, 2] and np.isnan(fin[3])  # inf * 0.5 = inf: the sum overflowed first; 3 * 2^-149 / 2 ties to even: 2
    assert R.scale_of(4) == f32(0.25) and R.scale_of(3) == f32(1.0 / 3.0) and R.scale_of(3, average=False) == f32(1.0)
    assert R.cycle([f32([1.0]), f32([2.0])], 0.5).tolist() == [1.5]


@pytest.mark.parametrize("every", [2, 4])
def test_reference_cycle_is_exact_on_dyadic_operands(every):
    """small dyadic operands (kref.exact_operands) and a power-of-two scale: every operation is exact, so the replay IS the
    fp64 sum times the scale"""
    n = 4 * (R.TRIP + 1)
    grads = [kref.exact_operands((n,), torch.float32, density=0.75, seed=10 * every + k, exp=k - 3, maxmag=7).numpy() for k in range(every)]
    assert all(np.count_nonzero(g) > n // 2 for g in grads)
    for average in (True, False):
        scale = R.scale_of(every, average)
        got = R.cycle(grads, scale)
        want = _rounded64(grads, scale)
        assert got.dtype == f32 and got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert np.count_nonzero(want) > n // 2


@pytest.mark.parametrize("every", [2, 3, 4])
def test_reference_cycle_stays_within_k_ulp_on_random_operands(every):
    """operands of one sign, in [1, 2): every partial sum is at most the final one, so each of the K - 1 additions errs by at
    most half an ulp of the final sum, the product by half an ulp of the result (whose ulp is the sum's times the scale, up to
    the scale's own half-ulp error when it is 1/3), and the reference's single rounding by another half: below K ulp"""
    rs = np.random.RandomState(every)
    n = 1 << 14
    grads = [(1.0 + rs.random_sample(n)).astype(f32) for _ in range(every)]
    scale = R.scale_of(every)
    got, want = R.cycle(grads, scale), _rounded64(grads, scale)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp
    assert float(err.max()) <= every, float(err.max())
    assert float(err.max()) > 0 or every == 2                                          # the bound is not vacuous: roundings do happen


# ------------------------------------------------------------------------------------------------------------------------
# GradAccumulator, epoch.train
# ------------------------------------------------------------------------------------------------------------------------
def test_accumulator_refusals_that_need_no_device():
    from ubresnet_amd.accum import GradAccumulator
    lin = torch.nn.Linear(3, 2)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="every must be an integer >= 1"):
            GradAccumulator(lin, every=bad)
    one = GradAccumulator(lin, every=1, average=False)
    assert (one.every, one.average, one.pending) == (1, False, 0)
    assert one.add() is True and one.pending == 0                                      # nothing to launch, nothing to check
    one.reset()
    with pytest.raises(AttributeError):
        one.every = 2
    with pytest.raises(AttributeError):
        one.average = True
    assert not hasattr(one, "state_dict")


def test_epoch_train_refuses_a_cycle_left_open():
    import inspect
    from ubresnet_amd.training import epoch
    p = inspect.signature(epoch.train).parameters
    assert p["accumulate"].default == 1 and list(p)[-1] == "ema"
    with pytest.raises(ValueError, match="not a multiple of accumulate=2"):
        epoch.train(None, None, None, None, 5, accumulate=2)                           # before the first batch: nothing is touched
    with pytest.raises(ValueError, match="accumulate must be an integer >= 1"):
        epoch.train(None, None, None, None, 4, accumulate=0)
