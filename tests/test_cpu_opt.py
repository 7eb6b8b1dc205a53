"""The guarded optimizer step without a GPU: libubresnet_opt.so's header is C99; header, binding and library agree on the entry
points and on the control block; the kernels compiled into it are exactly the ones the case table of tests/test_gpu_opt_exact.py
claims; the bias-correction table against kref.adam_ref's rounded corrections; opt_ref's decision rule by hand; the rule header
that ubr_opt.hip and ubr_group.hip share as a program of its own against opt_ref, bit for bit; every argument refusal returns its
error before any launch."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import kref
import opt_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_opt.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib, case_ids_run_by_the_gpu_module  # noqa: E402
from ubresnet_amd import _opt  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402

LIB = B.LIBS["opt"].out


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ubresnet_opt.h"\n'
                   'int main(void) {\n'
                   '  int (*n)(const float*, int64_t, float, float, int, const float*, int64_t, void*, void*) = ubo_grad_norm;\n'
                   '  int (*a)(float*, const float*, float*, float*, int64_t, float, float, float, float, float, const void*, void*) = ubo_adam_step;\n'
                   '  int (*s)(float*, const float*, float*, int64_t, float, float, float, float, int, const void*, void*) = ubo_sgd_step;\n'
                   '  int (*i)(void*, int64_t, void*) = ubo_ctl_init;\n'
                   '  return n == 0 || a == 0 || s == 0 || i == 0 || UBO_OK != 0 || sizeof(ubo_ctl) != UBO_CTL_HEAD_BYTES;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ubo_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_opt.SYMBOLS) and len(_opt.SYMBOLS) == len(set(_opt.SYMBOLS))
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBO_(BLOCK|UNROLL|MAX_GRID|CTL_HEAD_BYTES)\s+(\d+)", text)}
    assert geometry == dict(BLOCK=_opt.BLOCK, UNROLL=_opt.UNROLL, MAX_GRID=_opt.MAX_GRID, CTL_HEAD_BYTES=_opt.CTL_HEAD_BYTES)
    assert geometry == dict(BLOCK=R.BLOCK, UNROLL=R.UNROLL, MAX_GRID=R.MAX_GRID, CTL_HEAD_BYTES=R.CTL_HEAD_BYTES)
    assert re.search(r"#define\s+UBO_CTL_BYTES\s+\(UBO_CTL_HEAD_BYTES \+ 8 \* UBO_MAX_GRID\)", text)
    assert _opt.CTL_BYTES == R.CTL_BYTES == geometry["CTL_HEAD_BYTES"] + 8 * geometry["MAX_GRID"]
    need_lib(LIB)


def test_control_block_matches_the_header(tmp_path):
    """the ctypes Structure against offsetof() as a C compiler sees the header, and against opt_ref's table"""
    assert C.sizeof(_opt.Ctl) == _opt.CTL_HEAD_BYTES == 80
    mine = {name: getattr(_opt.Ctl, name).offset for name, _ in _opt.Ctl._fields_}
    assert mine == R.OFFSETS
    fields = ["sumsq", "norm", "scale", "gscale", "apply", "clipped", "bc1", "sqrt_bc2", "applied", "skipped", "clipped_total"]
    assert [n for n, _ in _opt.Ctl._fields_ if n not in ("reserved", "row")] == fields          # the order the ABI documents
    src, exe = tmp_path / "o.c", tmp_path / "o"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ubresnet_opt.h"\nint main(void) {\n' +
                   "".join('  printf("%s %%d\\n", (int)offsetof(ubo_ctl, %s));\n' % (n, n) for n in mine) +
                   '  printf("size %d\\nbytes %d\\n", (int)sizeof(ubo_ctl), (int)UBO_CTL_BYTES);\n  return 0;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().split("\n"))
    assert {k: int(v) for k, v in out.items()} == dict(mine, size=80, bytes=_opt.CTL_BYTES)
    types = dict(_opt.Ctl._fields_)
    assert types["sumsq"] is C.c_double and types["apply"] is C.c_int32 and types["applied"] is C.c_int64 and types["norm"] is C.c_float
    h = _opt.read_ctl(np.arange(96, dtype=np.uint8).tobytes())
    assert h.apply == int.from_bytes(bytes(range(20, 24)), "little") and h.skipped == int.from_bytes(bytes(range(48, 56)), "little")


def test_case_table_equals_the_compiled_kernels():
    need_lib(LIB)
    have = set(kernel_symbols.kernels(LIB))
    claimed = set(R.KERNEL_CASES)
    assert have - claimed == set(), "compiled kernels without a case in tests/test_gpu_opt_exact.py: %s" % sorted(have - claimed)
    assert claimed - have == set(), "cases for kernels that are not compiled: %s" % sorted(claimed - have)
    assert len(have) == 5
    assert case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_opt_exact.py"), call="_case") == set(i for ids in R.KERNEL_CASES.values() for i in ids)
    assert all(ids for ids in R.KERNEL_CASES.values())


def test_norm_sizes_follow_the_launch_geometry():
    s = R.norm_sizes()
    trip = R.BLOCK * R.UNROLL
    assert s["n4"] == 4 and R.grid(4) == 1
    assert (s["trip-1"], s["trip"], s["trip+1"]) == (4 * trip - 4, 4 * trip, 4 * trip + 4)
    assert [R.grid(s[k]) for k in ("trip-1", "trip", "trip+1")] == [1, 1, 2]
    n4 = s["two-trips"] // 4
    full = R.MAX_GRID * trip
    assert R.grid(s["two-trips"]) == R.MAX_GRID and s["two-trips"] % 4 == 0
    # second trip: lane l of the grid starts at unit full + l; the last workgroup's first lane is (MAX_GRID - 1) * BLOCK
    assert full + (R.MAX_GRID - 1) * R.BLOCK < n4 < full + R.MAX_GRID * R.BLOCK, "every workgroup works in the second trip, the last raggedly"
    assert (n4 - full) % R.BLOCK not in (0,) and n4 < 2 * full
    assert s["two-trips"] <= 6 * 2 ** 20, "at most a few million elements"


# ------------------------------------------------------------------------------------------------------------------------
# the bias-correction table
# ------------------------------------------------------------------------------------------------------------------------
def test_bias_table_equals_adam_refs_rounded_corrections():
    tab = _opt.bias_table(0.9, 0.999)
    assert tab.dtype == np.float32 and tab.ndim == 2 and tab.shape[1] == 2
    b1, b2 = kref.f32(0.9), kref.f32(0.999)
    for t in range(1, 201):
        want = (np.float32(kref.f32(1.0 - b1 ** t)), np.float32(kref.f32(math.sqrt(1.0 - b2 ** t))))       # adam_ref, round_bc=True
        assert (tab[t - 1, 0], tab[t - 1, 1]) == want, t
    # adam_ref itself, through a step whose result depends on the corrections: one element, step t, against the table's row
    p, g, z = torch.tensor([1.0]), torch.tensor([0.5]), torch.tensor([0.0])
    for t in (1, 2, 7, 200):
        (p1, m1, v1), _ = kref.adam_ref(p, g, z, z, 1e-3, 0.9, 0.999, 1e-8, 0.0, t)
        bc1, sbc2 = float(tab[t - 1, 0]), float(tab[t - 1, 1])
        den = math.sqrt(float(v1)) / sbc2 + kref.f32(1e-8)
        assert float(p1) == 1.0 - (kref.f32(1e-3) / bc1) * (float(m1) / den)
    assert np.array_equal(tab, R.bias_table(0.9, 0.999))


def test_bias_table_ends_where_both_corrections_are_one():
    tab = _opt.bias_table(0.9, 0.999)
    one = np.float32(1.0)
    assert tab[-1, 0] == one and tab[-1, 1] == one
    assert not (tab[-2, 0] == one and tab[-2, 1] == one)
    assert not ((tab[:-1, 0] == one) & (tab[:-1, 1] == one)).any()
    assert 16000 < len(tab) < 18000                                    # beta2^t < 2^-25 at t ~ 17.3 k
    assert (np.diff(tab[:, 0]) >= 0).all() and (np.diff(tab[:, 1]) >= 0).all()
    b2 = kref.f32(0.999)
    t = len(tab) + 1000                                                # and they stay there
    assert np.float32(1.0 - b2 ** t) == one and np.float32(math.sqrt(1.0 - b2 ** t)) == one


def test_bias_table_of_zero_betas_has_one_row_and_long_tables_are_refused():
    tab = _opt.bias_table(0.0, 0.0)
    assert tab.shape == (1, 2) and tab[0, 0] == 1.0 and tab[0, 1] == 1.0
    with pytest.raises(ValueError):
        _opt.bias_table(0.9, 1.0)
    assert _opt.MAX_TABLE == 4 << 20
    # 1 - 2^-24 is a float; its powers fall below 2^-25 only after ~2.9e8 steps
    with pytest.raises(ValueError, match="more than"):
        old, _opt.MAX_TABLE = _opt.MAX_TABLE, 5000
        try:
            _opt.bias_table(0.9, 1.0 - 2.0 ** -24)
        finally:
            _opt.MAX_TABLE = old


# ------------------------------------------------------------------------------------------------------------------------
# the decision rule, by hand
# ------------------------------------------------------------------------------------------------------------------------
def test_decide_reference_by_hand():
    tab = R.bias_table(0.9, 0.999)
    st = dict(applied=0, skipped=0, clipped_total=0, bc1=np.float32(0), sqrt_bc2=np.float32(0))
    d = R.decide(9.0, 1.0, 6.0, True, st, tab)                         # norm 3 under max_norm 6
    assert d["norm"] == 3.0 and d["scale"] == 1.0 and d["gscale"] == 1.0 and d["apply"] == 1 and d["clipped"] == 0 and d["applied"] == 1
    assert d["bc1"] == tab[0, 0]
    d = R.decide(16.0, -0.5, 1.0, True, st, tab)                       # |grad_scale| in the norm, its sign in gscale
    assert d["norm"] == 2.0 and d["scale"] == np.float32(1.0) / (np.float32(2.0) + np.float32(1e-6)) and d["gscale"] == np.float32(-0.5) * d["scale"]
    assert d["clipped"] == 1 and d["clipped_total"] == 1 and d["applied"] == 2 and d["sqrt_bc2"] == tab[1, 1]
    for bad in (float("nan"), float("inf")):
        d = R.decide(bad, 1.0, 1.0, True, st, tab)
        assert d["apply"] == 0 and d["clipped"] == 0 and d["applied"] == 2 and d["bc1"] == tab[1, 0]
    assert st["skipped"] == 2
    d = R.decide(float("nan"), 1.0, -1.0, False, st, tab)              # not guarded: applies, as the plain step does
    assert d["apply"] == 1 and d["scale"] == 1.0 and d["applied"] == 3 and math.isnan(d["norm"])
    d = R.decide(4.0, 1.0, -1.0, True, st, tab[:2])                    # past the table's end: its last row
    assert d["applied"] == 4 and d["bc1"] == tab[1, 0] and d["scale"] == 1.0


# ------------------------------------------------------------------------------------------------------------------------
# the rule header as a program
# ------------------------------------------------------------------------------------------------------------------------
def _f32(s):
    return np.array([int(s, 16)], np.uint32).view(np.float32)[0]


def _f64(s):
    return float(np.array([int(s, 16)], np.uint64).view(np.float64)[0])


def _b32(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def test_rule_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/opt_rule_host.cpp has its own main and includes ubr_opt_rule.h; built with -fsanitize=address,undefined and
    -ffp-contract=off (as the libraries are) and run as a process of its own.  Everything is compared bit for bit: the sum of
    squares against fp64 (the square of a float32 is exact there); fourteen decisions of one control block in sequence against
    opt_ref.decide -- clipped, not clipped, max_norm < 0 and 0, a sum of 0, inf and NaN with the guard on and off, tables shorter
    than the applied count; 54 Adam elements at t = 1, inside and past the table's end, and 216 SGD elements -- plain, momentum
    first and later step, nesterov -- against numpy fp32 with the fused multiply-add rounded once (opt_ref.fma32)"""
    exe = str(tmp_path / "opt_rule_host")
    r = subprocess.run([cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-Wall", "-Werror", "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "opt_rule_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
    rows = [l.replace("|", " ").split() for l in p.stdout.strip().split("\n")]
    by = {k: [row[1:] for row in rows if row[0] == k] for k in "TQDAS"}
    assert [len(by[k]) for k in "TQDAS"] == [4, 16, 14, 54, 216] and len(rows) == 304
    # fma32 itself: where a * b + c is a float32 it is that; where fp64 rounds twice it differs from the fp64 emulation
    assert R.fma32(np.float32(0.0625), np.float32(1.5), np.float32(0.375)) == np.float32(0.46875)
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -53)      # 1 + 2^-11 + 2^-24 (a tie) + 2^-53
    assert R.fma32(a, b, c) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23) != np.float32(float(a) * float(b) + float(c))
    table = np.array([[_f32(x), _f32(y)] for _, x, y in by["T"]], np.float32)
    assert np.array_equal(table, R.bias_table(0.9, 0.999)[:4])
    with np.errstate(all="ignore"):
        for acc, x, y, z, w, got in by["Q"]:
            want = _f64(acc)
            for v in (x, y, z, w):
                want = want + float(_f32(v)) * float(_f32(v))
            assert int(got, 16) == int(np.array([want]).view(np.uint64)[0]) or (math.isnan(want) and math.isnan(_f64(got))), (acc, x, y, z, w)
        # the decisions
        st = dict(applied=0, skipped=0, clipped_total=0, bc1=np.float32(0), sqrt_bc2=np.float32(0))
        seen = set()
        for sumsq, gs, mn, skip, bc_len, norm, scale, gscale, apply, clipped, bc1, sbc2, applied, skipped, ctotal, r0, r1, r2, r3 in by["D"]:
            what = (sumsq, gs, mn, skip, bc_len)
            d = R.decide(_f64(sumsq), float(_f32(gs)), float(_f32(mn)), bool(int(skip)), st, table[:int(bc_len)])
            same = lambda got, want: int(got, 16) == _b32(want) or (np.isnan(want) and np.isnan(_f32(got)))
            assert same(norm, d["norm"]) and same(scale, d["scale"]) and same(gscale, d["gscale"]), what
            assert (int(apply), int(clipped)) == (d["apply"], d["clipped"]), what
            assert (int(applied), int(skipped), int(ctotal)) == (d["applied"], d["skipped"], d["clipped_total"]), what
            assert int(bc1, 16) == _b32(d["bc1"]) and int(sbc2, 16) == _b32(d["sqrt_bc2"]), what
            assert (r0, r1, r3) == (norm, scale, gscale) and _f32(r2) == float(d["apply"]), what
            seen.add((d["apply"], d["clipped"], bool(_f32(mn) < 0), d["apply"] == 1 and int(bc_len) < d["applied"]))
        assert st["applied"] == 12 and st["skipped"] == 2 and st["clipped_total"] >= 3      # the guard skips the inf and the NaN only
        assert {(1, 0, False, False), (1, 1, False, False), (1, 0, True, False), (0, 0, False, False), (1, 1, False, True)} <= seen
        # the elements
        for p0, g, m, v, gs, wd, b1, b2, eps, lr, t, bc_len, p1, m1, v1 in by["A"]:
            row = table[min(int(t), int(bc_len)) - 1]
            want = R.adam_element(*(_f32(x) for x in (p0, g, m, v, gs, wd, b1, b2, eps, lr)), row[0], row[1])
            assert [int(x, 16) for x in (p1, m1, v1)] == [_b32(x) for x in want], (p0, g, m, v, gs, wd, t)
        assert {int(a[10]) for a in by["A"]} == {1, 3, 9}
        forms = set()
        for p0, g, b, gs, wd, lr, mom, damp, has_buf, first, nesterov, p1, b1 in by["S"]:
            form = (int(has_buf), int(first), int(nesterov))
            want = R.sgd_element(*(_f32(x) for x in (p0, g, b, gs, wd, lr, mom, damp)), *form)
            assert [int(x, 16) for x in (p1, b1)] == [_b32(x) for x in want], (p0, g, b, gs, wd, damp, form)
            forms.add(form)
        assert forms == {(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0), (1, 1, 1), (1, 0, 1)}


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------------------------------
# addresses that are never dereferenced: every call below is refused on the host, before any launch.  n = 64 floats (256 bytes)
_P = 0x100000
_G = dict(param=_P, grad=_P + 0x1000, m=_P + 0x2000, v=_P + 0x3000, table=_P + 0x4000, ctl=_P + 0x10000, n=64, max_norm=1.0,
          bc_len=4, momentum=0.9)
_INSIDE = _P + 0x10000 + R.CTL_BYTES - 16          # a 16-byte aligned address whose buffer starts inside the control block
_BAD = {
    "norm: null grad": ("norm", dict(grad=None), "null pointer"),
    "norm: null table": ("norm", dict(table=None), "null pointer"),
    "norm: null ctl": ("norm", dict(ctl=None), "null pointer"),
    "norm: n 0": ("norm", dict(n=0), "n=0 must be positive"),
    "norm: n negative": ("norm", dict(n=-4), "n=-4"),
    "norm: n % 4": ("norm", dict(n=62), "multiple of 4"),
    "norm: grad alignment": ("norm", dict(grad=_P + 0x1004), "16-byte aligned"),
    "norm: ctl alignment": ("norm", dict(ctl=_P + 0x10008), "16-byte aligned"),
    "norm: NaN max_norm": ("norm", dict(max_norm=float("nan")), "max_norm is NaN"),
    "norm: bc_len 0": ("norm", dict(bc_len=0), "bc_len=0 must be >= 1"),
    "norm: ctl overlaps grad": ("norm", dict(grad=_INSIDE), "ctl overlaps grad"),
    "norm: grad ends inside ctl": ("norm", dict(grad=_P + 0x10000 - 240), "ctl overlaps grad"),
    "norm: ctl overlaps the table": ("norm", dict(table=_INSIDE), "ctl overlaps bc_table"),
    "adam: null param": ("adam", dict(param=None), "null pointer"),
    "adam: null exp_avg_sq": ("adam", dict(v=None), "null pointer"),
    "adam: null ctl": ("adam", dict(ctl=None), "null pointer"),
    "adam: n 0": ("adam", dict(n=0), "n=0 must be positive"),
    "adam: n % 4": ("adam", dict(n=62), "multiple of 4"),
    "adam: exp_avg alignment": ("adam", dict(m=_P + 0x2004), "16-byte aligned"),
    "adam: ctl overlaps exp_avg": ("adam", dict(m=_INSIDE), "ctl overlaps exp_avg"),
    "adam: ctl overlaps param": ("adam", dict(param=_P + 0x10000), "ctl overlaps param"),
    "sgd: null grad": ("sgd", dict(grad=None), "null pointer"),
    "sgd: n % 4": ("sgd", dict(n=62), "multiple of 4"),
    "sgd: momentum without a buffer": ("sgd", dict(m=None), "momentum buffer iff momentum != 0"),
    "sgd: a buffer without momentum": ("sgd", dict(momentum=0.0), "momentum buffer iff momentum != 0"),
    "sgd: param alignment": ("sgd", dict(param=_P + 8), "16-byte aligned"),
    "sgd: ctl overlaps the momentum buffer": ("sgd", dict(m=_INSIDE), "ctl overlaps momentum_buf"),
    "init: null ctl": ("init", dict(ctl=None), "null ctl"),
    "init: ctl alignment": ("init", dict(ctl=_P + 4), "16-byte aligned"),
    "init: negative count": ("init", dict(applied=-1), "applied=-1 must be >= 0"),
}
_ENTRY = dict(norm="ubo_grad_norm", adam="ubo_adam_step", sgd="ubo_sgd_step", init="ubo_ctl_init")


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    which, change, message = _BAD[name]
    a = dict(_G, applied=0)
    a.update(change)
    lib = _opt.lib()
    if which == "norm":
        rc = lib.ubo_grad_norm(a["grad"], a["n"], 1.0, a["max_norm"], 1, a["table"], a["bc_len"], a["ctl"], None)
    elif which == "adam":
        rc = lib.ubo_adam_step(a["param"], a["grad"], a["m"], a["v"], a["n"], 1e-3, 0.9, 0.999, 1e-8, 1e-4, a["ctl"], None)
    elif which == "sgd":
        rc = lib.ubo_sgd_step(a["param"], a["grad"], a["m"], a["n"], 1e-2, a["momentum"], 0.0, 1e-4, 0, a["ctl"], None)
    else:
        rc = lib.ubo_ctl_init(a["ctl"], a["applied"], None)
    msg = lib.ubo_last_error().decode()
    assert rc == -1 and msg.startswith(_ENTRY[which] + ":") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=_ENTRY[which]):
        _opt.check(rc, name)
    assert C.sizeof(C.c_void_p) == 8
