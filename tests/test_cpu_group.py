"""The grouped optimizer library without a GPU: libubresnet_group.so's header is C99; header, binding and library agree on the entry
points and on the control block, whose head is ubo_ctl's; the kernels compiled into it are exactly the ones the case table of
tests/test_gpu_group_exact.py claims; the tile planner (pure host code) against group_ref's, through the library and as a
stand-alone program under the host sanitizers; every argument refusal returns its error before any launch; split_decay, the group
rules and torch's numbering of state_dict() on a stand-in that launches nothing."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import group_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_group.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib, case_ids_run_by_the_gpu_module  # noqa: E402
from ubresnet_amd import _group as G  # noqa: E402
from ubresnet_amd import _opt  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402

LIB = B.LIBS["group"].out


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ubresnet_group.h"\n'
                   'int main(void) {\n'
                   '  int64_t (*p)(const int64_t*, const int64_t*, int64_t, ubg_tile*, int64_t) = ubg_plan_tiles;\n'
                   '  int (*n)(const float*, int64_t, const void*, int64_t, const void*, void*, int64_t, float, float, int, const float*, int64_t, void*, void*) = ubg_grad_norm;\n'
                   '  int (*v)(const void*, void*, int64_t, float, const float*, int64_t, void*, void*) = ubg_advance;\n'
                   '  int (*a)(float*, const float*, float*, float*, int64_t, const void*, int64_t, const void*, const void*, int64_t, float, float, float, const void*, void*) = ubg_adam_step;\n'
                   '  int (*s)(float*, const float*, float*, int64_t, const void*, int64_t, const void*, const void*, int64_t, float, float, int, const void*, void*) = ubg_sgd_step;\n'
                   '  int (*ss)(void*, int64_t, int64_t, int64_t, const int64_t*, const float*, int64_t, void*) = ubg_state_set;\n'
                   '  int (*sg)(const void*, int64_t, ubg_state*, void*) = ubg_state_get;\n'
                   '  return p == 0 || n == 0 || v == 0 || a == 0 || s == 0 || ss == 0 || sg == 0 || UBG_OK != 0 || sizeof(ubg_ctl) != UBG_CTL_HEAD_BYTES\n'
                   '         || sizeof(ubg_tile) != 16 || sizeof(ubg_hyper) != 16 || sizeof(ubg_state) != 16;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ubg_[a-z_0-9]+)\s*\(", text))
    need_lib(LIB)
    assert declared == set(G.SYMBOLS) and len(G.SYMBOLS) == len(set(G.SYMBOLS))
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBG_(BLOCK|TILE_UNITS|MAX_GRID|STEP_GRID|CTL_HEAD_BYTES)\s+(\d+)", text)}
    assert geometry == dict(BLOCK=G.BLOCK, TILE_UNITS=G.TILE_UNITS, MAX_GRID=G.MAX_GRID, STEP_GRID=G.STEP_GRID, CTL_HEAD_BYTES=G.CTL_HEAD_BYTES)
    assert geometry == dict(BLOCK=R.BLOCK, TILE_UNITS=R.TILE_UNITS, MAX_GRID=R.MAX_GRID, STEP_GRID=R.STEP_GRID, CTL_HEAD_BYTES=R.CTL_HEAD_BYTES)
    assert G.TILE_UNITS == 4 * G.BLOCK == 1024
    assert re.search(r"#define\s+UBG_CTL_BYTES\s+\(UBG_CTL_HEAD_BYTES \+ 8 \* UBG_MAX_GRID\)", text)
    assert G.CTL_BYTES == R.CTL_BYTES == _opt.CTL_BYTES == geometry["CTL_HEAD_BYTES"] + 8 * geometry["MAX_GRID"]


def test_control_block_head_is_ubo_ctl_field_by_field(tmp_path):
    """offsetof() of every field of ubg_ctl and of ubo_ctl as a C compiler sees the two headers; the record sizes likewise"""
    need_lib(LIB)
    assert C.sizeof(G.Ctl) == G.CTL_HEAD_BYTES == 80
    mine = {name: getattr(G.Ctl, name).offset for name, _ in G.Ctl._fields_}
    assert mine == R.OFFSETS
    assert [(n, t) for n, t in G.Ctl._fields_] == [(n, t) for n, t in _opt.Ctl._fields_]
    src, exe = tmp_path / "o.c", tmp_path / "o"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ubresnet_group.h"\n#include "ubresnet_opt.h"\nint main(void) {\n' +
                   "".join('  printf("%s %%d %%d %%d\\n", (int)offsetof(ubg_ctl, %s), (int)offsetof(ubo_ctl, %s), '
                           '(int)(sizeof(((ubg_ctl*)0)->%s) == sizeof(((ubo_ctl*)0)->%s)));\n' % (n, n, n, n, n) for n in mine) +
                   '  printf("size %d %d 1\\n", (int)sizeof(ubg_ctl), (int)sizeof(ubo_ctl));\n'
                   '  printf("bytes %d %d 1\\n", (int)UBG_CTL_BYTES, (int)UBO_CTL_BYTES);\n'
                   '  printf("tile %d %d %d\\n", (int)offsetof(ubg_tile, unit0), (int)offsetof(ubg_tile, units), (int)offsetof(ubg_tile, seg));\n'
                   '  printf("hyper %d %d %d\\n", (int)offsetof(ubg_hyper, lr), (int)offsetof(ubg_hyper, weight_decay), (int)offsetof(ubg_hyper, active));\n'
                   '  printf("state %d %d %d\\n", (int)offsetof(ubg_state, applied), (int)offsetof(ubg_state, bc1), (int)offsetof(ubg_state, sqrt_bc2));\n'
                   '  return 0;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {l.split()[0]: tuple(int(x) for x in l.split()[1:]) for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().split("\n")}
    for name, off in mine.items():
        assert out[name] == (off, off, 1), name
    assert out["size"] == (80, 80, 1) and out["bytes"] == (G.CTL_BYTES, _opt.CTL_BYTES, 1)
    assert out["tile"] == tuple(G.TILE.fields[k][1] for k in ("unit0", "units", "seg")) == (0, 8, 12)
    assert out["hyper"] == tuple(G.HYPER.fields[k][1] for k in ("lr", "weight_decay", "active")) == (0, 4, 8)
    assert out["state"] == tuple(G.STATE.fields[k][1] for k in ("applied", "bc1", "sqrt_bc2")) == (0, 8, 12)
    assert G.TILE.itemsize == G.HYPER.itemsize == G.STATE.itemsize == 16
    h = G.read_ctl(np.arange(96, dtype=np.uint8).tobytes())
    assert h.apply == int.from_bytes(bytes(range(20, 24)), "little") and h.skipped == int.from_bytes(bytes(range(48, 56)), "little")


def test_case_table_equals_the_compiled_kernels():
    need_lib(LIB)
    have = set(kernel_symbols.kernels(LIB))
    claimed = set(R.KERNEL_CASES)
    assert have - claimed == set(), "compiled kernels without a case in tests/test_gpu_group_exact.py: %s" % sorted(have - claimed)
    assert claimed - have == set(), "cases for kernels that are not compiled: %s" % sorted(claimed - have)
    assert case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_group_exact.py"), call="_case") == set(i for ids in R.KERNEL_CASES.values() for i in ids)
    assert all(ids for ids in R.KERNEL_CASES.values())


def test_the_other_optimizer_library_is_as_it_was():
    """libubresnet_opt.so keeps its five kernels and its exports"""
    need_lib(B.LIBS["opt"].out)
    assert len(kernel_symbols.kernels(B.LIBS["opt"].out)) == 5
    assert _opt.SYMBOLS == ["ubo_ctl_init", "ubo_grad_norm", "ubo_adam_step", "ubo_sgd_step", "ubo_last_error", "ubo_version"]


# ------------------------------------------------------------------------------------------------------------------------
# the tile planner
# ------------------------------------------------------------------------------------------------------------------------
def _lists():
    return [(name, R.starts(units) if u0 is None else u0, units) for name, u0, units in R.PLAN_LISTS]


def test_reference_planner_by_hand():
    assert R.plan_tiles([0], [1]) == [(0, 1, 0)]
    assert R.plan_tiles([0, 1024], [1024, 1025]) == [(0, 1024, 0), (1024, 1024, 1), (2048, 1, 1)]
    assert R.plan_tiles([7], [3 * 1024 + 1]) == [(7, 1024, 0), (1031, 1024, 0), (2055, 1024, 0), (3079, 1, 0)]
    assert [n for n, _, _ in _lists()][:4] == ["edges", "single", "single-unit", "ones"]
    assert dict((n, u) for n, _, u in _lists())["edges"] == [1, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 1] and len(dict((n, u) for n, _, u in _lists())["ones"]) == 300


@pytest.mark.parametrize("name", [n for n, _, _ in R.PLAN_LISTS])
def test_plan_tiles_equals_the_reference_planner(name):
    need_lib(LIB)
    u0, units = {n: (a, b) for n, a, b in _lists()}[name]
    want = R.plan_tiles(u0, units)
    got = G.plan_tiles(u0, units)
    assert [(int(t["unit0"]), int(t["units"]), int(t["seg"])) for t in got] == want
    assert len(got) == G.tile_count(units)
    # properties, whatever the reference says: ascending, inside one segment, at most a tile, every unit of every segment once
    covered = 0
    for k, (a, n, s) in enumerate(want):
        assert 1 <= n <= R.TILE_UNITS and u0[s] <= a and a + n <= u0[s] + units[s]
        assert k == 0 or a >= want[k - 1][0] + want[k - 1][1]
        covered += n
    assert covered == sum(units)
    # with room for more the rest of the table is left alone
    room = np.full(len(want) + 3, -1, dtype=np.int64).repeat(2).view(G.TILE)
    a0, a1 = np.asarray(u0, np.int64), np.asarray(units, np.int64)
    assert G.lib().ubg_plan_tiles(a0.ctypes.data, a1.ctypes.data, len(u0), room.ctypes.data, len(room)) == len(want)
    assert (room[len(want):].view(np.int64) == -1).all()


@pytest.mark.parametrize("name", [n for n, _, _ in R.PLAN_LISTS if n != "single-unit"])
def test_plan_tiles_refuses_a_table_that_is_too_small(name):
    need_lib(LIB)
    u0, units = {n: (a, b) for n, a, b in _lists()}[name]
    want = R.plan_tiles(u0, units)
    cap = len(want) - 1
    table = np.full(2 * (len(want) + 2), -1, dtype=np.int64).view(G.TILE)
    a0, a1 = np.asarray(u0, np.int64), np.asarray(units, np.int64)
    rc = G.lib().ubg_plan_tiles(a0.ctypes.data, a1.ctypes.data, len(u0), table.ctypes.data, cap)
    msg = G.lib().ubg_last_error().decode()
    assert rc == -1 and "cap=%d is too small for %d tiles" % (cap, len(want)) in msg, (rc, msg)
    assert (table[cap:].view(np.int64) == -1).all(), "wrote at or past tiles[cap]"
    with pytest.raises(RuntimeError, match="too small"):
        G.plan_tiles(u0, units, cap=cap)


_BAD_PLANS = {
    "no segments": ([], [], "nseg=0"),
    "zero units": ([0, 4], [4, 0], "segment 1 has 0 units"),
    "negative units": ([0], [-3], "segment 0 has -3 units"),
    "overlap": ([0, 3], [4, 4], "segment 1 starts at unit 3"),
    "descending": ([10, 0], [1, 1], "segment 1 starts at unit 0"),
    "negative start": ([-1], [1], "segment 0 starts at unit -1"),
}


@pytest.mark.parametrize("name", sorted(_BAD_PLANS))
def test_plan_tiles_refuses_bad_segments(name):
    need_lib(LIB)
    u0, units, message = _BAD_PLANS[name]
    a0, a1 = np.asarray(u0 + [0], np.int64), np.asarray(units + [0], np.int64)
    table = np.full(64, -1, dtype=np.int64).view(G.TILE)
    rc = G.lib().ubg_plan_tiles(a0.ctypes.data, a1.ctypes.data, len(u0), table.ctypes.data, len(table))
    msg = G.lib().ubg_last_error().decode()
    assert rc == -1 and msg.startswith("ubg_plan_tiles:") and message in msg, (rc, msg)
    assert (table.view(np.int64) == -1).all(), "a refused plan wrote tiles"
    assert G.lib().ubg_plan_tiles(None, a1.ctypes.data, 1, table.ctypes.data, 4) == -1 and "null pointer" in G.lib().ubg_last_error().decode()


def test_planner_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/group_plan_host.cpp has its own main and includes the planner's header; built with -fsanitize=address,undefined and
    run as a process of its own over the same segment lists, with a table of exactly `cap` tiles on the heap"""
    exe = str(tmp_path / "group_plan_host")
    r = subprocess.run([cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "group_plan_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(cap, u0, units):
        p = subprocess.run([exe, str(cap)] + ["%d:%d" % (a, b) for a, b in zip(u0, units)], capture_output=True, text=True)
        assert p.returncode == 0, "sanitizer or planner failure:\n" + p.stderr[-2000:]
        lines = p.stdout.strip().split("\n")
        head = lines[0].split()
        return int(head[1]), int(head[3]), int(head[5]), [tuple(int(x) for x in l.split()) for l in lines[1:]]
    for name, u0, units in _lists():
        want = R.plan_tiles(u0, units)
        assert run(len(want), u0, units) == (len(want), 0, -1, want), name
        if len(want) > 1:                                       # too small: counted, the first cap tiles written, nothing past
            n, err, _, tiles = run(len(want) - 1, u0, units)
            assert (n, err != 0, tiles) == (len(want), True, want[:-1]), name
        n, err, _, tiles = run(0, u0, units)
        assert (n, err != 0, tiles) == (len(want), True, []), name
    for name, (u0, units, _) in _BAD_PLANS.items():
        if u0:
            n, err, bad, tiles = run(8, u0, units)
            assert err != 0 and tiles == [] and 0 <= bad < len(u0), name


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------------------------------
# addresses that are never dereferenced: every call below is refused on the host, before any launch.  n = 64 floats (256 bytes),
# 4 tiles, 3 segments
_P = 0x100000
_A = dict(param=_P, grad=_P + 0x1000, m=_P + 0x2000, v=_P + 0x3000, table=_P + 0x4000, tiles=_P + 0x5000, hyper=_P + 0x6000,
          state=_P + 0x7000, counts=_P + 0x8000, out=_P + 0x9000, ctl=_P + 0x10000, n=64, ntiles=4, nseg=3, max_norm=1.0, bc_len=4,
          momentum=0.9, seg0=0, count=3)
_INSIDE = _P + 0x10000 + R.CTL_BYTES - 16          # a 16-byte aligned address whose buffer starts inside the control block
_BAD = {
    "norm: null grad": ("norm", dict(grad=None), "null pointer"),
    "norm: null tiles": ("norm", dict(tiles=None), "null pointer"),
    "norm: null hyper": ("norm", dict(hyper=None), "null pointer"),
    "norm: null state": ("norm", dict(state=None), "null pointer"),
    "norm: null table": ("norm", dict(table=None), "null pointer"),
    "norm: null ctl": ("norm", dict(ctl=None), "null pointer"),
    "norm: n 0": ("norm", dict(n=0), "n=0 must be positive"),
    "norm: n % 4": ("norm", dict(n=62), "multiple of 4"),
    "norm: grad alignment": ("norm", dict(grad=_P + 0x1004), "16-byte aligned"),
    "norm: tiles alignment": ("norm", dict(tiles=_P + 0x5008), "16-byte aligned"),
    "norm: state alignment": ("norm", dict(state=_P + 0x7008), "16-byte aligned"),
    "norm: ctl alignment": ("norm", dict(ctl=_P + 0x10008), "16-byte aligned"),
    "norm: tile table empty": ("norm", dict(ntiles=0), "tile table empty"),
    "norm: tile count negative": ("norm", dict(ntiles=-1), "tile table empty"),
    "norm: no segments": ("norm", dict(nseg=0), "nseg=0"),
    "norm: NaN max_norm": ("norm", dict(max_norm=float("nan")), "max_norm is NaN"),
    "norm: bc_len 0": ("norm", dict(bc_len=0), "bc_len=0 must be >= 1"),
    "norm: ctl overlaps grad": ("norm", dict(grad=_INSIDE), "ctl overlaps grad"),
    "norm: grad ends inside ctl": ("norm", dict(grad=_P + 0x10000 - 240), "ctl overlaps grad"),
    "norm: ctl overlaps the table": ("norm", dict(table=_INSIDE), "ctl overlaps bc_table"),
    "norm: ctl overlaps state": ("norm", dict(state=_INSIDE), "ctl overlaps state"),
    "norm: ctl overlaps hyper": ("norm", dict(hyper=_INSIDE), "ctl overlaps hyper"),
    "norm: ctl overlaps tiles": ("norm", dict(tiles=_INSIDE), "ctl overlaps tiles"),
    "norm: hyper is state": ("norm", dict(hyper=_P + 0x7000), "hyper overlaps state"),
    "norm: state overlaps grad": ("norm", dict(state=_P + 0x1000 + 240), "state overlaps grad"),
    "advance: null state": ("advance", dict(state=None), "null pointer"),
    "advance: null table": ("advance", dict(table=None), "null pointer"),
    "advance: no segments": ("advance", dict(nseg=-2), "nseg=-2"),
    "advance: ctl alignment": ("advance", dict(ctl=_P + 0x10004), "16-byte aligned"),
    "advance: ctl overlaps state": ("advance", dict(state=_INSIDE), "ctl overlaps state"),
    "adam: null param": ("adam", dict(param=None), "null pointer"),
    "adam: null exp_avg_sq": ("adam", dict(v=None), "null pointer"),
    "adam: null ctl": ("adam", dict(ctl=None), "null pointer"),
    "adam: null tiles": ("adam", dict(tiles=None), "null pointer"),
    "adam: n 0": ("adam", dict(n=0), "n=0 must be positive"),
    "adam: n % 4": ("adam", dict(n=62), "multiple of 4"),
    "adam: tile table empty": ("adam", dict(ntiles=0), "tile table empty"),
    "adam: exp_avg alignment": ("adam", dict(m=_P + 0x2004), "16-byte aligned"),
    "adam: ctl overlaps exp_avg": ("adam", dict(m=_INSIDE), "ctl overlaps exp_avg"),
    "adam: ctl overlaps param": ("adam", dict(param=_P + 0x10000), "ctl overlaps param"),
    "adam: hyper inside exp_avg_sq": ("adam", dict(hyper=_P + 0x3000 + 16), "hyper overlaps exp_avg_sq"),
    "adam: tiles inside param": ("adam", dict(tiles=_P + 0x10), "tiles overlap param"),
    "sgd: null grad": ("sgd", dict(grad=None), "null pointer"),
    "sgd: n % 4": ("sgd", dict(n=62), "multiple of 4"),
    "sgd: tile table empty": ("sgd", dict(ntiles=0), "tile table empty"),
    "sgd: momentum without a buffer": ("sgd", dict(m=None), "momentum buffer iff momentum != 0"),
    "sgd: a buffer without momentum": ("sgd", dict(momentum=0.0), "momentum buffer iff momentum != 0"),
    "sgd: param alignment": ("sgd", dict(param=_P + 8), "16-byte aligned"),
    "sgd: ctl overlaps the momentum buffer": ("sgd", dict(m=_INSIDE), "ctl overlaps momentum_buf"),
    "set: null state": ("set", dict(state=None), "null pointer"),
    "set: null counts": ("set", dict(counts=None), "null pointer"),
    "set: null table": ("set", dict(table=None), "null pointer"),
    "set: seg below range": ("set", dict(seg0=-1), "seg out of range"),
    "set: seg past range": ("set", dict(seg0=1), "seg out of range"),
    "set: seg far past range": ("set", dict(seg0=3, count=1), "seg out of range"),
    "set: no segments to set": ("set", dict(count=0), "seg out of range"),
    "set: state alignment": ("set", dict(state=_P + 0x7004), "aligned"),
    "set: bc_len 0": ("set", dict(bc_len=0), "bc_len=0"),
    "set: state overlaps counts": ("set", dict(counts=_P + 0x7010), "state overlaps applied"),
    "get: null state": ("get", dict(state=None), "null pointer"),
    "get: null out": ("get", dict(out=None), "null pointer"),
    "get: no segments": ("get", dict(nseg=0), "nseg=0"),
    "get: state alignment": ("get", dict(state=_P + 0x7008), "aligned"),
}
_ENTRY = dict(norm="ubg_grad_norm", advance="ubg_advance", adam="ubg_adam_step", sgd="ubg_sgd_step", set="ubg_state_set", get="ubg_state_get")


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    which, change, message = _BAD[name]
    a = dict(_A)
    a.update(change)
    lib = G.lib()
    if which == "norm":
        rc = lib.ubg_grad_norm(a["grad"], a["n"], a["tiles"], a["ntiles"], a["hyper"], a["state"], a["nseg"], 1.0, a["max_norm"], 1,
                               a["table"], a["bc_len"], a["ctl"], None)
    elif which == "advance":
        rc = lib.ubg_advance(a["hyper"], a["state"], a["nseg"], 1.0, a["table"], a["bc_len"], a["ctl"], None)
    elif which == "adam":
        rc = lib.ubg_adam_step(a["param"], a["grad"], a["m"], a["v"], a["n"], a["tiles"], a["ntiles"], a["hyper"], a["state"], a["nseg"],
                               0.9, 0.999, 1e-8, a["ctl"], None)
    elif which == "sgd":
        rc = lib.ubg_sgd_step(a["param"], a["grad"], a["m"], a["n"], a["tiles"], a["ntiles"], a["hyper"], a["state"], a["nseg"],
                              a["momentum"], 0.0, 0, a["ctl"], None)
    elif which == "set":
        rc = lib.ubg_state_set(a["state"], a["nseg"], a["seg0"], a["count"], a["counts"], a["table"], a["bc_len"], None)
    else:
        rc = lib.ubg_state_get(a["state"], a["nseg"], a["out"], None)
    msg = lib.ubg_last_error().decode()
    assert rc == -1 and msg.startswith(_ENTRY[which] + ":") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=_ENTRY[which]):
        G.check(rc, name)
    assert C.sizeof(C.c_void_p) == 8


# ------------------------------------------------------------------------------------------------------------------------
# the reference itself, by hand
# ------------------------------------------------------------------------------------------------------------------------
def test_ordered_sum_by_hand():
    # one tile of 2 units: lane 0 has unit 0, lane 1 unit 1; tree: s[0] + s[1] at the last round
    g = np.array([1, 2, 3, 4, 5, 6, 7, 8], np.float32)
    s, part = R.ordered_sumsq(g, R.plan_tiles([0], [2]), [True])
    assert s == 204.0 and part.tolist() == [204.0]
    s, _ = R.ordered_sumsq(g, R.plan_tiles([0, 1], [1, 1]), [False, True])
    assert s == 25 + 36 + 49 + 64
    # order matters and is the stated one (x, y, z, w of a unit in one accumulator): 2^54 absorbs each 1.0 that comes after
    # it; three that came before it are 3.0, and 2^54 + 3 rounds up
    g = np.zeros(8, np.float32)
    g[:4] = [2.0 ** 27, 1.0, 1.0, 1.0]
    c, _ = R.ordered_sumsq(g, R.plan_tiles([0], [2]), [True])
    g[:4] = [1.0, 1.0, 1.0, 2.0 ** 27]
    d, _ = R.ordered_sumsq(g, R.plan_tiles([0], [2]), [True])
    assert c == 2.0 ** 54 and d == 2.0 ** 54 + 4.0
    # a lane's units of one tile before the tree: unit 0 and unit 256 are both lane 0's
    g = np.zeros(4 * 257, np.float32)
    g[0], g[4], g[5], g[6], g[4 * 256] = 1.0, 1.0, 1.0, 1.0, 2.0 ** 27
    e, _ = R.ordered_sumsq(g, R.plan_tiles([0], [257]), [True])       # lane 0: 1 + 2^54 = 2^54; lane 1: 3; tree: 2^54 + 3
    assert e == 2.0 ** 54 + 4.0
    # more tiles than workgroups: tile MAX_GRID goes to workgroup 0 again
    n = R.MAX_GRID + 1
    g = np.ones(4 * n, np.float32)
    s, part = R.ordered_sumsq(g, R.plan_tiles(list(range(n)), [1] * n), [True] * n)
    assert s == 4.0 * n and part[0] == 8.0 and part[1] == 4.0 and len(part) == R.MAX_GRID


def test_decide_reference_by_hand():
    tab = _opt.bias_table(0.9, 0.999)
    st = R.new_state(3, [0, 5, 0], tab)
    assert st["segs"][1]["bc1"] == tab[4, 0] and st["segs"][0]["bc1"] == 0
    d = R.decide(9.0, 1.0, 6.0, True, st, [True, True, False], tab)                      # norm 3 under max_norm 6
    assert d["norm"] == 3.0 and d["scale"] == 1.0 and d["gscale"] == 1.0 and d["apply"] == 1 and d["clipped"] == 0 and d["applied"] == 1
    assert [s["applied"] for s in st["segs"]] == [1, 6, 0] and st["segs"][0]["bc1"] == tab[0, 0] and st["segs"][1]["sqrt_bc2"] == tab[5, 1]
    d = R.decide(16.0, -0.5, 1.0, True, st, [False, False, True], tab)                   # |grad_scale| in the norm, its sign in gscale
    assert d["norm"] == 2.0 and d["scale"] == np.float32(1.0) / (np.float32(2.0) + np.float32(1e-6)) and d["gscale"] == np.float32(-0.5) * d["scale"]
    assert d["clipped"] == 1 and d["clipped_total"] == 1 and d["applied"] == 2 and [s["applied"] for s in st["segs"]] == [1, 6, 1]
    for bad in (float("nan"), float("inf")):
        d = R.decide(bad, 1.0, 1.0, True, st, [True, True, True], tab)
        assert d["apply"] == 0 and d["clipped"] == 0 and d["applied"] == 2 and [s["applied"] for s in st["segs"]] == [1, 6, 1]
    assert st["skipped"] == 2
    d = R.decide(float("nan"), 1.0, None, False, st, [True, True, True], tab)            # not guarded: applies
    assert d["apply"] == 1 and d["scale"] == 1.0 and math.isnan(d["norm"]) and [s["applied"] for s in st["segs"]] == [2, 7, 2]
    st = R.new_state(1, [5], tab[:2])
    d = R.advance(0.25, st, [True], tab[:2])                                             # past the table's end: its last row
    assert (d["sumsq"], d["norm"], d["scale"], d["gscale"], d["apply"]) == (0.0, 0.0, 1.0, 0.25, 1)
    assert st["segs"][0]["applied"] == 6 and st["segs"][0]["bc1"] == tab[1, 0]


# ------------------------------------------------------------------------------------------------------------------------
# the optimizer's host side: split_decay, the group rules, torch's numbering
# ------------------------------------------------------------------------------------------------------------------------
def _optim():
    from ubresnet_amd import optim
    assert hasattr(optim, "split_decay"), "ubresnet_amd.optim has no parameter groups"
    return optim


def _net():
    from ubresnet_amd.models.ub_uresnet import UResNet
    return UResNet(num_classes=3, input_channels=1, inplanes=16)


def test_split_decay_separates_conv_weights_from_batchnorm_and_biases():
    optim = _optim()
    m = _net()
    decay, rest = optim.split_decay(m, 1e-3)
    assert decay["weight_decay"] == 1e-3 and rest["weight_decay"] == 0.0 and sorted(decay) == sorted(rest) == ["params", "weight_decay"]
    names = {id(p): n for n, p in m.named_parameters()}
    kinds = {}
    for mn, mod in m.named_modules():
        for pn, p in mod.named_parameters(recurse=False):
            base = [c for c in (torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.BatchNorm2d) if isinstance(mod, c)]
            assert len(base) == 1, "a parameter of %r" % type(mod)
            kinds[id(p)] = (base[0], pn)
    assert len(decay["params"]) + len(rest["params"]) == len(names) and not {id(p) for p in decay["params"]} & {id(p) for p in rest["params"]}
    for p in decay["params"]:
        assert kinds[id(p)][0] in (torch.nn.Conv2d, torch.nn.ConvTranspose2d) and kinds[id(p)][1] == "weight", names[id(p)]
    for p in rest["params"]:
        assert kinds[id(p)][1] == "bias" or kinds[id(p)][0] is torch.nn.BatchNorm2d, names[id(p)]
    assert any(kinds[id(p)] == (torch.nn.BatchNorm2d, "weight") for p in rest["params"])
    assert any(kinds[id(p)] == (torch.nn.ConvTranspose2d, "weight") for p in decay["params"])
    assert any(kinds[id(p)][0] is torch.nn.Conv2d and kinds[id(p)][1] == "bias" for p in rest["params"])
    order = [id(p) for p in m.parameters()]
    for grp in (decay, rest):
        idx = [order.index(id(p)) for p in grp["params"]]
        assert idx == sorted(idx)
    torch.optim.Adam([decay, rest], lr=1e-3)                            # torch accepts them as they are


def test_group_rules_are_value_errors():
    optim = _optim()
    m = _net()
    ps = list(m.parameters())
    defaults = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    ok = optim._check_groups(ps, [{"params": ps[:3], "lr": 1e-6}, {"params": ps[3:], "weight_decay": 0.1, "betas": [0.9, 0.999], "eps": 1e-8}], defaults)
    assert [len(g["params"]) for g in ok] == [3, len(ps) - 3] and ok[0]["lr"] == 1e-6 and "lr" not in ok[1]
    assert optim._check_groups(ps, [{"params": ps[0]}], defaults)[0]["params"] == [ps[0]]           # a model parameter in no group is allowed
    stranger = torch.nn.Parameter(torch.zeros(3))
    for bad, message in (([{"params": ps[:3]}, {"params": ps[2:]}], "already in a group"),
                         ([{"params": ps[:3] + [ps[0]]}], "already in a group"),
                         ([{"params": ps + [stranger]}], "does not belong to the model"),
                         ([{"params": ps, "betas": (0.8, 0.999)}], "optimizer-wide"),
                         ([{"params": ps, "eps": 1e-6}], "optimizer-wide"),
                         ([{"params": ps, "amsgrad": True}], "not a hyper-parameter"),
                         ([{"lr": 1.0}], "no \"params\""),
                         ([], "non-empty list"),
                         ({"params": ps}, "non-empty list")):
        with pytest.raises(ValueError, match=message):
            optim._check_groups(ps, bad, defaults)
    sgd = dict(lr=1e-3, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False)
    for key, val in (("momentum", 0.5), ("dampening", 0.1), ("nesterov", True)):
        with pytest.raises(ValueError, match="optimizer-wide"):
            optim._check_groups(ps, [{"params": ps, key: val}], sgd)
    # the constructors take the argument (and refuse a model that is not on the device before anything else)
    with pytest.raises(RuntimeError, match="float32 on one ROCm device"):
        optim.FlatAdam(m, groups=[{"params": ps}])
    with pytest.raises(RuntimeError, match="float32 on one ROCm device"):
        optim.FlatSGD(m, groups=optim.split_decay(m, 1e-3))


class _Counts(object):
    """stands in for the device side: step counts per segment, no launch"""

    def __init__(self, counts):
        self._c, self.nseg = np.asarray(counts, np.int64), len(counts)

    def counts(self):
        return self._c


def _stand_in(cls, m, groups, defaults, counts, **buffers):
    """a grouped optimizer on the CPU as far as state_dict() goes: torch's own constructor, the layout of four parameters in
    REVERSE model order (the gradient layout is not model.parameters() order either), flat state buffers, counts by hand"""
    optim = _optim()
    opt = object.__new__(cls)
    torch.optim.Optimizer.__init__(opt, optim._check_groups(list(m.parameters()), groups, defaults), defaults)
    layout, off = [], 0
    for n, p in reversed(list(m.named_parameters())[:4]):
        layout.append((n, p, off))
        off += (p.numel() + 3) // 4 * 4
    opt._layout, opt._numel = layout, off
    opt._index = {id(p): i for i, p in enumerate(p for g in opt.param_groups for p in g["params"])}
    opt._grouped = _Counts(counts)
    opt.steps = max(counts)
    for k, fill in buffers.items():
        setattr(opt, k, None if fill is None else torch.arange(off, dtype=torch.float32) + fill)
    return opt


def test_state_dict_numbering_and_layout_are_torchs():
    optim = _optim()
    m = _net()
    named = list(m.named_parameters())[:4]
    ps = [p for _, p in named]
    # groups in an order that is neither the model's nor the layout's; ps[2] is in no group
    groups = [{"params": [ps[3], ps[0]], "lr": 1e-6}, {"params": [ps[1]], "weight_decay": 0.5}]
    defaults = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    # layout order is ps[3], ps[2], ps[1], ps[0]; counts by segment: ps[3] 3 steps, ps[2] (no group) 0, ps[1] 0 (never stepped), ps[0] 1
    opt = _stand_in(optim.FlatAdam, m, groups, defaults, [3, 0, 0, 1], exp_avg=1000.0, exp_avg_sq=2000.0)
    sd = opt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1], [2]]
    assert [(g["lr"], g["weight_decay"]) for g in sd["param_groups"]] == [(1e-6, 1e-4), (1e-3, 0.5)]
    assert all(g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 for g in sd["param_groups"])
    assert sorted(sd["state"]) == [0, 1], "no entry for a parameter that never stepped, none for one in no group"
    assert sd["state"][0]["step"].item() == 3.0 and sd["state"][1]["step"].item() == 1.0          # number 0 is ps[3], number 1 is ps[0]
    off = {id(p): o for _, p, o in opt._layout}
    for i, p in ((0, ps[3]), (1, ps[0])):
        e = sd["state"][i]
        assert sorted(e) == ["exp_avg", "exp_avg_sq", "step"] and e["exp_avg"].shape == p.shape
        assert torch.equal(e["exp_avg"].reshape(-1), torch.arange(off[id(p)], off[id(p)] + p.numel(), dtype=torch.float32) + 1000.0)
        assert torch.equal(e["exp_avg_sq"].reshape(-1), torch.arange(off[id(p)], off[id(p)] + p.numel(), dtype=torch.float32) + 2000.0)
        assert e["exp_avg"].data_ptr() != opt.exp_avg.data_ptr() + 4 * off[id(p)], "a clone, not a view"
    # torch.optim.Adam on the same grouping takes it, and gives the same layout back
    ref = torch.optim.Adam([dict(g) for g in groups], **defaults)
    ref.load_state_dict(sd)
    back = ref.state_dict()
    assert [g["params"] for g in back["param_groups"]] == [[0, 1], [2]] and sorted(back["state"]) == [0, 1]
    assert float(back["state"][0]["step"]) == 3.0 and torch.equal(back["state"][1]["exp_avg"], sd["state"][1]["exp_avg"])
    assert [(g["lr"], g["weight_decay"]) for g in back["param_groups"]] == [(1e-6, 1e-4), (1e-3, 0.5)]
    # SGD: momentum buffers of the parameters that stepped; none without momentum
    sgd = dict(lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False)
    opt = _stand_in(optim.FlatSGD, m, groups, sgd, [2, 0, 0, 0], momentum_buffer=500.0)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0] and sorted(sd["state"][0]) == ["momentum_buffer"] and [g["params"] for g in sd["param_groups"]] == [[0, 1], [2]]
    ref = torch.optim.SGD([dict(g) for g in groups], **sgd)
    ref.load_state_dict(sd)
    assert torch.equal(ref.state_dict()["state"][0]["momentum_buffer"], sd["state"][0]["momentum_buffer"])
    opt = _stand_in(optim.FlatSGD, m, groups, dict(sgd, momentum=0.0), [2, 0, 0, 1], momentum_buffer=None)
    assert opt.state_dict()["state"] == {}
