"""The parameter-averaging library without a GPU: libubresnet_ema.so's header is C99; header, binding, reference and library agree on
the entry points, the geometry and the control block; every argument refusal returns UBE_EINVAL with a message before any launch;
the schedule (a host/device inline function) as a stand-alone program under the host sanitizers against ema_ref bit for bit;
ParamEMA's own refusals."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ema_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_ema.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib  # noqa: E402
from ubresnet_amd import _ema as E  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402

LIB = B.LIBS["ema"].out


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99_and_fixes_the_layout(tmp_path):
    proto, src, exe = tmp_path / "p.c", tmp_path / "t.c", tmp_path / "t"
    proto.write_text('#include "ubresnet_ema.h"\n'
                     'int main(void) {\n'
                     '  int (*i)(void*, int64_t, void*) = ube_ctl_init;\n'
                     '  int (*a)(void*, const int32_t*, float, int64_t, void*) = ube_advance;\n'
                     '  int (*u)(float*, const float*, int64_t, const void*, void*) = ube_update;\n'
                     '  int (*s)(float*, float*, int64_t, void*) = ube_swap;\n'
                     '  int (*us)(const void*, int64_t, const void*, void*) = ube_update_segs;\n'
                     '  int (*ss)(const void*, int64_t, void*) = ube_swap_segs;\n'
                     '  return i == 0 || a == 0 || u == 0 || s == 0 || us == 0 || ss == 0 || UBE_OK != 0 || UBE_EINVAL != -1;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ubresnet_ema.h"\n'
                   'int main(void) {\n'
                   '  printf("ctl %d %d %d %d %d %d %d\\n", (int)sizeof(ube_ctl), (int)offsetof(ube_ctl, apply), (int)offsetof(ube_ctl, w),\n'
                   '         (int)offsetof(ube_ctl, d), (int)offsetof(ube_ctl, reserved), (int)offsetof(ube_ctl, updates), (int)offsetof(ube_ctl, held));\n'
                   '  printf("seg %d %d %d %d\\n", (int)sizeof(ube_seg), (int)offsetof(ube_seg, shadow), (int)offsetof(ube_seg, live), (int)offsetof(ube_seg, count));\n'
                   '  return 0;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().split("\n")}
    assert out["ctl"] == [R.CTL_BYTES] + [R.OFFSETS[k] for k in ("apply", "w", "d", "reserved", "updates", "held")]
    assert out["seg"] == [E.SEG.itemsize] + [E.SEG.fields[k][1] for k in ("shadow", "live", "count")] == [32, 0, 8, 16]
    assert C.sizeof(E.Ctl) == E.CTL_BYTES == R.CTL_BYTES == 32
    assert {n: getattr(E.Ctl, n).offset for n, _ in E.Ctl._fields_} == R.OFFSETS
    h = E.read_ctl(np.arange(48, dtype=np.uint8).tobytes())
    assert h.apply == int.from_bytes(bytes(range(0, 4)), "little") and h.held == int.from_bytes(bytes(range(24, 32)), "little")


def test_the_apply_flag_is_byte_20_of_both_optimizer_blocks():
    from ubresnet_amd import _group, _opt
    assert _opt.Ctl.apply.offset == _group.Ctl.apply.offset == E.APPLY_OFFSET == R.APPLY_OFFSET == 20
    assert _opt.Ctl.apply.size == 4


def test_header_binding_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ube_[a-z_0-9]+)\s*\(", text))
    need_lib(LIB)
    assert declared == set(E.SYMBOLS) and len(E.SYMBOLS) == len(set(E.SYMBOLS))
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBE_(BLOCK|UNROLL|MAX_GRID|SEG_GRID|CTL_BYTES)\s+(\d+)", text)}
    assert geometry == dict(BLOCK=E.BLOCK, UNROLL=E.UNROLL, MAX_GRID=E.MAX_GRID, SEG_GRID=E.SEG_GRID, CTL_BYTES=E.CTL_BYTES)
    assert geometry == dict(BLOCK=R.BLOCK, UNROLL=R.UNROLL, MAX_GRID=R.MAX_GRID, SEG_GRID=R.SEG_GRID, CTL_BYTES=R.CTL_BYTES)
    # six kernels, and nothing of them in the network library
    assert sorted(k.split("(")[0].split("::")[-1] for k in kernel_symbols.kernels(LIB)) == [
        "advance_kernel", "ctl_init_kernel", "swap_kernel", "swap_segs_kernel", "update_kernel", "update_segs_kernel"]


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------------------------------
# addresses that are never dereferenced: every call below is refused on the host, before any launch.  n = 64 floats (256 bytes)
_P = 0x100000
_A = dict(shadow=_P, param=_P + 0x1000, ctl=_P + 0x2000, flag=_P + 0x3000 + 20, table=_P + 0x4000, n=64, nseg=3, decay=0.999, warmup=10,
          updates=0)
_BAD = {
    "init: null ctl": ("init", dict(ctl=None), "null ctl"),
    "init: ctl alignment": ("init", dict(ctl=_P + 0x2008), "16-byte aligned"),
    "init: negative count": ("init", dict(updates=-1), "updates=-1"),
    "advance: null ctl": ("advance", dict(ctl=None), "null ctl"),
    "advance: ctl alignment": ("advance", dict(ctl=_P + 0x2004), "16-byte aligned"),
    "advance: flag alignment": ("advance", dict(flag=_P + 0x3000 + 21), "4-byte aligned"),
    "advance: flag inside ctl": ("advance", dict(flag=_P + 0x2000 + 16), "inside ctl"),
    "advance: decay 1": ("advance", dict(decay=1.0), "must lie in [0, 1)"),
    "advance: decay above 1": ("advance", dict(decay=1.5), "must lie in [0, 1)"),
    "advance: decay negative": ("advance", dict(decay=-0.25), "must lie in [0, 1)"),
    "advance: decay NaN": ("advance", dict(decay=float("nan")), "decay is NaN"),
    "advance: decay inf": ("advance", dict(decay=float("inf")), "must lie in [0, 1)"),
    "advance: warmup negative": ("advance", dict(warmup=-1), "warmup=-1"),
    "update: null shadow": ("update", dict(shadow=None), "null pointer"),
    "update: null param": ("update", dict(param=None), "null pointer"),
    "update: null ctl": ("update", dict(ctl=None), "null pointer"),
    "update: n 0": ("update", dict(n=0), "n=0 must be positive"),
    "update: n negative": ("update", dict(n=-4), "n=-4 must be positive"),
    "update: n % 4": ("update", dict(n=62), "multiple of 4"),
    "update: shadow alignment": ("update", dict(shadow=_P + 4), "16-byte aligned"),
    "update: param alignment": ("update", dict(param=_P + 0x1008), "16-byte aligned"),
    "update: ctl alignment": ("update", dict(ctl=_P + 0x2008), "16-byte aligned"),
    "update: shadow is param": ("update", dict(param=_P), "shadow overlaps param"),
    "update: param starts inside shadow": ("update", dict(param=_P + 240), "shadow overlaps param"),
    "update: ctl inside shadow": ("update", dict(ctl=_P + 16), "ctl overlaps shadow"),
    "update: param ends inside ctl": ("update", dict(param=_P + 0x2000 - 240), "ctl overlaps param"),
    "swap: null a": ("swap", dict(shadow=None), "null pointer"),
    "swap: null b": ("swap", dict(param=None), "null pointer"),
    "swap: n 0": ("swap", dict(n=0), "n=0 must be positive"),
    "swap: n % 4": ("swap", dict(n=6), "multiple of 4"),
    "swap: a alignment": ("swap", dict(shadow=_P + 8), "16-byte aligned"),
    "swap: b alignment": ("swap", dict(param=_P + 0x1004), "16-byte aligned"),
    "swap: a overlaps b": ("swap", dict(param=_P + 16), "a overlaps b"),
    "update_segs: null table": ("update_segs", dict(table=None), "null pointer"),
    "update_segs: null ctl": ("update_segs", dict(ctl=None), "null pointer"),
    "update_segs: no rows": ("update_segs", dict(nseg=0), "nseg=0"),
    "update_segs: negative rows": ("update_segs", dict(nseg=-3), "nseg=-3"),
    "update_segs: table alignment": ("update_segs", dict(table=_P + 0x4004), "aligned"),
    "update_segs: ctl inside the table": ("update_segs", dict(ctl=_P + 0x4000 + 32), "ctl overlaps table"),
    "swap_segs: null table": ("swap_segs", dict(table=None), "null pointer"),
    "swap_segs: no rows": ("swap_segs", dict(nseg=0), "nseg=0"),
    "swap_segs: table alignment": ("swap_segs", dict(table=_P + 0x4002), "aligned"),
}
_ENTRY = dict(init="ube_ctl_init", advance="ube_advance", update="ube_update", swap="ube_swap", update_segs="ube_update_segs",
              swap_segs="ube_swap_segs")


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    which, change, message = _BAD[name]
    a = dict(_A)
    a.update(change)
    lib = E.lib()
    if which == "init":
        rc = lib.ube_ctl_init(a["ctl"], a["updates"], None)
    elif which == "advance":
        rc = lib.ube_advance(a["ctl"], a["flag"], a["decay"], a["warmup"], None)
    elif which == "update":
        rc = lib.ube_update(a["shadow"], a["param"], a["n"], a["ctl"], None)
    elif which == "swap":
        rc = lib.ube_swap(a["shadow"], a["param"], a["n"], None)
    elif which == "update_segs":
        rc = lib.ube_update_segs(a["table"], a["nseg"], a["ctl"], None)
    else:
        rc = lib.ube_swap_segs(a["table"], a["nseg"], None)
    msg = lib.ube_last_error().decode()
    assert rc == -1 and msg.startswith(_ENTRY[which] + ":") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=_ENTRY[which]):
        E.check(rc, name)


# ------------------------------------------------------------------------------------------------------------------------
# the schedule
# ------------------------------------------------------------------------------------------------------------------------
def test_reference_schedule_by_hand():
    f32 = np.float32
    assert R.schedule(0.5, 0, 0) == (f32(0.5), f32(0.5)) and R.schedule(0.5, 1, 7) == (f32(0.5), f32(0.5))
    assert R.schedule(0.999, 10, 0) == (f32(0.9), f32(0.1))                       # (1 + 0) / (10 + 0)
    assert R.schedule(0.999, 10, 2) == (f32(0.75), f32(0.25))                     # 3 / 12
    assert R.schedule(0.0, 10, 5) == (f32(1.0), f32(0.0))                         # decay 0: the average is the last value
    big = R.schedule(0.999, 10, 10 ** 6)
    assert big == (f32(1.0 - float(f32(0.999))), f32(0.999))
    assert R.crossover(0.5, 10) == 8 and R.crossover(0.5, 0) is None and R.crossover(0.0, 10) == 0
    u = R.crossover(0.999, 10)
    assert 8980 < u < 9000 and R.schedule(0.999, 10, u)[1] == f32(0.999) and (1.0 + (u - 1)) / (10 + (u - 1)) < float(f32(0.999))
    c = R.Ctl(3)
    assert c.advance(0, 0.999, 10) == 0 and (c.updates, c.held) == (3, 1)
    assert c.advance(None, 0.999, 10) == 1 and (c.updates, c.held, c.d) == (4, 1, f32(4.0 / 13.0))
    assert c.advance(5, 0.999, 10) == 1 and c.updates == 5
    s, p = f32([1.0, -0.0, 1e-45]), f32([3.0, -0.0, 1e-45])
    got = R.update(s, p, f32(0.25))
    assert got.dtype == f32 and got.view(np.uint32).tolist() == [0x3fc00000, 0, 1]     # (-0) + 0.25 * ((-0) - (-0)) = (-0) + (+0) = +0


def test_schedule_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/ema_host.cpp has its own main and includes the schedule's header; built with -fsanitize=address,undefined and run as
    a process of its own; (w, d) bit for bit against ema_ref for u = 0 .. 2000 and around the u where the minimum changes sides"""
    exe = str(tmp_path / "ema_host")
    r = subprocess.run([cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-ffp-contract=off", "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "ema_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(decay, warmup, u0, u1):
        bits = int(np.float32(decay).view(np.uint32))
        p = subprocess.run([exe, "%08x" % bits, str(warmup), str(u0), str(u1)], capture_output=True, text=True)
        assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
        rows = [l.split() for l in p.stdout.strip().split("\n")]
        assert [int(x[0]) for x in rows] == list(range(u0, u1))
        return [(int(x[1], 16), int(x[2], 16)) for x in rows]

    def want(decay, warmup, u0, u1):
        return [tuple(int(v.view(np.uint32)) for v in R.schedule(decay, warmup, u)) for u in range(u0, u1)]
    sides = 0
    for warmup in (0, 2, 10):
        for decay in (0.0, 0.5, 0.999, 0.9999):
            assert run(decay, warmup, 0, 2001) == want(decay, warmup, 0, 2001), (decay, warmup)
            x = R.crossover(decay, warmup)
            if x is not None and x > 0:
                lo = max(x - 8, 0)
                assert run(decay, warmup, lo, x + 8) == want(decay, warmup, lo, x + 8), (decay, warmup, x)
                d32 = float(np.float32(decay))
                assert (1.0 + (x - 1)) / (warmup + (x - 1)) < d32 <= (1.0 + x) / (warmup + x)
                sides += 1
    assert sides == 5                    # decay 0.5, 0.999, 0.9999 at warmup 2 and 10, but for 0.5 at 2: that ramp starts at 1 / 2


# ------------------------------------------------------------------------------------------------------------------------
# ParamEMA
# ------------------------------------------------------------------------------------------------------------------------
def test_param_ema_refuses_what_is_not_a_flat_optimizer():
    from ubresnet_amd.ema import ParamEMA
    lin = torch.nn.Linear(3, 2)
    with pytest.raises(TypeError, match="FlatAdam or FlatSGD"):
        ParamEMA(torch.optim.Adam(lin.parameters(), lr=1e-3))
    with pytest.raises(TypeError, match="FlatAdam or FlatSGD"):
        ParamEMA(lin)


def test_the_wiring_is_keyword_arguments_with_todays_defaults():
    import inspect
    from ubresnet_amd import deploy
    from ubresnet_amd.training import epoch
    for fn, default in ((epoch.train, None), (epoch.validate, None), (deploy.load_model, False)):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "ema" and p["ema"].default is default, fn.__name__
    with pytest.raises(KeyError, match="ema"):
        deploy.load_model(None, "cpu", num_classes=3, state_dict={}, ema=True)
