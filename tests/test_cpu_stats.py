"""The running-statistics guard without a GPU: libubresnet_stats.so's header is C99; header, binding, reference and library agree on
the entry points, the geometry, the control block and the row; every argument refusal returns UBS_EINVAL with a message before any
launch; the decision rule (a host/device inline function) as a stand-alone program under the host sanitizers against stats_ref
over its whole truth table; the table builder on a CPU stand-in model; StatsGuard's own refusals; the wiring into the epoch loop."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import stats_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_stats.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib  # noqa: E402
from ubresnet_amd import _stats as S  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402

LIB = B.LIBS["stats"].out


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99_and_fixes_the_layout(tmp_path):
    proto, src, exe = tmp_path / "p.c", tmp_path / "t.c", tmp_path / "t"
    proto.write_text('#include "ubresnet_stats.h"\n'
                     'int main(void) {\n'
                     '  int (*i)(void*, void*) = ubs_ctl_init;\n'
                     '  int (*s)(const void*, int64_t, int32_t*, void*) = ubs_scan;\n'
                     '  int (*n)(int32_t*, const int32_t*, int64_t, void*) = ubs_note;\n'
                     '  int (*d)(void*, const int32_t*, int64_t, const int32_t*, int32_t, void*) = ubs_decide;\n'
                     '  int (*r)(const void*, int64_t, const void*, void*) = ubs_resolve;\n'
                     '  return i == 0 || s == 0 || n == 0 || d == 0 || r == 0 || UBS_OK != 0 || UBS_EINVAL != -1;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ubresnet_stats.h"\n'
                   'int main(void) {\n'
                   '  printf("ctl %d %d %d %d %d %d\\n", (int)sizeof(ubs_ctl), (int)offsetof(ubs_ctl, keep), (int)offsetof(ubs_ctl, bad_rows),\n'
                   '         (int)offsetof(ubs_ctl, kept), (int)offsetof(ubs_ctl, restored), (int)offsetof(ubs_ctl, restored_for_stats));\n'
                   '  printf("seg %d %d %d %d %d\\n", (int)sizeof(ubs_seg), (int)offsetof(ubs_seg, shadow), (int)offsetof(ubs_seg, live),\n'
                   '         (int)offsetof(ubs_seg, count), (int)offsetof(ubs_seg, kind));\n'
                   '  printf("kind %d %d\\n", UBS_KIND_F32, UBS_KIND_RAW);\n'
                   '  return 0;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().split("\n")}
    names = ("keep", "bad_rows", "kept", "restored", "restored_for_stats")
    assert out["ctl"] == [R.CTL_BYTES] + [R.OFFSETS[k] for k in names]
    assert out["seg"] == [S.SEG.itemsize] + [S.SEG.fields[k][1] for k in ("shadow", "live", "count", "kind")] == [32, 0, 8, 16, 24]
    assert out["kind"] == [S.KIND_F32, S.KIND_RAW] == [R.KIND_F32, R.KIND_RAW] == [0, 1]
    assert C.sizeof(S.Ctl) == S.CTL_BYTES == R.CTL_BYTES == S.CTL.itemsize == 32
    assert {n: getattr(S.Ctl, n).offset for n, _ in S.Ctl._fields_} == R.OFFSETS == {n: S.CTL.fields[n][1] for n in names}
    h = S.read_ctl(np.arange(48, dtype=np.uint8).tobytes())
    assert h.keep == int.from_bytes(bytes(range(0, 4)), "little") and h.restored_for_stats == int.from_bytes(bytes(range(24, 32)), "little")
    t = S.seg_table([16, 32], [48, 64], [5, 2], [0, 1])
    assert t.tobytes() == np.array([16, 48, 5, 0, 32, 64, 2, 1], dtype="<i8").tobytes()


def test_the_apply_flag_is_the_one_ube_advance_takes():
    from ubresnet_amd import _ema, _group, _opt
    assert _opt.Ctl.apply.offset == _group.Ctl.apply.offset == _ema.APPLY_OFFSET == R.APPLY_OFFSET == 20


def test_header_binding_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ubs_[a-z_0-9]+)\s*\(", text))
    need_lib(LIB)
    assert declared == set(S.SYMBOLS) and len(S.SYMBOLS) == len(set(S.SYMBOLS))
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBS_(BLOCK|SEG_GRID|CTL_BYTES)\s+(\d+)", text)}
    assert geometry == dict(BLOCK=S.BLOCK, SEG_GRID=S.SEG_GRID, CTL_BYTES=S.CTL_BYTES)
    assert geometry == dict(BLOCK=R.BLOCK, SEG_GRID=R.SEG_GRID, CTL_BYTES=R.CTL_BYTES)
    # five kernels
    assert sorted(k.split("(")[0].split("::")[-1] for k in kernel_symbols.kernels(LIB)) == [
        "ctl_init_kernel", "decide_kernel", "note_kernel", "resolve_kernel", "scan_kernel"]


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------------------------------
# addresses that are never dereferenced: every call below is refused on the host, before any launch.  3 rows: a table of 96 bytes
_P = 0x100000
_A = dict(table=_P, bad=_P + 0x1000, seen=_P + 0x1800, ctl=_P + 0x2000, flag=_P + 0x3000 + 20, nseg=3, check=1)
_BAD = {
    "init: null ctl": ("init", dict(ctl=None), "null ctl"),
    "init: ctl alignment": ("init", dict(ctl=_P + 0x2008), "16-byte aligned"),
    "scan: null table": ("scan", dict(table=None), "null pointer"),
    "scan: null bad": ("scan", dict(bad=None), "null pointer"),
    "scan: no rows": ("scan", dict(nseg=0), "nseg=0"),
    "scan: negative rows": ("scan", dict(nseg=-3), "nseg=-3"),
    "scan: table alignment": ("scan", dict(table=_P + 4), "aligned"),
    "scan: bad alignment": ("scan", dict(bad=_P + 0x1002), "aligned"),
    "scan: bad inside the table": ("scan", dict(bad=_P + 64), "bad overlaps table"),
    "scan: bad ends inside the table": ("scan", dict(bad=_P - 8), "bad overlaps table"),
    "note: null seen": ("note", dict(seen=None), "null pointer"),
    "note: null bad": ("note", dict(bad=None), "null pointer"),
    "note: no rows": ("note", dict(nseg=0), "nseg=0"),
    "note: seen alignment": ("note", dict(seen=_P + 0x1801), "4-byte aligned"),
    "note: seen is bad": ("note", dict(seen=_P + 0x1000), "seen overlaps bad"),
    "note: seen starts inside bad": ("note", dict(seen=_P + 0x1008), "seen overlaps bad"),
    "decide: null ctl": ("decide", dict(ctl=None), "null pointer"),
    "decide: null bad": ("decide", dict(bad=None), "null pointer"),
    "decide: no rows": ("decide", dict(nseg=0), "nseg=0"),
    "decide: negative rows": ("decide", dict(nseg=-1), "nseg=-1"),
    "decide: ctl alignment": ("decide", dict(ctl=_P + 0x2004), "16-byte aligned"),
    "decide: bad alignment": ("decide", dict(bad=_P + 0x1001), "4-byte aligned"),
    "decide: flag alignment": ("decide", dict(flag=_P + 0x3000 + 21), "4-byte aligned"),
    "decide: flag inside ctl": ("decide", dict(flag=_P + 0x2000 + 16), "inside ctl"),
    "decide: bad inside ctl": ("decide", dict(bad=_P + 0x2000 + 24), "ctl overlaps bad"),
    "decide: flag inside bad": ("decide", dict(flag=_P + 0x1000 + 8), "inside bad"),
    "resolve: null table": ("resolve", dict(table=None), "null pointer"),
    "resolve: null ctl": ("resolve", dict(ctl=None), "null pointer"),
    "resolve: no rows": ("resolve", dict(nseg=0), "nseg=0"),
    "resolve: negative rows": ("resolve", dict(nseg=-3), "nseg=-3"),
    "resolve: table alignment": ("resolve", dict(table=_P + 4), "aligned"),
    "resolve: ctl alignment": ("resolve", dict(ctl=_P + 0x2008), "aligned"),
    "resolve: ctl inside the table": ("resolve", dict(ctl=_P + 32), "ctl overlaps table"),
    "resolve: ctl ends inside the table": ("resolve", dict(ctl=_P - 16), "ctl overlaps table"),
}
_ENTRY = dict(init="ubs_ctl_init", scan="ubs_scan", note="ubs_note", decide="ubs_decide", resolve="ubs_resolve")


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    which, change, message = _BAD[name]
    a = dict(_A)
    a.update(change)
    lib = S.lib()
    if which == "init":
        rc = lib.ubs_ctl_init(a["ctl"], None)
    elif which == "scan":
        rc = lib.ubs_scan(a["table"], a["nseg"], a["bad"], None)
    elif which == "note":
        rc = lib.ubs_note(a["seen"], a["bad"], a["nseg"], None)
    elif which == "decide":
        rc = lib.ubs_decide(a["ctl"], a["bad"], a["nseg"], a["flag"], a["check"], None)
    else:
        rc = lib.ubs_resolve(a["table"], a["nseg"], a["ctl"], None)
    msg = lib.ubs_last_error().decode()
    assert rc == -1 and msg.startswith(_ENTRY[which] + ":") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=_ENTRY[which]):
        S.check(rc, name)


# ------------------------------------------------------------------------------------------------------------------------
# the decision rule
# ------------------------------------------------------------------------------------------------------------------------
TRUTH = list(itertools.product((None, 0, 1), (0, 1), (0, 1, 3)))         # flag x check x bad_rows


def test_reference_rule_by_hand():
    assert R.decide(None, 1, 0) == (1, 0) and R.decide(1, 1, 0) == (1, 0) and R.decide(-7, 0, 3) == (1, 0)
    assert R.decide(0, 1, 0) == (0, 0) and R.decide(0, 0, 3) == (0, 0) and R.decide(0, 1, 3) == (0, 0)     # the optimizer's flag alone
    assert R.decide(None, 1, 1) == (0, 1) and R.decide(1, 1, 3) == (0, 1)                                   # the scan alone
    assert R.decide(None, 0, 3) == (1, 0)                                                                   # check off: never
    assert sum(R.decide(*t)[0] for t in TRUTH) == 8 and sum(R.decide(*t)[1] for t in TRUTH) == 4
    c = R.Ctl()
    assert c.decide([0, 0, 0], 1, 1) == 1 and c.decide([0, 2, 0], 1, 1) == 0 and c.decide([1, 0, -1], 0, 1) == 0
    assert c.fields() == (0, 2, 1, 2, 1)
    live = np.array([0x7f800000, 0xff800001, 0x7f7fffff, 0x00000001, 0x80000000, 0x7fc00000, 0xffffffff], dtype=np.uint32)
    assert R.scan(live, [(0, 0, 4, 0), (0, 4, 3, 0), (0, 4, 3, 1), (0, 0, 0, 0), (0, 2, 3, 0)]).tolist() == [2, 2, 0, 0, 0]
    assert R.note(np.array([1, 0x7ffffffe, 5], np.int32), np.array([2, 7, 0], np.int32)).tolist() == [3, 0x7fffffff, 5]


def test_decision_rule_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/stats_host.cpp has its own main and includes the rule's header; built with -fsanitize=address,undefined and run as a
    process of its own: the full truth table of (flag NULL / 0 / 1) x (check 0 / 1) x (bad_rows 0 / 1 / 3), each alone on a fresh
    block and all in one sequence on one block, against stats_ref"""
    exe = str(tmp_path / "stats_host")
    r = subprocess.run([cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "stats_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(cases):
        args = [x for flag, check, bad in cases for x in ("null" if flag is None else str(flag), str(check), str(bad))]
        p = subprocess.run([exe] + args, capture_output=True, text=True)
        assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
        rows = [l.replace("|", " ").split() for l in p.stdout.strip().split("\n")]
        assert len(rows) == len(cases)
        return [tuple(int(v) for v in row) for row in rows]

    def want(cases):
        c, out = R.Ctl(), []
        for flag, check, bad in cases:
            verdict = R.decide(flag, check, bad)
            c.decide([1] * bad + [0], flag, check)
            out.append(verdict + c.fields())
        return out
    assert len(TRUTH) == 18
    for case in TRUTH:
        assert run([case]) == want([case]), case
    whole = run(TRUTH)
    assert whole == want(TRUTH)
    assert whole[-1][4:] == (8, 10, 4)                       # kept, restored, restored_for_stats over the whole table
    assert run([(-5, 1, 0), (1 << 30, 0, 3)]) == want([(-5, 1, 0), (1 << 30, 0, 3)])      # any non-zero flag is "applied"


# ------------------------------------------------------------------------------------------------------------------------
# the Python side
# ------------------------------------------------------------------------------------------------------------------------
class _StandIn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 4, 3)
        self.bn1 = torch.nn.BatchNorm2d(4)
        self.block = torch.nn.Sequential(torch.nn.Conv2d(4, 6, 1), torch.nn.BatchNorm2d(6), torch.nn.ReLU())
        self.register_buffer("scale", torch.ones(3))          # a buffer that is no BatchNorm's: not guarded
        self.bn_free = torch.nn.BatchNorm2d(5, track_running_stats=False)


def test_table_builder_on_a_cpu_stand_in_model():
    from ubresnet_amd import bnguard
    m = _StandIn()
    rows = bnguard.stat_rows(m)
    names = [n for n, _, _, _ in rows]
    assert names == ["bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked",
                     "block.1.running_mean", "block.1.running_var", "block.1.num_batches_tracked"]
    assert names == [k for k in m.state_dict() if k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked")]
    assert [(k, c) for _, _, k, c in rows] == [(0, 4), (0, 4), (1, 2), (0, 6), (0, 6), (1, 2)]
    assert all(b is dict(m.named_buffers())[n] for n, b, _, _ in rows)
    t, offs, total = bnguard.stat_table(rows, 0x4000)
    assert t.dtype == S.SEG and offs == [0, 4, 8, 10, 16, 22] and total == 24
    assert t["shadow"].tolist() == [0x4000 + 4 * o for o in offs] and t["live"].tolist() == [b.data_ptr() for _, b, _, _ in rows]
    assert t["count"].tolist() == [4, 4, 2, 6, 6, 2] and t["kind"].tolist() == [0, 0, 1, 0, 0, 1]
    m.bn1.double()
    with pytest.raises(RuntimeError, match="bn1.running_mean must be float32"):
        bnguard.stat_rows(m)


def test_stats_guard_refuses_what_it_cannot_work_with():
    from ubresnet_amd.bnguard import StatsGuard
    m = _StandIn()
    with pytest.raises(TypeError, match="FlatAdam or FlatSGD"):
        StatsGuard(m, optimizer=torch.optim.Adam(m.parameters(), lr=1e-3))
    with pytest.raises(ValueError, match="could never restore"):
        StatsGuard(m, optimizer=None, check_nonfinite=False)
    with pytest.raises(ValueError, match="no BatchNorm buffers"):
        StatsGuard(torch.nn.Linear(3, 2))


def test_the_wiring_is_a_keyword_argument_with_todays_default():
    import inspect
    from ubresnet_amd.training import epoch
    p = inspect.signature(epoch.train).parameters
    assert p["stats_guard"].default is None and list(p)[-2:] == ["stats_guard", "ema"]
    assert "stats_guard" not in inspect.signature(epoch.validate).parameters
    rec = epoch._EpochRecord(4, 3)
    assert rec.stats is None and "BNRestored" not in rec.tail()
    soak = open(os.path.join(REPO, "tools", "soak.py")).read()
    assert "--stats-guard" in soak
