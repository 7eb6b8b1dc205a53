"""Detector effects without a GPU: libubresnet_det.so's header is C99; header, binding, reference and library agree on the entry
points and the geometry; the compiled kernels are exactly those the case table of tests/test_gpu_det_exact.py runs; every argument
refusal returns UBX_EINVAL with a message before any launch; the rule header as a stand-alone program under the host sanitizers
against tests/det_ref.py (Philox words and dead / gained values bit for bit, noisy values within the derived bound);
DetectorEffects.table; the distribution of the reference's normals; the host-side refusals of a stager that carries a detector."""
import ast
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import det_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_det.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib, case_ids_run_by_the_gpu_module  # noqa: E402
from ubresnet_amd import _det as K  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd import synthetic  # noqa: E402
from ubresnet_amd.augment import Augment  # noqa: E402
from ubresnet_amd.detector import DetectorEffects, STREAM_TAG  # noqa: E402
from ubresnet_amd.staging import BatchStager  # noqa: E402

LIB = B.LIBS["det"].out
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_det.h"\n'
                     'int main(void) {\n'
                     '  int (*f)(float*, int64_t*, float*, int, int, int, int, const uint32_t*, float, int, uint32_t, uint32_t, int, int64_t, int,\n'
                     '           float, void*) = ubx_apply;\n'
                     '  const char* (*e)(void) = ubx_last_error;\n'
                     '  int (*v)(void) = ubx_version;\n'
                     '  return f == 0 || e == 0 || v == 0 || UBX_OK != 0 || UBX_EINVAL != -1 || UBX_ELAUNCH != -2 || UBX_LANE_PIXELS != 4\n'
                     '         || UBX_PHILOX_TAG != 0x55425844u;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ubx_[a-z_0-9]+)\s*\(", text))
    assert declared == set(K.SYMBOLS) and len(K.SYMBOLS) == len(set(K.SYMBOLS)) == 3
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBX_(LANE_PIXELS|BLOCK|MAX_GRID)\s+(\d+)", text)}
    assert geometry == dict(LANE_PIXELS=K.LANE_PIXELS, BLOCK=K.BLOCK, MAX_GRID=K.MAX_GRID)
    assert geometry == dict(LANE_PIXELS=R.LANE_PIXELS, BLOCK=R.BLOCK, MAX_GRID=R.MAX_GRID) == dict(LANE_PIXELS=4, BLOCK=256, MAX_GRID=1024)
    tag = int(re.search(r"#define\s+UBX_PHILOX_TAG\s+(0x[0-9a-fA-F]+)u", text).group(1), 16)
    assert tag == K.PHILOX_TAG == R.PHILOX_TAG == STREAM_TAG == 0x55425844
    assert [K.row_words(w) for w in (1, 32, 33, 832)] == [R.row_words(w) for w in (1, 32, 33, 832)] == [2, 2, 3, 27]
    # the rule, the trust in the table and which template is which are stated in the header
    for phrase in ("THE KERNEL TRUSTS THE TABLE", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "cospif(2 u2)", "sinpif(2 u2)",
                   "__fsqrt_rn", "bit for bit", "EVERY plane", "detector_kernel<false>", "detector_kernel<true>", "not a byte is written"):
        assert phrase in raw, phrase
    need_lib(LIB)


def test_the_compiled_kernels_are_the_case_table():
    """no kernel without a case, no case without a kernel; the table's ids are the ids the GPU module runs"""
    need_lib(LIB)
    compiled = kernel_symbols.kernels(LIB)
    assert compiled == sorted(R.KERNEL_CASES) == ["detector_kernel<false>", "detector_kernel<true>"], compiled
    assert all(R.KERNEL_CASES[k] for k in compiled)
    ids = [i for v in R.KERNEL_CASES.values() for i in v]
    assert len(ids) == len(set(ids)) and case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_det_exact.py")) == set(ids)


def test_shapes_follow_the_launch_geometry():
    b, p, h, w = R.STRIDE_SHAPE
    assert R.groups(b, h, w) > R.MAX_GRID * R.BLOCK and w % 4 == 0 and b * p * h * w <= 4 * 2 ** 20
    assert R.SHAPES == [(2, 1, 3, 8), (2, 3, 5, 12), (1, 1, 5, 7), (2, 3, 2, 37), (1, 2, 3, 260)]
    assert [R.row_words(s[3]) for s in R.SHAPES] == [2, 2, 2, 3, 10]
    assert R.groups(1, 5, 7) == 10 and R.groups(2, 2, 37) == 40


def test_detector_does_not_import_torch():
    tree = ast.parse(open(os.path.join(REPO, "ubresnet_amd", "detector.py")).read())
    names = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    names += [n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert "torch" not in [str(n).split(".")[0] for n in names]


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------------------------------
# addresses that are never dereferenced: every call below is refused on the host, before any launch.  2 x 1 x 8 x 8: the image and
# the weights are 512 bytes each, the labels 1024, the table 2 x 1 x 2 words = 16
_P = 0x100000
_GOOD = dict(image=_P, label=_P + 0x1000, weight=_P + 0x2000, table=_P + 0x3000, B=2, P=1, H=8, W=8, sigma=0.0, all=0, seed=1, seq=2,
             set_label=1, dead_label=0, set_weight=1, dead_weight=0.0)
_BAD = {
    "null image": (dict(image=None), "null pointer (image, table)"),
    "null table": (dict(table=None), "null pointer (image, table)"),
    "null label with set_label": (dict(label=None), "null label with set_label"),
    "null weight with set_weight": (dict(weight=None), "null weight with set_weight"),
    "B 0": (dict(B=0), "must all be >= 1"),
    "P 0": (dict(P=0), "must all be >= 1"),
    "H negative": (dict(H=-8), "must all be >= 1"),
    "W 0": (dict(W=0), "must all be >= 1"),
    "B*H*W 2^31": (dict(B=2, H=32768, W=32768), "must be below 2^31"),
    "sigma negative": (dict(sigma=-1.0), "must be finite and >= 0"),
    "sigma inf": (dict(sigma=float("inf")), "must be finite and >= 0"),
    "sigma NaN": (dict(sigma=float("nan")), "must be finite and >= 0"),
    "dead_weight inf": (dict(dead_weight=float("inf")), "dead_weight"),
    "dead_weight NaN": (dict(dead_weight=float("nan")), "dead_weight"),
    "image not 4-byte aligned": (dict(image=_P + 2), "natural alignment"),
    "label not 8-byte aligned": (dict(label=_P + 0x1004), "natural alignment"),
    "weight not 4-byte aligned": (dict(weight=_P + 0x2001), "natural alignment"),
    "table not 4-byte aligned": (dict(table=_P + 0x3002), "natural alignment"),
    "label is image": (dict(label=_P), "image overlaps label"),
    "weight starts inside image": (dict(weight=_P + 508), "image overlaps weight"),
    "weight inside label": (dict(weight=_P + 0x1000 + 1020), "label overlaps weight"),
    "table inside image": (dict(table=_P + 256), "image overlaps table"),
    "table ends inside label": (dict(table=_P + 0x1000 - 12), "label overlaps table"),
    "table inside weight": (dict(table=_P + 0x2000 + 508), "weight overlaps table"),
}


def _call(a):
    lib = K.lib()
    rc = lib.ubx_apply(a["image"], a["label"], a["weight"], a["B"], a["P"], a["H"], a["W"], a["table"], a["sigma"], a["all"], a["seed"], a["seq"],
                       a["set_label"], a["dead_label"], a["set_weight"], a["dead_weight"], None)
    return rc, lib.ubx_last_error().decode()


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    a = dict(_GOOD)
    change, message = _BAD[name]
    a.update(change)
    rc, msg = _call(a)
    assert rc == -1 and msg.startswith("ubx_apply") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match="ubx_apply"):
        K.check(rc, name)
    assert C.sizeof(C.c_void_p) == 8


def test_refusals_table_covers_every_check_of_the_source():
    src = open(os.path.join(B.CSRC, "ubr_det.hip")).read()
    assert src.count("SAT_CHECK(") == 9 and "define SAT_CHECK" not in src   # (the macro's definition is in ubr_sat.h)
    assert "Malloc" not in src and "hipFree" not in src and "Synchronize" not in src, "no allocation, free or sync"


# ------------------------------------------------------------------------------------------------------------------------
# the rule header as a program
# ------------------------------------------------------------------------------------------------------------------------
def _bits_to_f32(s):
    return np.array([int(s, 16)], np.uint32).view(f32)[0]


def test_rule_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/det_host.cpp has its own main and includes ubr_det_rule.h; built with -fsanitize=address,undefined (and
    -ffp-contract=off, as the library is) and run as a process of its own.  Philox words of 42 (key, counter) pairs against the
    uint64 restatement of det_ref, bit for bit; the whole rule over x in {+-0, a subnormal, ordinary values, FLT_MAX, inf, NaNs}
    x five gains x four sigmas x dead x lit/all x the four columns: dead and gained values bit for bit, noisy ones within the
    bound; the normals at the ends of the uniforms"""
    exe = str(tmp_path / "det_host")
    r = subprocess.run([cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-Wall", "-Werror", "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "det_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
    rows = [l.replace("|", " ").split() for l in p.stdout.strip().split("\n")]
    Wl = [[int(v, 16) for v in row[1:]] for row in rows if row[0] == "W"]
    El = [row[1:] for row in rows if row[0] == "E"]
    Nl = [[int(v, 16) for v in row[1:]] for row in rows if row[0] == "N"]
    assert len(Wl) == 6 * 7 and len(El) == 10 * 5 * 4 * 2 * 2 * 4 and len(Nl) == 5 * 11
    # the words: two implementations written apart agree
    seen = set()
    for seed, seq, g, r_, plane, w0, w1, w2, w3 in Wl:
        want = [int(v) for v in R.philox(seed, seq, g, r_, plane, R.PHILOX_TAG)]
        assert [w0, w1, w2, w3] == want, ((seed, seq, g, r_, plane), [hex(v) for v in want])
        seen.add((w0, w1, w2, w3))
    assert len(seen) == len(Wl), "two counters gave the same words"
    one = [int(v) for v in R.philox(np.array([7, 7]), 1000, np.array([207, 208]), 511, 47, R.PHILOX_TAG)[0]]     # broadcasting changes nothing
    assert one[0] == [w[5] for w in Wl if w[:5] == [7, 1000, 207, 511, 47]][0] and one[0] != one[1]
    # the rule
    worst, kinds = 0.0, set()
    for xb, dead, gb, sb, all_, seed, seq, g, r_, plane, c, yb in El:
        x, gain, sigma = _bits_to_f32(xb), _bits_to_f32(gb), _bits_to_f32(sb)
        dead, all_, c = int(dead), int(all_), int(c)
        seed, seq, g, r_, plane = (int(v, 16) for v in (seed, seq, g, r_, plane))
        got = _bits_to_f32(yb)
        what = "x=%s dead=%d gain=%s sigma=%s all=%d c=%d" % (xb, dead, gb, sb, all_, c)
        with np.errstate(all="ignore"):
            y = f32(0.0) if dead else (x if int(gb, 16) == R.ONE_BITS else f32(x * gain))
            noisy = (not dead) and sigma > 0 and (all_ or bool(x != 0))
            if not noisy:
                assert int(yb, 16) == int(np.array([y]).view(np.uint32)[0]), what       # bit for bit, NaN payload and -0.0 included
                kinds.add("dead" if dead else "quiet")
                continue
            z = float(R.group_normals(seed, seq, g, r_, plane)[c])
            assert abs(z) <= R.Z_MAX
            want = float(x) * float(gain) + float(sigma) * z if np.isfinite(y) else float(y)     # an overflowed product stays
            if not math.isfinite(want):
                assert (math.isnan(want) and math.isnan(got)) or float(got) == want, what
                kinds.add("wild")
                continue
            lim = R.bound(x, gain, sigma, z)
            assert abs(float(got) - want) <= lim, "%s: got %r, reference %r, bound %r" % (what, float(got), want, lim)
            worst = max(worst, abs(float(got) - want) / lim)
            kinds.add("noisy")
    assert kinds == {"dead", "quiet", "wild", "noisy"} and 0.0 < worst <= 1.0
    # the ends of the uniforms
    for a, b, ze, zo in Nl:
        we, wo = (float(v) for v in R.pair_normals(a, b))
        ge, go = (float(np.array([v], np.uint32).view(f32)[0]) for v in (ze, zo))
        for got, want in ((ge, we), (go, wo)):
            assert abs(got - want) <= R.C_ACC * R.U32 * R.Z_REL * abs(want) + R.FLOOR, (hex(a), hex(b), got, want)
        if a == 0xFFFFFFFF:
            assert ge == 0.0 and go == 0.0                                               # u1 == 1: radius 0
        if a == 0 and b == 0:
            assert abs(ge - R.Z_MAX) <= 1e-6 and go == 0.0                               # the largest |z| there is
        if b in (0x40000000, 0xC0000000):
            assert ge == 0.0                                                             # cos at a quarter and three quarters of a turn
        if b in (0, 0x80000000):
            assert go == 0.0


# ------------------------------------------------------------------------------------------------------------------------
# the distribution of z
# ------------------------------------------------------------------------------------------------------------------------
def test_the_normals_of_the_reference_are_standard_normal():
    """N = 2^20 counters (2^22 normals: the statistics are taken per column of the group, N each, and over all)"""
    n = 1 << 20
    z = R.group_normals(12345, 6, np.arange(1024, dtype=np.uint64)[None, :], np.arange(1024, dtype=np.uint64)[:, None], 3).reshape(n, 4)
    assert np.abs(z).max() <= 5.77 and np.abs(z).max() <= R.Z_MAX
    p2 = 0.0455002638963584                                          # P(|z| > 2) = erfc(sqrt 2)
    assert abs(p2 - math.erfc(math.sqrt(2.0))) < 1e-15 and abs(p2 - 0.0455) < 1e-5
    for col in list(z.T) + [z.reshape(-1)]:
        N = col.size
        assert abs(col.mean()) <= 5.0 / math.sqrt(N)
        assert abs(col.var() - 1.0) <= 5.0 * math.sqrt(2.0 / N)
        assert abs((np.abs(col) > 2.0).mean() - 0.0455) <= 5.0 * math.sqrt(0.0455 * (1.0 - 0.0455) / N)
    assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) <= 5.0 / math.sqrt(n)            # the cosine and the sine of one pair
    assert abs(np.corrcoef(z[:, 0], z[:, 2])[0, 1]) <= 5.0 / math.sqrt(n)
    # every element of a batch is reached through its own counter: normals() is group_normals() laid out
    full = R.normals(9, 4, 2, 3, 5, 11)
    assert full.shape == (2, 3, 5, 11)
    assert full[1, 2, 4, 10] == R.group_normals(9, 4, 2, 4, 1 * 3 + 2)[2] and full[0, 1, 3, 4] == R.group_normals(9, 4, 1, 3, 1)[0]
    assert not np.array_equal(full, R.normals(9, 5, 2, 3, 5, 11)) and not np.array_equal(full, R.normals(10, 4, 2, 3, 5, 11))


# ------------------------------------------------------------------------------------------------------------------------
# DetectorEffects.table
# ------------------------------------------------------------------------------------------------------------------------
DET = dict(dead_runs=(0, 3), run_len=(1, 40), gain=(0.9, 1.1), seed=5)
_BW = (8, 3, 100)                                                    # batch, planes, width of the draws below: a partial fourth word


def _runs_of(dead_row):
    """[(start, length)] of the maximal runs of a bool row"""
    d = np.diff(np.concatenate([[0], dead_row.astype(np.int8), [0]]))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return list(zip(starts.tolist(), (ends - starts).tolist()))


def test_table_is_a_pure_function_of_seed_and_seq():
    d = DetectorEffects(**DET)
    first = {s: d.table(s, *_BW) for s in (0, 1, 2, 5, 1000)}
    again = {s: DetectorEffects(**DET).table(s, *_BW) for s in (1000, 5, 2, 1, 0)}       # another object, another order
    for s in first:
        assert first[s].dtype == np.uint32 and first[s].shape == (8, 3, 1 + 4)
        assert np.array_equal(first[s], again[s]) and np.array_equal(first[s], d.table(s, *_BW))
    assert np.array_equal(d.table(3, 8, 3, 100)[:4], d.table(3, 4, 3, 100))               # a prefix: draws come image by image
    assert not np.array_equal(first[0], first[1]) and not np.array_equal(first[1], first[2])
    assert not np.array_equal(first[0], DetectorEffects(**dict(DET, seed=6)).table(0, *_BW))
    assert np.array_equal(first[5], d.draw(np.random.RandomState(np.array([5, 5, 0x55425844], np.uint32)), *_BW))
    # apart from Augment's stream under the same seed
    assert Augment(seed=5).params(5, 8).tolist() == Augment(seed=5).draw(np.random.RandomState(np.array([5, 5], np.uint32)), 8).tolist()
    with pytest.raises(ValueError, match="seq must fit 32 bits"):
        d.table(2 ** 32, *_BW)
    with pytest.raises(ValueError, match=">= 1"):
        d.table(0, 0, 3, 100)


def test_table_draws_stay_in_their_ranges_and_reach_the_edges():
    """40 batches of 8 x 3 planes: 960 draws of (runs, gain), replayed from the documented order"""
    d = DetectorEffects(**DET)
    b, p, w = _BW
    counts, lengths, crossing, clipped, gains = [], [], 0, 0, []
    for seq in range(40):
        t = d.table(seq, b, p, w)
        gbits, dead = R.unpack_table(t, w)
        assert not (t[..., -1] >> np.uint32(w - 96)).any(), "a bit at or beyond W is set"
        rs = np.random.RandomState(np.array([5, seq, 0x55425844], np.uint32))
        for i in range(b):
            for j in range(p):
                runs = d.runs(rs, w)                                              # the runs, then the gain: the documented order
                g = f32(rs.uniform(0.9, 1.1))
                assert gbits[i, j] == g.view(np.uint32)
                want = np.zeros(w, bool)
                for start, length in runs:
                    assert 0 <= start < w and 1 <= length <= 40
                    want[start:start + length] = True
                    crossing += (start >> 5) != ((min(start + length, w) - 1) >> 5)
                    clipped += start + length > w
                    lengths.append(length)
                assert np.array_equal(dead[i, j], want)
                counts.append(len(runs))
                gains.append(float(g))
                assert sum(n for _, n in _runs_of(dead[i, j])) == dead[i, j].sum()
    assert len(counts) == 960 and set(counts) == {0, 1, 2, 3} and min(lengths) == 1 and max(lengths) == 40
    assert crossing > 0 and clipped > 0, "no run crossed a 32-column word boundary / was clipped at W with this seed"
    assert f32(0.9) <= min(gains) and max(gains) <= f32(1.1) and max(gains) - min(gains) > 0.15


def test_disabled_effects_draw_nothing():
    t = DetectorEffects(seed=3).table(2, 4, 3, 70)
    assert t.shape == (4, 3, 1 + 3) and (t[..., 0] == R.ONE_BITS).all() and not t[..., 1:].any()
    # only the gain is drawn: its draw of the first plane is then the first number of the stream
    rs = np.random.RandomState(11)
    t = DetectorEffects(gain=(0.5, 2.0)).draw(np.random.RandomState(11), 1, 1, 8)
    assert t[0, 0, 0] == f32(rs.uniform(0.5, 2.0)).view(np.uint32) and not t[..., 1:].any()
    # only the runs are drawn: the count, then length and start of each
    rs = np.random.RandomState(12)
    t = DetectorEffects(dead_runs=(2, 2), run_len=(3, 3)).draw(np.random.RandomState(12), 1, 1, 64)
    assert rs.randint(2, 3) == 2
    want = np.zeros(64, bool)
    for _ in range(2):
        assert rs.randint(3, 4) == 3
        s = rs.randint(0, 64)
        want[s:s + 3] = True
    assert np.array_equal(R.unpack_table(t, 64)[1][0, 0], want) and t[0, 0, 0] == R.ONE_BITS
    # det_ref builds the same words from a bool mask
    assert np.array_equal(R.make_table(np.ones((1, 1), f32), want[None, None]), t)


def test_detector_refusals():
    for kw in (dict(dead_runs=(-1, 2)), dict(dead_runs=(3, 2)), dict(dead_runs=3), dict(dead_runs=(0.5, 2)), dict(run_len=(0, 4)),
               dict(run_len=(5, 4)), dict(gain=(1.1, 0.9)), dict(gain=(1.0, float("inf"))), dict(gain=(float("nan"), 1.0)), dict(gain=1.0),
               dict(noise_sigma=-0.5), dict(noise_sigma=float("nan")), dict(noise_sigma=float("inf")), dict(noise_on="dark"),
               dict(seed=-1), dict(seed=2 ** 32), dict(dead_weight=float("inf")), dict(dead_label=2 ** 63)):
        with pytest.raises(ValueError, match="DetectorEffects"):
            DetectorEffects(**kw)
    d = DetectorEffects()
    assert (d.dead_runs, d.run_len, d.gain, d.noise_sigma, d.noise_on, d.dead_label, d.dead_weight, d.seed) == \
        ((0, 0), (1, 32), (1.0, 1.0), 0.0, "lit", 0, None, 0)
    assert DetectorEffects(dead_label=None, dead_weight=0.0).dead_label is None


# ------------------------------------------------------------------------------------------------------------------------
# the stager's host half
# ------------------------------------------------------------------------------------------------------------------------
def test_host_mode_stager_takes_no_detector_and_the_default_is_none():
    ld = synthetic.SyntheticLArCVDataset(height=8, width=12, tag="train", nentries=16)
    ld.start(2)
    with pytest.raises(ValueError, match="device=None"):
        BatchStager(ld, 2, 8, 12, device=None, pin=False, detector=DetectorEffects())
    with BatchStager(ld, 2, 8, 12, device=None, pin=False, timeout=5.0) as st:
        assert st.detector is None
        assert st.next().seq == 0
