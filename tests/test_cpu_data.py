"""libubresnet_data.so without a GPU: its header is C99, the header / binding / library agree on the entry points, the kernels
compiled into it are exactly the ones the case table of tests/test_gpu_data_exact.py claims, the numpy reference those GPU tests
compare against agrees with prep_data's own arithmetic, and every argument refusal returns its error before any launch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import data_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_data.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib, case_ids_run_by_the_gpu_module  # noqa: E402
from ubresnet_amd import _data  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402

LIB = B.LIBS["data"].out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ubresnet_data.h"\nint main(void) { int (*f)(const float*, int64_t*, int64_t, int32_t, float*, int, int64_t, int, float, float*, void*) = ubd_prep_batch; return f == 0 || UBD_LANE_PIXELS != 4 || UBD_OK != 0; }\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ubd_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_data.SYMBOLS) and len(_data.SYMBOLS) == len(set(_data.SYMBOLS))
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBD_(LANE_PIXELS|BLOCK|MAX_GRID)\s+(\d+)", text)}
    assert geometry == dict(LANE_PIXELS=_data.LANE_PIXELS, BLOCK=_data.BLOCK, MAX_GRID=_data.MAX_GRID)
    assert geometry == dict(LANE_PIXELS=R.LANE_PIXELS, BLOCK=R.BLOCK, MAX_GRID=R.MAX_GRID)
    need_lib(LIB)


def test_case_table_equals_the_compiled_kernels():
    need_lib(LIB)
    have = set(kernel_symbols.kernels(LIB))
    claimed = set(R.KERNEL_CASES)
    assert have - claimed == set(), "compiled kernels without a case in tests/test_gpu_data_exact.py: %s" % sorted(have - claimed)
    assert claimed - have == set(), "cases for kernels that are not compiled: %s" % sorted(claimed - have)
    assert case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_data_exact.py")) == set(i for ids in R.KERNEL_CASES.values() for i in ids)
    assert all(ids for ids in R.KERNEL_CASES.values())


def test_counts_follow_the_launch_geometry():
    L, wave, wg = R.LANE_PIXELS, 64 * R.LANE_PIXELS, R.BLOCK * R.LANE_PIXELS
    for s in (L, wave, wg):
        assert {s - 1, s, s + 1} <= set(R.COUNTS)
    assert 1 in R.COUNTS
    assert any(n > wg and 0 < n % wg < wg and (n % wg) % wave for n in R.COUNTS)            # a partial last workgroup
    assert R.STRIDE_COUNT >= 2 * R.MAX_GRID * wg and R.STRIDE_COUNT % wg and R.STRIDE_COUNT % L


def _prep_data_labels(wire, shape, offset=0):
    """prep_data's own line :601 (np.int is int64 there), plus the offset of larcv1_interface.py:59"""
    return wire.reshape(shape).astype(np.int64) + offset


def test_reference_is_prep_data_with_the_threshold_off():
    rs = np.random.RandomState(3)
    shape = (3, 5, 7)
    n = int(np.prod(shape))
    for wire in (rs.randint(0, 3, n).astype(np.float32),                       # integer-valued labels
                 rs.uniform(-40.0, 40.0, n).astype(np.float32)):               # fractional and negative values
        for off in (0, -1):
            wgt0 = rs.rand(n).astype(np.float32)
            lab, img, wgt = R.reference(wire, off, weight=wgt0, fill_weight=True)
            assert np.array_equal(lab.reshape(shape), _prep_data_labels(wire, shape, off))
            assert img is None and np.array_equal(wgt.reshape(shape), np.ones(shape, dtype=np.float32))          # :605
            assert np.array_equal(R.reference(wire, off, weight=wgt0)[2], wgt0)                                  # a wire weight stays


def test_reference_on_the_edge_list():
    """where |v| < 2^31 the reference is astype's value; elsewhere astype's result is undefined behaviour of the C cast (this
    host gives INT64_MIN for NaN, the infinities and 3e38, and +-2^31 for +-2^31) and the rule gives INT64_MIN: either is outside
    [0, C) and different from ignore_index, so PixelWiseNLLLoss reports both as a bad label"""
    wire = np.array([e for e, _ in R.EDGE_LABELS], np.float32)
    for off in (0, -1):
        lab = R.reference(wire, off)[0]
        for (v, want), got in zip(R.EDGE_LABELS, lab):
            if want is None:
                assert not abs(float(v)) < 2.0 ** 31 and got == R.INT64_MIN, v
            else:
                assert abs(float(v)) < 2.0 ** 31 and got == want + off, v
                assert got == _prep_data_labels(np.array([v], np.float32), (1,), off)[0], v
    assert float(np.float32(2147483520.0)) == 2.0 ** 31 - 128 and np.nextafter(np.float32(2147483520.0), np.float32(np.inf)) == np.float32(2.0 ** 31)
    assert 0 < abs(float(np.float32(1e-40))) < float(np.finfo(np.float32).tiny)


def test_reference_is_the_two_commented_lines_with_the_threshold_on():
    """lines :608-609 on a one-plane batch, positive threshold (the second line then sees the zeros the first wrote: still below)"""
    rs = np.random.RandomState(4)
    b, h, w, thr = 3, 5, 7, 10.0
    src = R.adc_image(rs, b, 1, h * w, thr)
    src = np.where(np.isnan(src), np.float32(12.0), src)          # (torch's < agrees on NaN; keep the comparison about the rule)
    wire = rs.randint(0, 3, b * h * w).astype(np.float32)
    lab, img, _ = R.reference(wire, 0, image=src, planes=1, hw=h * w, threshold=thr)
    source_t = torch.from_numpy(src.copy().reshape(b, 1, h, w))
    label_t = torch.from_numpy(_prep_data_labels(wire, (b, h, w)))
    source_t[source_t < thr] = 0.0
    label_t[(source_t < thr)[:, 0]] = 0
    assert np.array_equal(img.view(np.int32), source_t.numpy().reshape(-1).view(np.int32))
    assert np.array_equal(lab, label_t.numpy().reshape(-1))
    assert 0.2 < (lab == 0).mean() < 0.95 and (img == 0).any() and (img > thr).any()


def test_reference_threshold_rules():
    t = np.float32(10.0)
    below, above = np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))
    # 4 pixels x 3 planes, hw = 4, one image: all below | lit in plane 1 only | at the threshold in plane 2 | NaN in plane 0
    img = np.array([[below, 3.0, -0.0, np.nan],
                    [-0.0, above, 1.0, 2.0],
                    [1.0, 2.0, t, 3.0]], np.float32).reshape(-1)
    lab, out, _ = R.reference(np.array([2, 2, 2, 2], np.float32), -1, image=img, planes=3, hw=4, threshold=10.0)
    assert lab.tolist() == [0, 1, 1, 1]
    want = np.array([[0.0, 0.0, 0.0, np.nan], [0.0, above, 0.0, 0.0], [0.0, 0.0, t, 0.0]], np.float32).reshape(-1)
    assert np.array_equal(out.view(np.int32), want.view(np.int32))              # -0.0 became +0.0, the NaN kept its bits
    # threshold 0.0: -0.0 is not below, it stays as it is and keeps the pixel's label
    lab, out, _ = R.reference(np.array([2, 2], np.float32), 0, image=np.array([-0.0, -1.0], np.float32), planes=1, hw=2, threshold=0.0)
    assert lab.tolist() == [2, 0] and out.view(np.int32).tolist() == [-2 ** 31, 0]


# a pointer that is never dereferenced: every call below is refused on the host, before any launch
_P = 0x10000
_GOOD = dict(wire=_P, out=_P, n=64, off=0, image=_P, planes=1, hw=64, use=0, thr=10.0, wgt=_P)
_BAD = {
    "n 0": dict(n=0),
    "n negative": dict(n=-5),
    "n 2^31": dict(n=2 ** 31),
    "planes 0": dict(planes=0),
    "null wire label": dict(wire=None),
    "null label output": dict(out=None),
    "threshold on, null image": dict(use=1, image=None),
    "threshold on, hw does not divide n": dict(use=1, hw=48),
    "wire label not 4-byte aligned": dict(wire=_P + 2),
    "label output not 8-byte aligned": dict(out=_P + 4),
}


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    a = dict(_GOOD)
    a.update(_BAD[name])
    lib = _data.lib()
    rc = lib.ubd_prep_batch(a["wire"], a["out"], a["n"], a["off"], a["image"], a["planes"], a["hw"], a["use"], a["thr"], a["wgt"], None)
    msg = lib.ubd_last_error().decode()
    assert rc == -1 and msg.startswith("ubd_prep_batch"), (rc, msg)
    with pytest.raises(RuntimeError, match="ubd_prep_batch"):
        _data.check(rc, name)
    assert C.sizeof(C.c_void_p) == 8
