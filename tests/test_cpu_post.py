"""libubresnet_post.so without a GPU: its header is C99, the header / binding / library agree on the entry points, the kernels
compiled into it are exactly the ones the case table of tests/test_gpu_post_exact.py claims, and the numpy reference those GPU
tests compare against agrees with torch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import post_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_post.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib, case_ids_run_by_the_gpu_module  # noqa: E402
from ubresnet_amd import _post  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd import deploy  # noqa: E402

LIB = B.LIBS["post"].out


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ubresnet_post.h"\nint main(void) { int (*f)(const float*, int, int, int, const int32_t*, int, const float*, int, float, uint8_t*, uint16_t*, unsigned long long*, int, int, int, int, void*) = ubp_stitch_products; return f == 0 || UBP_MAX_TILES != 64 || UBP_OK != 0; }\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_and_library_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ubp_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_post.SYMBOLS) and len(_post.SYMBOLS) == len(set(_post.SYMBOLS))
    need_lib(LIB)
    assert _post.lib().ubp_last_error() == b""


def test_case_table_equals_the_compiled_kernels():
    need_lib(LIB)
    have = set(kernel_symbols.kernels(LIB))
    claimed = set(R.KERNEL_CASES)
    assert have - claimed == set(), "compiled kernels without a case in tests/test_gpu_post_exact.py: %s" % sorted(have - claimed)
    assert claimed - have == set(), "cases for kernels that are not compiled: %s" % sorted(claimed - have)
    assert case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_post_exact.py")) == set(i for ids in R.KERNEL_CASES.values() for i in ids)
    assert all(ids for ids in R.KERNEL_CASES.values())


def test_edge_rows_of_the_reference():
    for name, s, lab, bits in R.EDGE_ROWS + [("filler", R.EDGE_FILLER, 2, 0x3A3B)]:
        best, bv = R.first_argmax(np.array(s, np.float32).reshape(4, 1, 1))
        h, _, near = R.confidence_bits(bv)
        assert int(best[0, 0]) == lab and not near[0, 0], name
        assert R._is_nan16(h[0, 0]) if bits is None else int(h[0, 0]) == bits, name


def test_near_tie_rule_flags_a_midpoint_and_nothing_far_from_one():
    lo, hi = np.float16(0.5), np.nextafter(np.float16(0.5), np.float16(1))
    mid = 0.5 * (float(lo) + float(hi))
    bv = np.array([np.log(mid), np.log(float(lo)), np.log(mid * (1 + 1e-5))], np.float64).astype(np.float32)
    h, other, near = R.confidence_bits(bv)
    assert near.tolist() == [True, False, False]
    assert {int(h[0]), int(other[0])} == {int(lo.view(np.uint16)), int(hi.view(np.uint16))}


def test_numpy_reference_against_torch():
    """ragged tiling, NaN-free scores: torch stitches by slicing, then argmax / exp().half() / bincount on the full view"""
    P, rows, cols, th, tw, Cn, thr = 2, 45, 83, 32, 64, 4, 10.0
    desc = R.regular_desc(P, [0, 13], [0, 19], th, tw, rows, cols, deploy._keep_windows)
    rs = np.random.RandomState(5)
    logp = R.logsoftmax_scores(rs, len(desc), Cn, th, tw)
    adc = R.adc_view(rs, P, rows, cols, thr)
    counts0 = rs.randint(1, 1000, (P, Cn)).astype(np.int64)
    ref = R.reference(logp, Cn, th, tw, desc, adc, 1, thr, np.full((P, rows, cols), 0xA5, np.uint8),
                      np.full((P, rows, cols), 0x7B7B, np.uint16), counts0, 255, P, rows, cols)
    full = torch.full((P, Cn, rows, cols), float("nan"))
    lt = torch.from_numpy(logp)
    for t, (p, r0, c0, kr0, kr1, kc0, kc1) in enumerate(desc):
        y1, x1 = min(kr1, rows - r0), min(kc1, cols - c0)
        full[p, :, r0 + kr0:r0 + y1, c0 + kc0:c0 + x1] = lt[t, :, kr0:y1, kc0:x1]
    assert not torch.isnan(full).any()
    lit = torch.from_numpy(adc) > thr
    lab = torch.where(lit, full.argmax(1), torch.tensor(255)).to(torch.uint8)
    conf = torch.where(lit, full.max(1)[0].exp().half(), torch.zeros((), dtype=torch.float16))
    counts = torch.stack([torch.bincount(full[p].argmax(0)[lit[p]], minlength=Cn) for p in range(P)]) + torch.from_numpy(counts0)
    share = R.accept(lab.numpy(), conf.view(torch.int16).numpy().view(np.uint16), counts.numpy(), ref, "torch")
    assert np.array_equal(ref["lit"], lit.numpy()) and 0.4 < ref["lit"].mean() < 0.6
    assert share <= R.NEAR_SHARE


def test_python_surface_rejects_a_wrong_output_without_a_gpu():
    class M:
        pass
    with pytest.raises(ValueError):
        deploy.WholeViewSegmenter(M(), 64, 96, output="labels")
    with pytest.raises(ValueError):
        deploy.segment_crops(M(), torch.zeros(1, 1, 8, 8), output="labels")
    assert deploy.Products._fields == ("label", "confidence", "counts")


def test_products_path_refuses_a_tiling_that_does_not_partition_the_view():
    deploy._check_cover(deploy.view_tiles(1008, 3456, 3, 512, 832, False), 3, 1008, 3456)
    deploy._check_cover(deploy.view_tiles(64, 160, 3, 64, 96, True), 1, 64, 160)
    tiles = deploy.view_tiles(96, 160, 2, 64, 96, False)
    with pytest.raises(ValueError):
        deploy._check_cover(tiles[:-1], 2, 96, 160)                       # a hole
    with pytest.raises(ValueError):
        deploy._check_cover(tiles + tiles[:1], 2, 96, 160)                # a pixel kept twice
