"""Batch augmentation without a GPU: Augment's draws and the numpy reference of uba_augment_batch reproduce the recorded outputs of
the reference's padandcropandflip bit for bit; params is a pure function of (seed, seq); libubresnet_aug.so's header is C99,
header / binding / library agree on the entry points, the kernels compiled into it are exactly the ones the case table of
tests/test_gpu_augment_exact.py claims, every argument refusal returns its error before any launch; the track/shower accuracy; and
the host half of a stager that carries an Augment."""
import ast
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_aug.h")
GOLDEN = os.path.join(REPO, "tests", "golden", "augment_padcropflip.npz")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib, case_ids_run_by_the_gpu_module  # noqa: E402
from ubresnet_amd import _aug, metrics, synthetic  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402
from ubresnet_amd.augment import Augment  # noqa: E402
from ubresnet_amd.staging import BatchStager  # noqa: E402

LIB = B.LIBS["aug"].out


# ------------------------------------------------------------------------------------------------------------------------
# the draws and the rule against the reference's own function
# ------------------------------------------------------------------------------------------------------------------------
def test_draws_and_rule_reproduce_the_recorded_outputs_of_padandcropandflip():
    g = np.load(GOLDEN)
    seeds, outs = g["seeds"], g["outputs"]
    assert seeds.tolist() == list(range(16)) and outs.shape == (16, 256, 256) and outs.dtype == np.float32
    seen = set()
    for k, want in zip(seeds, outs):
        x = synthetic.make_batch(1, 256, 256, 1000 + int(k))[0]
        par = Augment(pad=4).draw(np.random.RandomState(int(k)), 1)
        seen.add(tuple(par[0, :2]))
        got, _, _ = R.reference(x, np.zeros((1, 256, 256), np.float32), None, par, 4)
        assert np.array_equal(got[0, 0].view(np.int32), want.view(np.int32)), "seed %d, params %s" % (k, par[0])
        assert (want != 0).any()
    assert len(seen) == 4, "the sixteen seeds must cover the four flip combinations"


def test_labels_and_weights_follow_the_image_in_the_reference():
    """image, label wire and weight filled with the pixel's own index: the three outputs name the same source pixel"""
    b, h, w, pad = 3, 6, 9, 2
    idx = np.arange(b * h * w, dtype=np.float32).reshape(b, h, w) + 1.0
    par = np.array([[0, 0, 0, 4], [1, 0, 3, 1], [1, 1, 4, 0]], np.int32)
    img, lab, wgt = R.reference(idx[:, None], idx, idx, par, pad, pad_label=0, pad_weight=0.0)
    assert np.array_equal(img[:, 0], wgt) and np.array_equal(lab, wgt.astype(np.int64))
    assert (lab == 0).any() and (lab != 0).any()
    # by hand: image 1 is flipped in the rows and cut at (3, 1): output (0, 0) is row 3 of the flipped padded image = row
    # 10 - 1 - 3 = 6 of the padded one = source row 4, and padded column 1 = source column -1: outside; (0, 1) is source (4, 0)
    assert lab[1, 0, 0] == 0 and lab[1, 0, 1] == int(idx[1, 4, 0])


# ------------------------------------------------------------------------------------------------------------------------
# Augment.params
# ------------------------------------------------------------------------------------------------------------------------
def test_params_is_a_pure_function_of_seed_and_seq():
    a = Augment(seed=7)
    first = {s: a.params(s, 16) for s in (0, 1, 2, 5, 1000)}
    again = {s: Augment(seed=7).params(s, 16) for s in (1000, 5, 2, 1, 0)}             # another object, another order
    for s in first:
        assert first[s].dtype == np.int32 and first[s].shape == (16, 4)
        assert np.array_equal(first[s], again[s]) and np.array_equal(first[s], a.params(s, 16))
        assert set(first[s][:, :2].reshape(-1)) <= {0, 1} and first[s][:, 2:].min() >= 0 and first[s][:, 2:].max() <= 7
    assert np.array_equal(a.params(3, 16)[:4], a.params(3, 4))                           # a prefix: draws come image by image
    assert not np.array_equal(first[0], first[1]) and not np.array_equal(first[1], first[2])
    assert not np.array_equal(first[0], Augment(seed=8).params(0, 16))
    assert np.array_equal(first[5], a.draw(np.random.RandomState(np.array([7, 5], np.uint32)), 16))
    every = np.concatenate([a.params(s, 16) for s in range(40)])
    assert set(every[:, 2]) == set(range(8)) and set(every[:, 3]) == set(range(8)) and 0.3 < every[:, 0].mean() < 0.7


def test_disabled_flips_and_pad_zero_give_zeros():
    assert not Augment(flip_rows=False, flip_cols=False, pad=0, seed=3).params(2, 8).any()
    p = Augment(flip_rows=False, seed=3).params(2, 64)
    assert not p[:, 0].any() and p[:, 1].any() and p[:, 2:].any()
    p = Augment(flip_cols=False, seed=3).params(2, 64)
    assert p[:, 0].any() and not p[:, 1].any()
    p = Augment(pad=0, seed=3).params(2, 64)
    assert p[:, :2].any() and not p[:, 2:].any()
    # a disabled flip draws nothing: the rows' draw of the first image is then the first number of the stream
    rs = np.random.RandomState(11)
    assert Augment(flip_cols=False, pad=0).draw(np.random.RandomState(11), 1)[0, 0] == int(rs.rand() > 0.5)
    with pytest.raises(ValueError):
        Augment(pad=-1)


def test_augment_module_does_not_import_torch():
    tree = ast.parse(open(os.path.join(REPO, "ubresnet_amd", "augment.py")).read())
    names = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    names += [n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert "torch" not in [str(n).split(".")[0] for n in names]


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ubresnet_aug.h"\nint main(void) { int (*f)(const float*, const float*, const float*, float*, int64_t*, float*, '
                   'int, int, int, int, int, const int32_t*, int32_t, int, float, int32_t, float, void*) = uba_augment_batch; '
                   'return f == 0 || UBA_LANE_PIXELS != 4 || UBA_OK != 0 || UBA_MAX_BATCH != 256; }\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(uba_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_aug.SYMBOLS) and len(_aug.SYMBOLS) == len(set(_aug.SYMBOLS))
    geometry = {k: int(v) for k, v in re.findall(r"#define\s+UBA_(LANE_PIXELS|BLOCK|MAX_GRID|MAX_BATCH|MAX_PAD)\s+(\d+)", text)}
    assert geometry == dict(LANE_PIXELS=_aug.LANE_PIXELS, BLOCK=_aug.BLOCK, MAX_GRID=_aug.MAX_GRID, MAX_BATCH=_aug.MAX_BATCH, MAX_PAD=_aug.MAX_PAD)
    assert geometry == dict(LANE_PIXELS=R.LANE_PIXELS, BLOCK=R.BLOCK, MAX_GRID=R.MAX_GRID, MAX_BATCH=R.MAX_BATCH, MAX_PAD=R.MAX_PAD)
    assert geometry["LANE_PIXELS"] == 4 and geometry["BLOCK"] == 256 and geometry["MAX_BATCH"] == 256
    need_lib(LIB)


def test_case_table_equals_the_compiled_kernels():
    need_lib(LIB)
    have = set(kernel_symbols.kernels(LIB))
    claimed = set(R.KERNEL_CASES)
    assert have - claimed == set(), "compiled kernels without a case in tests/test_gpu_augment_exact.py: %s" % sorted(have - claimed)
    assert claimed - have == set(), "cases for kernels that are not compiled: %s" % sorted(claimed - have)
    assert len(have) <= 2
    assert case_ids_run_by_the_gpu_module(os.path.join(REPO, "tests", "test_gpu_augment_exact.py")) == set(i for ids in R.KERNEL_CASES.values() for i in ids)
    assert all(ids for ids in R.KERNEL_CASES.values())


def test_stride_shape_follows_the_launch_geometry():
    b, h, w = R.stride_shape()
    items, trip = R.groups(b, h, w), R.MAX_GRID * R.BLOCK
    assert w % 4 == 0 and 2 * trip < items < 3 * trip and (items - 2 * trip) % R.BLOCK == 0
    assert b * h * w <= 4 * 2 ** 20, "at most a few million pixels"
    assert R.groups(1, 5, 7) == 10 and R.groups(2, 3, 260) == 6 * 65


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------------------------------
# pointers that are never dereferenced: every call below is refused on the host, before any launch.  The regions are laid out
# apart for a 2 x 1 x 8 x 8 batch (512 bytes of image, label wire and weight each, 1024 of labels)
_P = 0x100000
_GOOD = dict(image=_P, wire=_P + 0x1000, weight=_P + 0x2000, image_out=_P + 0x3000, label_out=_P + 0x4000, weight_out=_P + 0x5000,
             B=2, P=1, H=8, W=8, pad=4, params=[[0, 0, 0, 0], [1, 1, 8, 8]], off=0, use=0, thr=10.0, pad_label=0, pad_weight=0.0)
_BAD = {
    "null image": (dict(image=None), "null source"),
    "null label wire": (dict(wire=None), "null source"),
    "null image_out": (dict(image_out=None), "null destination"),
    "null label_out": (dict(label_out=None), "null destination"),
    "null weight_out": (dict(weight_out=None), "null destination"),
    "null params": (dict(params=None), "null params"),
    "B 0": (dict(B=0, params=[]), "must all be >= 1"),
    "W 0": (dict(W=0), "must all be >= 1"),
    "B above UBA_MAX_BATCH": (dict(B=257, H=1, W=1, params=[[0, 0, 0, 0]] * 257), "exceeds UBA_MAX_BATCH=256"),
    "B*H*W 2^31": (dict(B=2, H=32768, W=32768), "must be below 2^31"),
    "pad negative": (dict(pad=-1), "pad=-1"),
    "row offset above 2*pad": (dict(params=[[0, 0, 0, 0], [0, 0, 9, 0]]), "image 1: offsets (9, 0) must be 0..2*pad=8"),
    "column offset above 2*pad": (dict(params=[[0, 0, 0, 9], [0, 0, 0, 0]]), "image 0: offsets (0, 9)"),
    "offset negative": (dict(params=[[0, 0, -1, 0], [0, 0, 0, 0]]), "image 0: offsets (-1, 0)"),
    "offset with pad 0": (dict(pad=0, params=[[0, 0, 0, 0], [0, 0, 0, 1]]), "must be 0..2*pad=0"),
    "flip 2": (dict(params=[[2, 0, 0, 0], [0, 0, 0, 0]]), "image 0: flips (2, 0) must be 0 or 1"),
    "flip -1": (dict(params=[[0, 0, 0, 0], [0, -1, 0, 0]]), "image 1: flips (0, -1)"),
    "image_out is image": (dict(image_out=_P), "image overlaps image_out"),
    "image_out starts inside image": (dict(image_out=_P + 508), "image overlaps image_out"),
    "weight_out is weight": (dict(weight_out=_P + 0x2000), "weight overlaps weight_out"),
    "label_out covers the label wire": (dict(label_out=_P + 0x1000 - 1016), "label_wire overlaps label_out"),
    "weight_out inside label_out": (dict(weight_out=_P + 0x4000 + 1020), "label_out overlaps weight_out"),
    "image not 4-byte aligned": (dict(image=_P + 2), "natural alignment"),
    "label_out not 8-byte aligned": (dict(label_out=_P + 0x4004), "natural alignment"),
}


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    a = dict(_GOOD)
    change, message = _BAD[name]
    a.update(change)
    par = None if a["params"] is None else np.ascontiguousarray(np.array(a["params"], np.int32).reshape(-1, 4))
    lib = _aug.lib()
    rc = lib.uba_augment_batch(a["image"], a["wire"], a["weight"], a["image_out"], a["label_out"], a["weight_out"],
                               a["B"], a["P"], a["H"], a["W"], a["pad"], None if par is None else par.ctypes.data,
                               a["off"], a["use"], a["thr"], a["pad_label"], a["pad_weight"], None)
    msg = lib.uba_last_error().decode()
    assert rc == -1 and msg.startswith("uba_augment_batch") and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match="uba_augment_batch"):
        _aug.check(rc, name)
    assert C.sizeof(C.c_void_p) == 8


def test_binding_checks_the_shape_of_params():
    need_lib(LIB)
    with pytest.raises(ValueError, match="params"):
        _aug.augment_batch(_P, _P + 0x1000, None, _P + 0x3000, _P + 0x4000, _P + 0x5000, (2, 1, 8, 8), 4, np.zeros((3, 4), np.int32))
    with pytest.raises(RuntimeError, match="image 1: offsets"):
        _aug.augment_batch(_P, _P + 0x1000, None, _P + 0x3000, _P + 0x4000, _P + 0x5000, (2, 1, 8, 8), 4, [[0, 0, 0, 0], [0, 0, 0, 9]])


# ------------------------------------------------------------------------------------------------------------------------
# the fifth accuracy
# ------------------------------------------------------------------------------------------------------------------------
def test_track_shower_accuracy_on_a_hand_made_matrix():
    cm = torch.tensor([[50, 3, 2], [4, 30, 6], [1, 9, 20]], dtype=torch.int64)
    plain = metrics.accuracy_from_confusion(cm)
    five = metrics.accuracy_from_confusion(cm, track_shower=True)
    assert len(plain) == 4 and five[:4] == plain
    assert five[4] == 100.0 * (30 + 20) / (40 + 30)
    # background only: the reference would divide by zero
    cm = torch.tensor([[7, 1, 2], [0, 0, 0], [0, 0, 0]], dtype=torch.int64)
    five = metrics.accuracy_from_confusion(cm, track_shower=True)
    assert five == [70.0, 0.0, 0.0, 70.0, 0.0]
    assert metrics.accuracy_from_confusion(cm) == [70.0, 0.0, 0.0, 70.0]
    with pytest.raises(ValueError):
        metrics.accuracy_from_confusion(torch.ones((2, 2), dtype=torch.int64), track_shower=True)


# ------------------------------------------------------------------------------------------------------------------------
# host-mode stager
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 2])
def test_host_mode_stager_hands_out_seq_and_the_augment(threads):
    b, h, w = 3, 8, 12
    ld = synthetic.SyntheticLArCVDataset(height=h, width=w, tag="train", nentries=64)
    ld.start(b)
    aug = Augment(pad=2, seed=5)
    got = []
    with BatchStager(ld, b, h, w, device=None, pin=False, threads=threads, timeout=5.0, augment=aug) as st:
        assert st.augment is aug
        for k in range(6):
            batch = st.next()
            assert batch.seq == k
            x, lab, wgt = synthetic.make_batch(b, h, w, 1000 + b * k)
            assert np.array_equal(batch.image, x) and np.array_equal(batch.label_wire, lab.astype(np.float32))     # not augmented
            par = st.augment.params(batch.seq, b)
            got.append(R.reference(batch.image, batch.label_wire, batch.weight, par, aug.pad))
    ref = test_host_mode_stager_hands_out_seq_and_the_augment.__dict__.setdefault("first", got)
    for one, other in zip(ref, got):                               # the same batches whatever the thread count
        assert all(np.array_equal(p, q) for p, q in zip(one, other))
    with BatchStager(ld, b, h, w, device=None, pin=False, timeout=5.0) as st:
        assert st.augment is None
