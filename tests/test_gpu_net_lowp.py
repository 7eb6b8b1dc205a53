"""Stem, head and the whole networks in bf16 and fp16, launch by launch (GPU).

The stage cases of tests/test_gpu_stages_lowp.py stop at the blocks, the decoder layer and one ASPP level.  These cases run
Engine.stem_pool_fwd / stem_pool_bwd, Engine.head_fwd / head_bwd and whole training passes of UResNet and ASPP_ResNet
(Engine.forward_eager / backward_eager, never the plan; weight-gradient side stream off) under the launch tap of
tests/stage_shadow.py and finish through the same checks:
  * wiring: the recorded tape against the launch graph written down from the module (Graph.match binds every launch): the
    per-plane image, addend and dst_offset of the stem launches, the skip half of cat1 the pool copies into, the saved arg-max, the
    fresh fp32 NCHW tensor of the head, and for the networks which channel slice of which concat buffer every encoder level
    writes and every decoder level reads, which gradient slice every encoder level is owed, and the arena affines of
    ASPP_ResNet's dec_layer5 / dec_layer4;
  * numerics: every launch against fp64 of ITS OWN recorded inputs with the bounds kref.py derives (log-softmax epilogue on
    inexact logits, the pool on an on-load affine, the arg-max's near-tie window), every ratio <= 1, and the gradient buffer;
  * the end result: outputs finite; bytes around every output view untouched (for storages above stage_shadow.BIG_STORAGE the
    comparison runs on the device when the launch is recorded); outputs and gradients equal the chain of once-rounded replays
    wherever its bound is zero, and that set is not empty in a training case.
There is no end-to-end tolerance and no comparison with another path of the library.  Measured ratios and wall times:
profiles/net_lowp.txt.
"""
import time

import pytest
import torch

import stage_shadow as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.bfloat16, torch.float16]


def _finish(name, dt, r, training=True):
    t0 = time.time()
    stat = S.check_all(r)
    for o in r["outputs"]:
        assert bool(torch.isfinite(o.float()).all()), "%s: stage output not finite" % name
    n = sum(v[0] for v in stat.values())
    print("%-28s %-8s launches %3d  exact %6d  %s" % (name, str(dt).replace("torch.", ""), n, r["exact"],
                                                     "  ".join("%s %d x %.3f" % (k, v[0], v[1]) for k, v in sorted(stat.items()))))
    if "t_run" in r:
        print("%-28s %-8s pass under the tap %.1f s, checks %.1f s" % (name, str(dt).replace("torch.", ""), r["t_run"], time.time() - t0))
    assert all(v[1] <= 1.0 for v in stat.values())
    assert n == len(r["tape"]), "%s: %d of %d launches checked" % (name, n, len(r["tape"]))
    assert r["exact"] > 0 or not training, "%s: the chain of rounded replays compared nothing" % name
    return stat


# one plane, 16 channels; three planes (planes 1 and 2 add onto c0 in place, bias on plane 0, statistics on plane 2), the 32-channel thin kernel
STEMS = [(2, 1, 24, 40, 16), (2, 3, 20, 36, 32)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cfg", STEMS)
def test_stem_and_pool(monkeypatch, dt, cfg):
    _finish("stem+pool %dx%dx%dx%d ip%d" % cfg, dt, S.stem_case(monkeypatch, dt, DEV, *cfg))


@pytest.mark.parametrize("dt", DTS)
def test_stem_and_pool_eval(monkeypatch, dt):
    """bn1 frozen, nothing saved: bn_eval_affine, no arg-max; pooled is the maximum of the stored window"""
    _finish("stem+pool eval", dt, S.stem_case(monkeypatch, dt, DEV, *STEMS[0], training=False), training=False)


HEADS = [((2, 24, 40, 16, 16, 3), ()), ((2, 20, 36, 16, 16, 4), ()), ((2, 24, 40, 16, 16, 3), ("bn10",))]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cfg,freeze", HEADS)
def test_head(monkeypatch, dt, cfg, freeze):
    _finish("head %dx%dx%d ncls%d%s" % (cfg[0], cfg[1], cfg[2], cfg[5], " bn10 frozen" if freeze else ""), dt,
            S.head_case(monkeypatch, dt, DEV, *cfg, freeze=freeze))


@pytest.fixture(scope="module")
def uresnet_run():
    mp = pytest.MonkeyPatch()
    try:
        r = S.net_case(mp, torch.bfloat16, DEV, "uresnet")
    finally:
        mp.undo()          # (the tap comes off before any other test launches anything: the tape is this pass and nothing else)
    return r


def test_whole_uresnet(uresnet_run):
    """UResNet(3 classes, 1 plane, inplanes 16) at 2 x 1 x 32 x 64 in bf16"""
    _finish("whole UResNet", torch.bfloat16, uresnet_run)


def test_whole_aspp_resnet(monkeypatch):
    """ASPP_ResNet (inplanes 16, the only width it builds) at 2 x 3 x 32 x 64 in fp16.  At the 1 x 2 bottom level gradient operands
    fall below f16's smallest normal; the matrix cores take such an operand at the nominal exponent 2^-14, which the weight
    gradient's bound accounts for (kref.nominal_abs).  The pass differs from run to run (the bottom level normalises over 4 values
    per channel and amplifies the order of the statistics' atomics); the bounds hold whichever way it goes."""
    _finish("whole ASPP_ResNet", torch.float16, S.net_case(monkeypatch, torch.float16, DEV, "aspp"))


@pytest.mark.parametrize("kind", S.NET_MUTATIONS)
def test_corrupted_network_tape_is_rejected(uresnet_run, kind):
    """the recorded tape of the whole UResNet with ONE record changed (the launches are not touched)"""
    tape, what = S.mutate(uresnet_run["tape"], kind)
    with pytest.raises(AssertionError):
        uresnet_run["graph"].match(tape)
    if kind in S.VALUE_MUTATIONS:
        with pytest.raises(AssertionError):
            S.replay([L for L in tape if L.op == "conv" and L.args["logsoftmax"]])
    print("mutation %-18s (%s): rejected" % (kind, what))


@pytest.mark.parametrize("kind", S.STEM_MUTATIONS)
def test_corrupted_stem_tape_is_rejected(monkeypatch, kind):
    """the one-plane network has no second stem plane: this record is changed on the three-plane stem case's tape"""
    r = S.stem_case(monkeypatch, torch.bfloat16, DEV, *STEMS[1])
    tape, what = S.mutate(r["tape"], kind)
    with pytest.raises(AssertionError):
        r["graph"].match(tape)
    print("mutation %-18s (%s): rejected" % (kind, what))
