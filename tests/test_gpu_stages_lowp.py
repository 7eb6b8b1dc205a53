"""BasicBlock / DoubleResNet / ConvTransposeLayer / ASPP-level stages in bf16 and fp16, launch by launch (GPU).

Every case runs a stage of ubresnet_amd.engine under the launch tap of tests/stage_shadow.py and then checks
  * wiring: the recorded tape against the launch graph written down from the module (stage_shadow.Graph.match);
  * numerics: every launch against fp64 of ITS OWN recorded inputs, with the bounds kref.py derives (stage_shadow.replay),
    and the flat gradient buffer after the stage's flush (check_gradients);
  * the end result: outputs and gradients finite; bytes around every output view untouched; and the outputs and the gradient
    buffer as they stand at the end of the stage equal the chain of per-launch replays, each rounded once to its stored type,
    wherever that chain's bound is zero (stage_shadow.check_chain).
There is no end-to-end tolerance.  Measured ratios of observed error to bound: profiles/stage_lowp.txt.
"""
import pytest
import torch

import kref
import stage_shadow as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = [torch.bfloat16, torch.float16]


def _finish(name, dt, r):
    stat = S.check_all(r)
    for o in r["outputs"]:
        assert bool(torch.isfinite(o.float()).all()), "%s: stage output not finite" % name
    n = sum(v[0] for v in stat.values())
    line = "%-28s %-8s launches %3d  exact %6d  %s" % (name, str(dt).replace("torch.", ""), n, r["exact"],
                                            "  ".join("%s %d x %.3f" % (k, v[0], v[1]) for k, v in sorted(stat.items())))
    print(line)
    assert all(v[1] <= 1.0 for v in stat.values())
    return stat


# identity blocks: the skip gradient re-formed from the mask (one gradient operand) or written (two); thin kernels and igemm
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C,hw,go2", [(16, (24, 40), False), (16, (20, 36), True), (32, (24, 40), False), (32, (20, 36), True),
                                     (64, (24, 40), False), (64, (20, 36), True)])
def test_identity_block(monkeypatch, dt, C, hw, go2):
    _finish("identity %d go2=%d" % (C, go2), dt, S.block_case(monkeypatch, dt, DEV, C, C, 1, hw, go2=go2))


# projection blocks: bypass conv, redb, the 1x1 data gradient added onto g_x in place, the phased stride-2 data gradient
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin,cout,stride,hw", [(16, 32, 1, (20, 36)), (32, 64, 2, (24, 40))])
def test_projection_block(monkeypatch, dt, cin, cout, stride, hw):
    _finish("projection %d->%d s%d" % (cin, cout, stride), dt, S.block_case(monkeypatch, dt, DEV, cin, cout, stride, hw))


@pytest.mark.parametrize("dt", DTS)
def test_block_with_virtual_input(monkeypatch, dt):
    """32 -> 32 with a bypass (stride 2) and an input affine: rec.xf_in must reach conv1, the bypass and both weight gradients"""
    _finish("virtual input 32->32 s2", dt, S.block_case(monkeypatch, dt, DEV, 32, 32, 2, (24, 40), virtual=True))


@pytest.mark.parametrize("dt", DTS)
def test_block_separate_finalize(monkeypatch, dt):
    """_FIN_MAX_C lowered to 16 for one 32 -> 32 block: the separate finalize + apply branch of the tail and of bn1"""
    _finish("separate finalize 32", dt, S.block_case(monkeypatch, dt, DEV, 32, 32, 1, (20, 36), fin_max=16))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cin,cout,stride", [(16, 16, 1), (32, 64, 2)])
def test_block_eval_forward(monkeypatch, dt, cin, cout, stride):
    """eval mode: bn_eval_affine at every site and the plain tail"""
    _finish("eval %d->%d s%d" % (cin, cout, stride), dt,
            S.block_case(monkeypatch, dt, DEV, cin, cout, stride, (24, 40), training=False, backward=False))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("need_gx", [True, False])
def test_double_resnet(monkeypatch, dt, need_gx):
    _finish("double 32->64 s2 gx=%d" % need_gx, dt, S.double_case(monkeypatch, dt, DEV, 32, 64, 2, (24, 40), need_gx=need_gx))


@pytest.mark.parametrize("dt", DTS)
def test_conv_transpose_layer(monkeypatch, dt):
    """64 -> up 32 + skip 32 -> 32: the four-phase deconv into channels [0, 32) of a buffer whose skip half is filled, four phase
    weight gradients into one dW, g_cat[..., 32:] left as the block wrote it"""
    r = S.declayer_case(monkeypatch, dt, DEV, 64, 32, 32, 32, (12, 20))
    _finish("deconv layer 64->32+32->32", dt, r)


# BatchNorm modules in eval mode inside a training pass: every site of the tail frozen -> the one-pass backward (and, on an identity
# block, the skip gradient re-formed from the mask); one of two -> the two passes with k1 = k2 = 0 at the frozen site
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name,cfg,freeze", [("all frozen identity 32", (32, 32, 1, (20, 36)), ("bn1", "bn2")),
                                             ("all frozen 16->32", (16, 32, 1, (20, 36)), ("bn1", "bn2", "bnpass")),
                                             ("mixed: bn2 frozen 16->32", (16, 32, 1, (20, 36)), ("bn2",)),
                                             ("mixed: bnpass frozen 32->64 s2", (32, 64, 2, (24, 40)), ("bnpass",))])
def test_block_with_frozen_sites(monkeypatch, dt, name, cfg, freeze):
    cin, cout, stride, hw = cfg
    _finish(name, dt, S.block_case(monkeypatch, dt, DEV, cin, cout, stride, hw, freeze=freeze))


@pytest.mark.parametrize("dt", DTS)
def test_aspp_level(monkeypatch, dt):
    """128 channels (8 x inplanes, the narrowest level ASPP_ResNet builds): d1 / d3 / d5 branches into channel slices of the concat
    buffer, the stride-1 max-pool beside them, the 1x1 over the virtual concat, and their backward into one g_e"""
    _finish("aspp level 128", dt, S.aspp_case(monkeypatch, dt, DEV, 128, (20, 36)))


@pytest.mark.parametrize("kind", S.MUTATIONS)
def test_corrupted_tape_is_rejected(monkeypatch, kind):
    """the recorded tape of a real projection block with ONE record changed (the launches are not touched): the checks fail"""
    r = S.block_case(monkeypatch, torch.bfloat16, DEV, 16, 32, 1, (20, 36))
    S.check_all(r)
    tape, what = S.mutate(r["tape"], kind)
    with pytest.raises(AssertionError):
        r["graph"].match(tape)
    if kind in ("swap_bn2_bnpass", "xf_identity", "swap_red"):     # values changed too: the replay alone sees it
        with pytest.raises(AssertionError):
            S.replay(tape)
    print("mutation %-18s (%s): rejected" % (kind, what))
