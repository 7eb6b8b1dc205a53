"""The region-loss library without a GPU: libubresnet_dice.so's header is C99; header, binding, reference and library agree on the
entry points, the geometry, the workspace row and the control block; the library holds exactly its thirteen kernels; every
argument refusal returns UBK_EINVAL with a message before any launch; tests/dice_ref.py against torch.autograd on the plain fp64
composite; the arithmetic header as a stand-alone host program against dice_ref over its edge cases; the refusals of
PixelWiseDiceLoss and WeightedSumLoss that need no device."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dice_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_dice.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib  # noqa: E402
from ubresnet_amd import _dice as K  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402

LIB = B.LIBS["dice"].out


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_dice.h"\n'
                     'int main(void) {\n'
                     '  int (*f)(const float*, const int64_t*, const float*, const float*, int, int, int, int, int64_t, float, float, float, int,\n'
                     '           void*, void*, float*, void*) = ubk_dice_fwd;\n'
                     '  int (*b)(const float*, const void*, const float*, const int64_t*, const float*, int, int, int, int, int64_t, float*,\n'
                     '           void*) = ubk_dice_bwd;\n'
                     '  const char* (*e)(void) = ubk_last_error;\n'
                     '  int (*v)(void) = ubk_version;\n'
                     '  return f == 0 || b == 0 || e == 0 || v == 0 || UBK_OK != 0 || UBK_EINVAL != -1 || UBK_ELAUNCH != -2;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ubk_[a-z_0-9]+)\s*\(", text))
    need_lib(LIB)
    assert declared == set(K.SYMBOLS) and len(K.SYMBOLS) == len(set(K.SYMBOLS)) == 4
    num = {k: int(v) for k, v in re.findall(r"#define\s+UBK_([A-Z_0-9]+)\s+\(?(-?\d+)\)?\s", text)}
    assert dict(BLOCK=num["BLOCK"], UNROLL=num["UNROLL"], MAX_GRID=num["MAX_GRID"]) == dict(BLOCK=K.BLOCK, UNROLL=K.UNROLL, MAX_GRID=K.MAX_GRID)
    assert (K.BLOCK, K.UNROLL, K.MAX_GRID, K.TRIP_PIXELS, K.MAX_CLASSES, K.REG_CLASSES) \
        == (R.BLOCK, R.UNROLL, R.MAX_GRID, R.TRIP_PIXELS, R.MAX_CLASSES, R.REG_CLASSES)
    assert num["MAX_CLASSES"] == K.MAX_CLASSES == 16 and num["REG_CLASSES"] == K.REG_CLASSES == 4
    assert num["ROW_WORDS"] == K.ROW_WORDS == 4 * 16 + 2 and num["CTL_WORDS"] == K.CTL_WORDS == K.ROW_WORDS + 3 * 16 + 2
    assert {k: num["CTL_" + k] for k in K.CTL} == K.CTL and {k: num["ROW_" + k] for k in K.ROW} == K.ROW
    assert all(K.CTL[k] == K.ROW[k] for k in K.ROW), "the first words of the control block are the row words"
    assert K.WORKSPACE_BYTES == K.MAX_GRID * K.ROW_WORDS * 8 and K.CTL_BYTES == 928
    assert [K.grid(n) for n in (1, K.TRIP_PIXELS, K.TRIP_PIXELS + 1, K.TRIP_PIXELS * K.MAX_GRID + 5)] == [1, 1, 2, K.MAX_GRID] \
        == [R.grid(n) for n in (1, R.TRIP_PIXELS, R.TRIP_PIXELS + 1, R.TRIP_PIXELS * R.MAX_GRID + 5)]
    # the arithmetic and the contracts are stated in the header
    for phrase in ("expm1f", "expf(lp_c)", "not contracted", "NaN", "Dn_c == 0", "S == 0", "present_only", "no atomic", "4 C + 12", "8 C + 12",
                   "the other channels stay finite", "lp = -inf"):
        assert phrase in raw, phrase
    # thirteen kernels: the forward for C = 1 .. 4 and for the runtime C, in both forms; the finish; both forms of the backward
    want = ["dice_fwd_kernel<%d, %s>" % (c, v) for c in range(K.REG_CLASSES + 1) for v in ("false", "true")]
    want += ["dice_bwd_kernel<false>", "dice_bwd_kernel<true>", "dice_finish_kernel"]
    assert sorted(kernel_symbols.kernels(LIB)) == sorted(want)
    # no atomic operation anywhere in the source, nor in any header of csrc/ that it includes
    files = [os.path.join(B.CSRC, f) for f in B.LIBS["dice"].sources + B.LIBS["dice"].headers if not f.startswith("..")]
    assert sorted(os.path.basename(f) for f in files) == ["ubr_dice.hip", "ubr_dice_term.h", "ubr_rows.h", "ubr_sat.h"]
    for f in files:
        assert "atomic" not in re.sub(r"//.*", "", open(f).read()), f


def test_read_ctl_unpacks_the_words():
    words = np.zeros(K.CTL_WORDS, dtype="<f8")
    words[K.CTL["TP"] + 1], words[K.CTL["FP"] + 2], words[K.CTL["FN"] + 15], words[K.CTL["T"] + 3], words[K.CTL["S"]] = 1.5, 2.5, 3.5, 0.75, 2.0
    u = words.view("<u8")
    u[K.CTL["PIXELS"] + 4], u[K.CTL["VALID"]], u[K.CTL["BAD"]] = 9, 7, 3
    u[K.CTL["K1"] + 5] = int(np.float32(-0.25).view(np.uint32))
    u[K.CTL["K0"] + 15] = int(np.float32(0.125).view(np.uint32))
    u[K.CTL["LOSS"]] = int(np.float32(0.75).view(np.uint32))
    c = K.read_ctl(words.tobytes())
    assert (c["tp"][1], c["fp"][2], c["fn"][15], c["T"][3], c["S"], c["pixels"][4], c["valid"], c["bad"]) == (1.5, 2.5, 3.5, 0.75, 2.0, 9, 7, 3)
    assert (c["k1"][5], c["k0"][15], c["loss"]) == (-0.25, 0.125, 0.75)
    assert all(len(c[k]) == 16 for k in ("tp", "fp", "fn", "pixels", "T", "k1", "k0"))


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------------------------------
# addresses that are never dereferenced: every call below is refused on the host, before any launch.  2 x 3 x 4 x 4: g_predict is
# 384 bytes, target 256, pixelweights 128
_P = 0x100000
_A = dict(predict=_P, target=_P + 0x1000, pw=_P + 0x2000, classw=_P + 0x3000, ws=_P + 0x100000, ctl=_P + 0x4000, loss=_P + 0x5000,
          g_loss=_P + 0x6000, g=_P + 0x7000, N=2, C=3, H=4, W=4, ign=-100, alpha=0.5, beta=0.5, eps=1.0, present=1)
_SHARED = {
    "null predict": (dict(predict=None), "null pointer (predict"),
    "null target": (dict(target=None), "null pointer (predict"),
    "null pixelweights": (dict(pw=None), "null pointer (predict"),
    "N 0": (dict(N=0), "bad extents N=0"),
    "H negative": (dict(H=-4), "bad extents"),
    "W 0": (dict(W=0), "bad extents"),
    "C 0": (dict(C=0), "C=0 must be in [1, 16]"),
    "C 17": (dict(C=17), "C=17 must be in [1, 16]"),
    "predict alignment": (dict(predict=_P + 2), "4-byte aligned"),
    "target alignment": (dict(target=_P + 0x1004), "8-byte aligned"),
    "pixelweights alignment": (dict(pw=_P + 0x2001), "4-byte aligned"),
}
_FWD = {
    "null workspace": (dict(ws=None), "null pointer (workspace"),
    "null ctl": (dict(ctl=None), "null pointer (workspace"),
    "null loss": (dict(loss=None), "null pointer (workspace"),
    "alpha negative": (dict(alpha=-0.5), "alpha=-0.5 must be finite and >= 0"),
    "alpha inf": (dict(alpha=float("inf")), "alpha=inf must be finite and >= 0"),
    "alpha NaN": (dict(alpha=float("nan")), "alpha="),
    "beta negative": (dict(beta=-1.0), "beta=-1 must be finite and >= 0"),
    "beta inf": (dict(beta=float("inf")), "beta=inf must be finite and >= 0"),
    "beta NaN": (dict(beta=float("nan")), "beta="),
    "eps negative": (dict(eps=-1e-6), "eps=-1e-06 must be finite and >= 0"),
    "eps inf": (dict(eps=float("inf")), "eps=inf must be finite and >= 0"),
    "eps NaN": (dict(eps=float("nan")), "eps="),
    "present_only 2": (dict(present=2), "present_only=2 must be 0 or 1"),
    "classw alignment": (dict(classw=_P + 0x3002), "classw must be 4-byte aligned"),
    "workspace alignment": (dict(ws=_P + 0x100008), "workspace must be 16-byte aligned"),
    "ctl alignment": (dict(ctl=_P + 0x4004), "ctl must be 8-byte aligned"),
    "loss alignment": (dict(loss=_P + 0x5002), "loss 4-byte aligned"),
    "ctl inside the workspace": (dict(ctl=_P + 0x100000 + 64), "ctl overlaps workspace"),
    "ctl ends inside the workspace": (dict(ctl=_P + 0x100000 - 8), "ctl overlaps workspace"),
    "loss inside the workspace": (dict(loss=_P + 0x100000 + K.WORKSPACE_BYTES - 4), "loss inside workspace"),
    "loss inside ctl": (dict(loss=_P + 0x4000 + 48), "loss inside ctl"),
}
_BWD = {
    "null g_loss": (dict(g_loss=None), "null pointer (g_loss"),
    "null ctl": (dict(ctl=None), "null pointer (g_loss"),
    "null g_predict": (dict(g=None), "null pointer (g_loss"),
    "ctl alignment": (dict(ctl=_P + 0x4004), "ctl must be 8-byte aligned"),
    "g_loss alignment": (dict(g_loss=_P + 0x6001), "4-byte aligned"),
    "g_predict alignment": (dict(g=_P + 0x7002), "4-byte aligned"),
    "g_predict is predict": (dict(g=_P), "g_predict overlaps predict"),
    "g_predict starts inside predict": (dict(g=_P + 380), "g_predict overlaps predict"),
    "g_predict ends inside target": (dict(g=_P + 0x1000 - 380), "g_predict overlaps"),
    "g_predict inside pixelweights": (dict(g=_P + 0x2000 + 124), "g_predict overlaps pixelweights"),
    "ctl inside g_predict": (dict(ctl=_P + 0x7000 + 376), "g_predict overlaps ctl"),
    "g_loss inside g_predict": (dict(g_loss=_P + 0x7000 + 380), "g_predict overlaps g_loss"),
}
_BAD = {"fwd: %s" % k: ("fwd", c, m) for k, (c, m) in list(_SHARED.items()) + list(_FWD.items())}
_BAD.update({"bwd: %s" % k: ("bwd", c, m) for k, (c, m) in list(_SHARED.items()) + list(_BWD.items())})
_ENTRY = dict(fwd="ubk_dice_fwd", bwd="ubk_dice_bwd")


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    which, change, message = _BAD[name]
    a = dict(_A)
    a.update(change)
    lib = K.lib()
    if which == "fwd":
        rc = lib.ubk_dice_fwd(a["predict"], a["target"], a["pw"], a["classw"], a["N"], a["C"], a["H"], a["W"], a["ign"], a["alpha"], a["beta"],
                              a["eps"], a["present"], a["ws"], a["ctl"], a["loss"], None)
    else:
        rc = lib.ubk_dice_bwd(a["g_loss"], a["ctl"], a["predict"], a["target"], a["pw"], a["N"], a["C"], a["H"], a["W"], a["ign"], a["g"], None)
    msg = lib.ubk_last_error().decode()
    assert rc == -1 and msg.startswith(_ENTRY[which]) and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=_ENTRY[which]):
        K.check(rc, name)


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def _operands(seed=0, N=2, C=4, H=5, W=7, ignore_index=-100):
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(3.0 * torch.randn(N, C, H, W, generator=g, dtype=torch.float64), dim=1)
    target = torch.randint(0, C - 1, (N, H, W), generator=g)              # class C - 1 is absent
    target[0, 0, :3] = ignore_index
    target[1, 2, 4] = ignore_index
    pw = torch.rand(N, H, W, generator=g, dtype=torch.float64) + 0.25
    cw = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    return lp, target, pw, cw


def _composite(x, target, pw, cw, alpha, beta, eps, present_only):
    """the expression a user would write with torch: one-hot masks, sums over the batch, the class-weighted mean of 1 - T"""
    C = x.shape[1]
    ok = (target != -100).unsqueeze(1).double()
    onehot = torch.nn.functional.one_hot(target.clamp(0), C).permute(0, 3, 1, 2).double()
    p = x.exp()
    w = pw.unsqueeze(1) * ok
    tp = (w * p * onehot).sum(dim=(0, 2, 3))
    fp = (w * p * (1 - onehot)).sum(dim=(0, 2, 3))
    fn = (w * (1 - p) * onehot).sum(dim=(0, 2, 3))
    T = (tp + eps) / (tp + alpha * fp + beta * fn + eps)
    present = ((onehot * ok).sum(dim=(0, 2, 3)) > 0).double() if present_only else torch.ones(C, dtype=torch.float64)
    a = cw * present / (cw * present).sum()
    return (a * (1 - T)).sum(), tp, fp, fn, T


@pytest.mark.parametrize("present_only", [True, False])
@pytest.mark.parametrize("alpha,beta,eps", [(0.5, 0.5, 1.0), (0.3, 0.7, 1e-6), (0.0, 1.0, 1.0), (1.0, 0.0, 0.25)])
def test_reference_is_the_autograd_of_the_fp64_composite(alpha, beta, eps, present_only):
    lp, target, pw, cw = _operands(int(100 * alpha) + int(present_only))
    cw = cw.float().double()
    a32, b32, e32 = (float(np.float32(v)) for v in (alpha, beta, eps))
    x = lp.clone().requires_grad_(True)
    loss, tp, fp, fn, T = _composite(x, target, pw, cw, a32, b32, e32, present_only)
    loss.backward()
    f = R.forward(lp.numpy(), target.numpy(), pw.numpy(), cw.numpy(), -100, alpha, beta, eps, present_only)
    assert f["valid"] == int((target != -100).sum()) and f["bad"] == 0 and f["pixels"][3] == 0 and bool(f["present"][3]) == (not present_only)
    for got, want in ((f["tp"], tp), (f["fp"], fp), (f["fn"], fn), (f["T"], T)):
        assert np.abs(got - want.detach().numpy()).max() <= 1e-12 * max(1.0, float(want.detach().abs().max()))
    assert abs(f["loss"] - float(loss)) <= 1e-12
    g, lim, ok = R.backward(1.0, f)
    want = x.grad.numpy()
    assert np.abs(g - want).max() <= 1e-12 * np.abs(want).max() and np.abs(want).max() > 0
    assert (g[~np.broadcast_to(ok[:, None], g.shape)] == 0).all() and (lim[np.broadcast_to(ok[:, None], g.shape)] > 0).all()
    assert np.isfinite(lim).all() and np.isfinite(f["lim_loss"]) and f["lim_loss"] < 1e-5 and (lim <= 1e-5 * np.abs(g).max() + 1e-30).all()


def test_reference_edge_rules():
    lp, target, pw, cw = _operands(3)
    target[1, 0, 0], target[1, 0, 1] = 9, -3                                     # labels out of range: counted, no contribution
    f = R.forward(lp.numpy(), target.numpy(), pw.numpy(), None, -100)
    assert f["bad"] == 2 and f["valid"] == int(((target >= 0) & (target < 4)).sum())
    # soft Dice is (2 TP + 2 eps) / (2 TP + FP + FN + 2 eps)
    assert np.allclose(f["T"], (2 * f["tp"] + 2) / (2 * f["tp"] + f["fp"] + f["fn"] + 2), rtol=1e-14)
    # TP + FN is the weighted pixel count of the class
    assert np.allclose(f["tp"] + f["fn"], f["weighted_pixels"], rtol=1e-12)
    # an absent class without eps and without a price on false positives: Dn == 0 -> T = 1, coefficients 0, nothing is NaN
    f0 = R.forward(lp.numpy(), target.numpy(), pw.numpy(), None, -100, 0.0, 1.0, 0.0, False)
    assert f0["T"][3] == 1.0 and f0["K1"][3] == 0.0 and f0["K0"][3] == 0.0 and f0["lim_T"][3] == 0.0 and math.isfinite(f0["loss"])
    # nothing contributes: S == 0 under present_only, loss 0, gradient 0
    target[:] = -100
    fz = R.forward(lp.numpy(), target.numpy(), pw.numpy(), cw.numpy(), -100)
    g, lim, ok = R.backward(1.0, fz)
    assert fz["S"] == 0.0 and fz["loss"] == 0.0 and not g.any() and not ok.any() and not fz["K1"].any() and not fz["K0"].any()
    # all class weights zero
    fw = R.forward(lp.numpy(), _operands(3)[1].numpy(), pw.numpy(), np.zeros(4, np.float32), -100)
    assert fw["S"] == 0.0 and fw["loss"] == 0.0 and not fw["K1"].any() and not fw["K0"].any() and fw["T"][0] > 0


# ------------------------------------------------------------------------------------------------------------------------
# the arithmetic header as a program
# ------------------------------------------------------------------------------------------------------------------------
def _hex(s):
    return float.fromhex(s) if s.lstrip("-") not in ("nan", "inf") else float(s.lstrip("-") if "nan" in s else s)


def test_arithmetic_as_a_host_program_matches_the_reference(tmp_path):
    """tests/dice_host.cpp has its own main and includes ubr_dice_term.h; built with -ffp-contract=off, as the library is, and run
    as a process of its own.  lp over {0, -0.0, -1e-30, -1e-45, -104, -110, -inf, NaN, below the underflow of expf} and ordinary
    values, pw over {0.5, 2, a subnormal, 0}: the addends and the gradient against dice_ref within its bound; then the finish rule"""
    exe = str(tmp_path / "dice_host")
    r = subprocess.run([cc(plus=True), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                        "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "dice_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [l.replace("|", " ").split() for l in p.stdout.strip().split("\n")]
    P = [[_hex(v) for v in row[1:]] for row in rows if row[0] == "P"]
    F = [[_hex(v) for v in row[1:]] for row in rows if row[0] == "F"]
    assert len(P) == 13 * 4 and len(F) == 13
    seen, worst = set(), 0.0
    for lp, pw, s, k, hit, lost, grad in P:
        what = "lp=%r pw=%r" % (lp, pw)
        seen.add(("nan" if math.isnan(lp) else lp, pw))
        if math.isnan(lp):
            assert math.isnan(hit) and math.isnan(lost) and math.isnan(grad), what       # a NaN log-probability poisons every sum it enters
            continue
        with np.errstate(all="ignore"):
            want_hit, want_lost, want_g = pw * math.exp(lp) if lp > -800 else 0.0, pw * float(R.miss(lp)), s * (math.exp(lp) if lp > -800 else 0.0) * k
        if math.isinf(lp):
            assert hit == 0.0 and lost == pw and grad == 0.0, what                     # lp = -inf: p = 0, q = 1, all finite
            continue
        lim_hit, lim_lost = float(R.term_bound(want_hit, pw)), float(R.term_bound(want_lost, pw))
        lim_g = R.C_ACC * R.U32 * R.GRAD_U * abs(want_g) + R.FLOOR * max(1.0, abs(s)) * max(1.0, abs(k))
        assert abs(hit - want_hit) <= lim_hit and hit >= 0.0, "%s: hit %r, reference %r, bound %r" % (what, hit, want_hit, lim_hit)
        assert abs(lost - want_lost) <= lim_lost and 0.0 <= lost <= pw, "%s: lost %r, reference %r, bound %r" % (what, lost, want_lost, lim_lost)
        assert abs(grad - want_g) <= lim_g, "%s: grad %r, reference %r, bound %r" % (what, grad, want_g, lim_g)
        if lp == 0.0:
            assert hit == pw and lost == 0.0 and grad == s * k, what
        if lp <= -104.0:
            assert hit == 0.0 and lost == pw, what                                     # below the underflow of expf
        worst = max([worst] + [abs(a - b) / l for a, b, l in ((hit, want_hit, lim_hit), (lost, want_lost, lim_lost), (grad, want_g, lim_g))])
    f32 = lambda v: float(np.float32(v))                                             # noqa: E731
    assert {(0.0, 0.5), (f32(-1e-30), 2.0), (f32(-1e-45), 0.5), (-104.0, 0.5), (-110.0, 2.0), (-math.inf, 0.5), ("nan", 0.5), (-5.0, f32(1e-40)),
            (-88.5, 0.5), (-5.0, 0.0)} <= seen
    assert 0.0 < worst <= 1.0
    # the finish rule against the reference's, class by class (C = 1 with the class weight folded into a)
    for live, a, tp, fp, fn, alpha, beta, eps, T, term, k1, k0 in F:
        what = (live, a, tp, fp, fn, alpha, beta, eps)
        if live and (math.isnan(tp) or math.isnan(fp)):
            assert math.isnan(T) and math.isnan(term) and math.isnan(k1) and math.isnan(k0), what      # also where a == 0
            continue
        if not live:
            assert term == 0.0 and k1 == 0.0 and k0 == 0.0 and (math.isnan(T) if math.isnan(tp) else 0.0 < T < 1.0), what
            continue
        r = R.finish([tp], [fp], [fn], [1], None, alpha, beta, eps, False)
        assert abs(T - r["T"][0]) <= 4 * 2.0 ** -53 * T and abs(term - a * (1.0 - r["T"][0])) <= 1e-15, what
        for got, want in ((k1, a * r["K1"][0]), (k0, a * r["K0"][0])):
            assert abs(got - want) <= (R.U32 + R.E64) * abs(want) + 2.0 ** -149 and math.isfinite(got), (what, got, want)
        assert k1 <= 0.0 <= k0, what
        if tp + alpha * fp + beta * fn + eps == 0.0:
            assert T == 1.0 and term == 0.0 and k1 == 0.0 and k0 == 0.0, what
    assert sum(1 for f in F if f[2] + f[5] * f[3] + f[6] * f[4] + f[7] == 0.0) == 1                       # the Dn == 0 row is there


# ------------------------------------------------------------------------------------------------------------------------
# the modules
# ------------------------------------------------------------------------------------------------------------------------
def test_module_refusals_that_need_no_device():
    import inspect
    from ubresnet_amd import training
    from ubresnet_amd.training import pixelwise_diceloss, pixelwise_nllloss
    from ubresnet_amd.training.pixelwise_diceloss import PixelWiseDiceLoss, WeightedSumLoss
    assert training.PixelWiseDiceLoss is PixelWiseDiceLoss and training.WeightedSumLoss is WeightedSumLoss
    assert pixelwise_diceloss._label_check is pixelwise_nllloss._label_check           # imported, not copied
    sig = inspect.signature(PixelWiseDiceLoss.__init__).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("weight", None), ("alpha", 0.5), ("beta", 0.5), ("eps", 1.0), ("ignore_index", -100),
                                                           ("present_only", True)]
    assert list(inspect.signature(PixelWiseDiceLoss.forward).parameters) == ["self", "predict", "target", "pixelweights"]
    for name in ("alpha", "beta", "eps"):
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="%s must be finite and >= 0" % name):
                PixelWiseDiceLoss(**{name: bad})
    crit = PixelWiseDiceLoss(weight=torch.ones(3), alpha=0.3, beta=0.7, eps=0, present_only=0)
    assert (crit.alpha, crit.beta, crit.eps, crit.ignore_index, crit.present_only) == (0.3, 0.7, 0.0, -100, False) and hasattr(crit, "flush")
    with pytest.raises(RuntimeError, match="no forward yet"):
        crit.read()
    p, t, w = torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.int64), torch.ones(2, 4, 4)
    with pytest.raises(RuntimeError, match="expected predict/pixelweights float32 and target int64"):
        crit(p.double(), t, w)
    with pytest.raises(RuntimeError, match="expected predict/pixelweights float32 and target int64"):
        crit(p, t.int(), w)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        crit(p, t[:, :3], w)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        crit(p, t, w[:1])
    with pytest.raises(RuntimeError, match="shape mismatch"):
        crit(p[0], t, w)
    with pytest.raises(RuntimeError, match="weight has 3 entries for 4 classes"):
        crit(torch.zeros(2, 4, 4, 4), t, w)
    with pytest.raises(RuntimeError, match="17 classes"):
        PixelWiseDiceLoss()(torch.zeros(2, 17, 4, 4), t, w)
    with pytest.raises(AssertionError, match="gradient w.r.t. targets"):
        crit(p, t, w.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(p, t, w)                                                                  # a missing device is an error, not eager torch
    # the sum of criteria
    with pytest.raises(ValueError, match="no parts"):
        WeightedSumLoss([])
    with pytest.raises(ValueError, match="not finite"):
        WeightedSumLoss([(float("nan"), crit)])
    with pytest.raises(ValueError, match="has no forward"):
        WeightedSumLoss([(1.0, object())])

    class Part(torch.nn.Module):
        def __init__(self, scale):
            super(Part, self).__init__()
            self.scale, self.flushed = scale, 0

        def forward(self, predict, target, pixelweights):
            return self.scale * (predict * pixelweights.unsqueeze(1)).sum()

        def flush(self):
            self.flushed += 1

        def read(self):
            return dict(scale=self.scale)

    a, b = Part(2.0), Part(3.0)
    both = WeightedSumLoss([(1.0, a), (0.5, b)])
    x = torch.ones(2, 3, 4, 4, requires_grad=True)
    loss = both(x, t, w)
    loss.backward()
    assert float(loss) == 96 * 2.0 + 0.5 * 96 * 3.0 and bool((x.grad == 3.5).all())
    both.flush()
    assert (a.flushed, b.flushed) == (1, 1) and both.read() == [(1.0, dict(scale=2.0)), (0.5, dict(scale=3.0))]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        WeightedSumLoss([(1.0, PixelWiseDiceLoss())])(p, t, w)
