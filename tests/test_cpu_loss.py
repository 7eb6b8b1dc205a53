"""The focal-loss library without a GPU: libubresnet_loss.so's header is C99; header, binding, reference and library agree on the
entry points, the geometry, the workspace row and the control block; every argument refusal returns UBL_EINVAL with a message
before any launch; tests/loss_ref.py against torch.autograd on the fp64 composite, against kref's NLL reference and the reference
criterion's semantics at gamma = 0, and against torch's weighted mean; the arithmetic header as a stand-alone program under the
host sanitizers against loss_ref over its edge cases; PixelWiseFocalLoss's refusals that need no device."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import kref
import loss_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ubresnet_loss.h")
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_symbols  # noqa: E402
from cpu_helpers import cc, need_lib  # noqa: E402
from ubresnet_amd import _loss as K  # noqa: E402
from ubresnet_amd import build as B  # noqa: E402

LIB = B.LIBS["loss"].out
GAMMAS = [0.5, 1.0, 2.0, 5.0]


# ------------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    proto = tmp_path / "p.c"
    proto.write_text('#include "ubresnet_loss.h"\n'
                     'int main(void) {\n'
                     '  int (*f)(const float*, const int64_t*, const float*, const float*, int, int, int, int, int64_t, float, int, void*, void*,\n'
                     '           float*, void*) = ubl_focal_fwd;\n'
                     '  int (*b)(const float*, const void*, const float*, const int64_t*, const float*, const float*, int, int, int, int, int64_t,\n'
                     '           float, float*, void*) = ubl_focal_bwd;\n'
                     '  const char* (*e)(void) = ubl_last_error;\n'
                     '  int (*v)(void) = ubl_version;\n'
                     '  return f == 0 || b == 0 || e == 0 || v == 0 || UBL_OK != 0 || UBL_EINVAL != -1 || UBL_ELAUNCH != -2;\n}\n')
    r = subprocess.run([cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(proto)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_reference_and_library_agree():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ubl_[a-z_0-9]+)\s*\(", text))
    need_lib(LIB)
    assert declared == set(K.SYMBOLS) and len(K.SYMBOLS) == len(set(K.SYMBOLS)) == 4
    num = {k: int(v) for k, v in re.findall(r"#define\s+UBL_([A-Z_]+)\s+\(?(-?\d+)\)?\s", text)}
    assert dict(BLOCK=num["BLOCK"], UNROLL=num["UNROLL"], MAX_GRID=num["MAX_GRID"]) == dict(BLOCK=K.BLOCK, UNROLL=K.UNROLL, MAX_GRID=K.MAX_GRID)
    assert (K.BLOCK, K.UNROLL, K.MAX_GRID, K.TRIP_PIXELS, K.MAX_CLASSES) == (R.BLOCK, R.UNROLL, R.MAX_GRID, R.TRIP_PIXELS, R.MAX_CLASSES)
    assert num["MAX_CLASSES"] == K.MAX_CLASSES == 16 and num["ROW_WORDS"] == K.ROW_WORDS == 4 + 2 * 16 and num["CTL_WORDS"] == K.CTL_WORDS == 40
    assert {k: num["CTL_" + k] for k in K.CTL} == K.CTL and {k: num["ROW_" + k] for k in K.ROW} == K.ROW
    assert (num["MEAN_PIXELS"], num["MEAN_VALID"], num["MEAN_WEIGHTS"]) == (K.MEAN_PIXELS, K.MEAN_VALID, K.MEAN_WEIGHTS) == (0, 1, 2)
    assert [K.MODES[m] for m in R.MODES] == [0, 1, 2]
    assert K.WORKSPACE_BYTES == K.MAX_GRID * K.ROW_WORDS * 8 and K.CTL_BYTES == 320
    assert [K.grid(n) for n in (1, K.TRIP_PIXELS, K.TRIP_PIXELS + 1, K.TRIP_PIXELS * K.MAX_GRID + 5)] == [1, 1, 2, K.MAX_GRID] \
        == [R.grid(n) for n in (1, R.TRIP_PIXELS, R.TRIP_PIXELS + 1, R.TRIP_PIXELS * R.MAX_GRID + 5)]
    # the arithmetic and the contracts are stated in the header
    for phrase in ("expm1f", "exp2f(gamma * log2f(q))", "contracted", "NaN", "nll_bwd_kernel", "denom == 0", "bit for bit", "no atomic"):
        assert phrase in raw, phrase
    # five kernels: both forms of the two streaming passes, and the finish
    assert sorted(kernel_symbols.kernels(LIB)) == ["focal_bwd_kernel<false>", "focal_bwd_kernel<true>", "focal_finish_kernel",
                                                   "focal_fwd_kernel<false>", "focal_fwd_kernel<true>"]
    # no atomic operation anywhere in the source, nor in any header of csrc/ that it includes
    files = [os.path.join(B.CSRC, f) for f in B.LIBS["loss"].sources + B.LIBS["loss"].headers if not f.startswith("..")]
    assert sorted(os.path.basename(f) for f in files) == ["ubr_loss.hip", "ubr_loss_term.h", "ubr_rows.h", "ubr_sat.h"]
    for f in files:
        assert "atomic" not in re.sub(r"//.*", "", open(f).read()), f


def test_read_ctl_unpacks_the_words():
    words = np.zeros(K.CTL_WORDS, dtype="<f8")
    words[K.CTL["LOSS_SUM"]], words[K.CTL["WEIGHT_SUM"]], words[K.CTL["DENOM"]] = 1.5, 2.5, 7.0
    u = words.view("<u8")
    u[K.CTL["VALID"]], u[K.CTL["BAD"]], u[K.CTL["MODE"]] = 7, 3, 1
    u[K.CTL["INV_DENOM"]] = int(np.float32(0.25).view(np.uint32))
    u[K.CTL["LOSS"]] = int(np.float32(0.75).view(np.uint32))
    words[K.CTL["CLASS_LOSS"] + 2] = 4.0
    u[K.CTL["CLASS_PIXELS"] + 15] = 9
    c = K.read_ctl(words.tobytes())
    assert (c["loss_sum"], c["weight_sum"], c["valid"], c["bad"], c["denom"], c["inv_denom"], c["loss"], c["mode"]) == (1.5, 2.5, 7, 3, 7.0, 0.25, 0.75, 1)
    assert c["class_loss"][2] == 4.0 and c["class_pixels"][15] == 9 and len(c["class_loss"]) == len(c["class_pixels"]) == 16


# ------------------------------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------------------------------
# addresses that are never dereferenced: every call below is refused on the host, before any launch.  2 x 3 x 4 x 4: g_predict is
# 384 bytes, target 256, pixelweights 128
_P = 0x100000
_A = dict(predict=_P, target=_P + 0x1000, pw=_P + 0x2000, classw=_P + 0x3000, ws=_P + 0x100000, ctl=_P + 0x4000, loss=_P + 0x5000,
          g_loss=_P + 0x6000, g=_P + 0x7000, N=2, C=3, H=4, W=4, ign=-100, gamma=2.0, mode=0)
_SHARED = {
    "null predict": (dict(predict=None), "null pointer (predict"),
    "null target": (dict(target=None), "null pointer (predict"),
    "null pixelweights": (dict(pw=None), "null pointer (predict"),
    "N 0": (dict(N=0), "bad extents N=0"),
    "H negative": (dict(H=-4), "bad extents"),
    "W 0": (dict(W=0), "bad extents"),
    "C 0": (dict(C=0), "C=0 must be in [1, 16]"),
    "C 17": (dict(C=17), "C=17 must be in [1, 16]"),
    "gamma negative": (dict(gamma=-0.5), "finite and >= 0"),
    "gamma inf": (dict(gamma=float("inf")), "finite and >= 0"),
    "gamma NaN": (dict(gamma=float("nan")), "gamma is NaN"),
    "predict alignment": (dict(predict=_P + 2), "4-byte aligned"),
    "target alignment": (dict(target=_P + 0x1004), "8-byte aligned"),
    "pixelweights alignment": (dict(pw=_P + 0x2001), "4-byte aligned"),
    "classw alignment": (dict(classw=_P + 0x3002), "4-byte aligned"),
}
_FWD = {
    "null workspace": (dict(ws=None), "null pointer (workspace"),
    "null ctl": (dict(ctl=None), "null pointer (workspace"),
    "null loss": (dict(loss=None), "null pointer (workspace"),
    "mode 3": (dict(mode=3), "unknown mode 3"),
    "mode negative": (dict(mode=-1), "unknown mode -1"),
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
_ENTRY = dict(fwd="ubl_focal_fwd", bwd="ubl_focal_bwd")


@pytest.mark.parametrize("name", sorted(_BAD))
def test_argument_refusals_precede_any_launch(name):
    need_lib(LIB)
    which, change, message = _BAD[name]
    a = dict(_A)
    a.update(change)
    lib = K.lib()
    if which == "fwd":
        rc = lib.ubl_focal_fwd(a["predict"], a["target"], a["pw"], a["classw"], a["N"], a["C"], a["H"], a["W"], a["ign"], a["gamma"], a["mode"],
                               a["ws"], a["ctl"], a["loss"], None)
    else:
        rc = lib.ubl_focal_bwd(a["g_loss"], a["ctl"], a["predict"], a["target"], a["pw"], a["classw"], a["N"], a["C"], a["H"], a["W"], a["ign"],
                               a["gamma"], a["g"], None)
    msg = lib.ubl_last_error().decode()
    assert rc == -1 and msg.startswith(_ENTRY[which]) and message in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=_ENTRY[which]):
        K.check(rc, name)


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def _operands(seed=0, N=2, C=4, H=5, W=7, ignore_index=-100):
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(3.0 * torch.randn(N, C, H, W, generator=g, dtype=torch.float64), dim=1)
    target = torch.randint(0, C, (N, H, W), generator=g)
    target[0, 0, :3] = ignore_index
    target[1, 2, 4] = ignore_index
    pw = torch.rand(N, H, W, generator=g, dtype=torch.float64) + 0.25
    cw = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    return lp, target, pw, cw


@pytest.mark.parametrize("gamma", GAMMAS)
def test_reference_is_the_autograd_of_the_fp64_composite(gamma):
    """the expression a user would write: -(1 - exp(lp))**gamma * lp * w, summed, under torch.autograd"""
    lp, target, pw, cw = _operands(int(10 * gamma))
    x = lp.clone().requires_grad_(True)
    ok = target != -100
    t = target.clamp(0)
    lpt = x.gather(1, t.unsqueeze(1)).squeeze(1)
    w = cw[t] * pw
    terms = torch.where(ok, -(1.0 - torch.exp(lpt)) ** gamma * lpt * w, torch.zeros((), dtype=torch.float64))
    for mode in R.MODES:
        denom = {"pixels": float(target.numel()), "valid": float(ok.sum()), "weights": float((w * ok).sum())}[mode]
        loss = terms.sum() / denom
        x.grad = None
        loss.backward(retain_graph=True)
        f = R.forward(lp.numpy(), target.numpy(), pw.numpy(), cw.numpy(), -100, gamma, mode)
        # (weight_sum is the sum of fp32 products in the reference: compare the denominator at that precision)
        assert f["valid"] == int(ok.sum()) and f["bad"] == 0 and abs(f["denom"] - denom) <= 1e-6 * denom
        assert abs(f["loss_sum"] - float(terms.detach().sum())) <= 1e-12 * float(terms.detach().abs().sum())
        f["denom"] = denom
        g, lim, hot = R.backward(1.0, f, gamma, lp.shape[1])
        want = x.grad.numpy()
        assert np.abs(g - want).max() <= 1e-12 * np.abs(want).max() and np.count_nonzero(want) == int(ok.sum())
        assert (g[~hot] == 0).all() and hot.sum() == int(ok.sum()) and (lim[hot] > 0).all() and (lim[~hot] == 0).all()
    # the per-class by-products
    for c in range(lp.shape[1]):
        sel = ok & (t == c)
        assert f["class_pixels"][c] == int(sel.sum()) and abs(f["class_loss"][c] - float(terms.detach()[sel].sum())) <= 1e-12 * float(terms.detach().abs().sum())


def test_reference_at_gamma_0_is_the_nll_reference_and_the_reference_criterion():
    lp, target, pw, cw = _operands(3)
    target[1, 0, 0], target[1, 0, 1] = 9, -3                                     # labels out of range: counted, no contribution
    for classw in (None, cw):
        s, sabs, bad, ok, w = kref.nll_ref(lp, target, pw, classw, -100)
        f = R.forward(lp.numpy(), target.numpy(), pw.numpy(), None if classw is None else classw.numpy(), -100, 0.0, "pixels")
        assert bad == f["bad"] == 2 and f["valid"] == int(ok.sum()) and (f["ok"] == ok.numpy()).all()
        assert abs(f["loss_sum"] - float(s)) <= 1e-13 * float(sabs) and abs(f["abs_sum"] - float(sabs)) <= 1e-13 * float(sabs)
        assert f["denom"] == float(target.numel()) and abs(f["loss"] - float(s) / target.numel()) <= 1e-15
        # the gradient: kref.nll_bwd_ref rounds g_loss / total to fp32 first; pick a total's reciprocal that is exact: compare at 1e-7
        g, _, _ = R.backward(1.0, f, 0.0, lp.shape[1])
        want = kref.nll_bwd_ref(1.0, target, pw, classw, -100, lp.shape[1]).numpy()
        assert np.abs(g - want).max() <= 2.0 ** -23 * np.abs(want).max()
    # the reference criterion: F.nll_loss(reduction="none") * pixelweights, then torch.mean over all b*h*w pixels
    good = target.clone()
    good[1, 0, 0], good[1, 0, 1] = 1, -100
    per_pixel = torch.nn.functional.nll_loss(lp, good, weight=cw, reduction="none", ignore_index=-100) * pw
    f = R.forward(lp.numpy(), good.numpy(), pw.numpy(), cw.numpy(), -100, 0.0, "pixels")
    assert abs(f["loss"] - float(per_pixel.mean())) <= 1e-14 * abs(float(per_pixel.mean()))


def test_weights_mode_is_torch_nll_loss_with_class_weights():
    lp, target, _, cw = _operands(5)
    ones = torch.ones(target.shape, dtype=torch.float64)
    cw = (cw * 4).round() / 4                                                    # dyadic: the fp32 products of the weight sum are exact
    x = lp.clone().requires_grad_(True)
    want = torch.nn.functional.nll_loss(x, target, weight=cw, reduction="mean", ignore_index=-100)
    want.backward()
    f = R.forward(lp.numpy(), target.numpy(), ones.numpy(), cw.numpy(), -100, 0.0, "weights")
    assert abs(f["loss"] - float(want)) <= 1e-14 * abs(float(want))
    g, _, _ = R.backward(1.0, f, 0.0, lp.shape[1])
    assert np.abs(g - x.grad.numpy()).max() <= 1e-14


def test_the_mean_of_nothing_is_zero():
    lp, target, pw, cw = _operands(7)
    target[:] = -100
    for mode in R.MODES:
        f = R.forward(lp.numpy(), target.numpy(), pw.numpy(), cw.numpy(), -100, 2.0, mode)
        assert f["loss"] == 0.0 and f["valid"] == 0 and f["loss_sum"] == 0.0
        g, lim, hot = R.backward(1.0, f, 2.0, lp.shape[1])
        assert not g.any() and not hot.any()
    assert R.mean("valid", 0.0, 0.0, 0, 72) == (0.0, 0.0, 0.0) and R.mean("weights", 0.0, 0.0, 0, 72) == (0.0, 0.0, 0.0)
    assert R.mean("pixels", 0.0, 0.0, 0, 72)[1] == np.float32(1.0) / np.float32(72.0)


# ------------------------------------------------------------------------------------------------------------------------
# the arithmetic header as a program
# ------------------------------------------------------------------------------------------------------------------------
def _hex(s):
    return float.fromhex(s) if s.lstrip("-") not in ("nan", "inf") else float(s)


def test_arithmetic_as_a_program_under_the_host_sanitizers(tmp_path):
    """tests/loss_host.cpp has its own main and includes ubr_loss_term.h; built with -fsanitize=address,undefined (and
    -ffp-contract=off, as the library is) and run as a process of its own.  lp over {0, -0.0, -1e-30, -1e-45, -104, -110, -inf,
    +1e-3, NaN} and four ordinary values, gamma over {0, 0.01, 0.5, 1, 2, 5}: q, m, term, d and g against loss_ref within its
    bound; then the finish rule, bit for bit"""
    exe = str(tmp_path / "loss_host")
    r = subprocess.run([cc(plus=True), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-Wall", "-Werror", "-I", os.path.join(REPO, "ubresnet_amd", "csrc"), os.path.join(REPO, "tests", "loss_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, "sanitizer or program failure:\n" + p.stderr[-2000:]
    rows = [l.replace("|", " ").split() for l in p.stdout.strip().split("\n")]
    T = [[_hex(v) for v in row[1:]] for row in rows if row[0] == "T"]
    M = [[_hex(v) if "." in v or "x" in v or "n" in v else int(v) for v in row[1:]] for row in rows if row[0] == "M"]
    assert len(T) == 13 * 6 and len(M) == 15
    seen_lp, seen_gamma, worst = set(), set(), {}
    for lp, gamma, w_c, pw, s, q, m, term, d, g in T:
        seen_gamma.add(gamma)
        seen_lp.add("nan" if math.isnan(lp) else lp)
        gam = float(np.float32(gamma))
        what = "lp=%r gamma=%r" % (lp, gamma)
        if math.isnan(lp):
            assert math.isnan(term) and math.isnan(d) and math.isnan(g), what      # a NaN log-probability poisons loss and gradient
            continue
        want_t, lim_t = float(R.term(lp, gam, w_c * pw)), float(R.term_bound(lp, gam, w_c, pw))
        want_d, lim_d = float(R.deriv(lp, gam)), float(R.deriv_bound(lp, gam))
        if math.isinf(lp):
            assert term == math.inf and want_t == math.inf and d == -1.0 == want_d and q == 1.0 and m == 1.0, what
            continue
        assert abs(q - float(R.miss(lp))) <= R.C_ACC * R.U32 * R.LIB * float(R.miss(lp)) + R.FLOOR and 0.0 <= q <= 1.0, what
        assert abs(term - want_t) <= lim_t, "%s: term %r, reference %r, bound %r" % (what, term, want_t, lim_t)
        assert abs(d - want_d) <= lim_d, "%s: d %r, reference %r, bound %r" % (what, d, want_d, lim_d)
        S = s * pw * w_c
        assert abs(g - S * want_d) <= abs(S) * lim_d + R.C_ACC * R.U32 * 3.0 * abs(S * want_d) + R.FLOOR, what
        if gamma == 0.0:
            assert m == 1.0 and d == -1.0 and term == -lp * w_c * pw and g == -s * pw * w_c, what      # the NLL term and gradient, exactly
        if lp >= 0.0 or lp == 0.0:
            assert q == 0.0 and d == -m and (m == (1.0 if gamma == 0.0 else 0.0)), what
        if lp <= -104.0:
            assert q == 1.0 and m == 1.0 and d == -1.0, what                        # below the underflow of expf: c is taken as 0
        for key, got, want, lim in (("term", term, want_t, lim_t), ("d", d, want_d, lim_d)):
            if lim > 0:
                worst[(gamma, key)] = max(worst.get((gamma, key), 0.0), abs(got - want) / lim)
    assert seen_gamma == {0.0, float(np.float32(0.01)), 0.5, 1.0, 2.0, 5.0}
    assert {0.0, float(np.float32(-1e-30)), float(np.float32(-1e-45)), -104.0, -110.0, -math.inf, float(np.float32(1e-3)), "nan"} <= seen_lp
    assert max(worst.values()) <= 1.0 and len(worst) == 12
    # the finish rule
    modes = {0: "pixels", 1: "valid", 2: "weights"}
    for mode, loss_sum, weight_sum, valid, total, denom, inv_denom, loss in M:
        want = R.mean(modes[mode], loss_sum, weight_sum, valid, total)
        got = (denom, np.float32(inv_denom), np.float32(loss))
        assert [float(v).hex() for v in got] == [float(v).hex() for v in want], (mode, loss_sum, weight_sum, valid, total, got, want)
    zero = [m for m in M if m[5] == 0.0]
    assert len(zero) == 2 and all(m[6] == 0.0 and m[7] == 0.0 for m in zero)        # denom == 0: zero loss, zero gradient
    sub = [m for m in M if m[0] == 2 and 0 < m[5] < 2.0 ** -126]
    assert len(sub) == 1 and sub[0][6] == math.inf and math.isfinite(sub[0][7])     # a subnormal weight sum has no fp32 reciprocal
    rounded = [m for m in M if m[0] == 0 and m[4] == 16777217]
    assert rounded[0][6] == 2.0 ** -24                                              # 1.0f / (float)total, as nll_bwd_kernel divides


# ------------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------------
def test_module_refusals_that_need_no_device():
    import inspect
    from ubresnet_amd import training
    from ubresnet_amd.training.pixelwise_focalloss import PixelWiseFocalLoss
    from ubresnet_amd.training import pixelwise_focalloss, pixelwise_nllloss
    assert training.PixelWiseFocalLoss is PixelWiseFocalLoss
    assert pixelwise_focalloss._label_check is pixelwise_nllloss._label_check          # imported, not copied
    sig = inspect.signature(PixelWiseFocalLoss.__init__).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("weight", None), ("gamma", 2.0), ("ignore_index", -100), ("normalize", "pixels")]
    assert list(inspect.signature(PixelWiseFocalLoss.forward).parameters) == ["self", "predict", "target", "pixelweights"]
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="gamma must be finite and >= 0"):
            PixelWiseFocalLoss(gamma=bad)
    with pytest.raises(ValueError, match="normalize must be one of"):
        PixelWiseFocalLoss(normalize="mean")
    crit = PixelWiseFocalLoss(weight=torch.ones(3), gamma=0, normalize="weights")
    assert (crit.gamma, crit.normalize, crit.ignore_index) == (0.0, "weights", -100) and hasattr(crit, "flush")
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
        PixelWiseFocalLoss()(torch.zeros(2, 17, 4, 4), t, w)
    with pytest.raises(AssertionError, match="gradient w.r.t. targets"):
        crit(p, t, w.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(p, t, w)                                                                  # a missing device is an error, not eager torch
