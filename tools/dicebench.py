#!/usr/bin/env python3
"""The region-loss library (libubresnet_dice.so) against its byte bounds, against the focal pair of libubresnet_loss.so and the
NLL pair of libubresnet_hip.so, and against what a user could write with torch, alone on the device and inside a train step,
alternated in one process (the method of tools/lossbench.py).

    python tools/dicebench.py [--launches N] [--reps R] [--steps S] [--no-train] [--no-accuracy] [--out FILE]

Kernel legs, fp32, at 16 x 3 x 512 x 512 and 16 x 3 x 512 x 832 (a log-softmax of seeded logits, a synthetic target that is
mostly background, unit weights): ubk_dice_fwd (alpha = beta = 0.5, eps = 1) and ubk_dice_bwd, ubl_focal_fwd and ubl_focal_bwd at
gamma = 2, ubr_pixelwise_nll_fwd and ubr_pixelwise_nll_bwd, each alone (a pair is the sum of its two), and the torch composite
under autograd, forward and backward:

    p = logp.exp();  oh = one_hot(t);  TP = (w p oh).sum((0, 2, 3));  FP = (w p (1 - oh)).sum(..);  FN = (w (1 - p) oh).sum(..)
    loss = (1 - (TP + 1) / (TP + 0.5 FP + 0.5 FN + 1)).mean()

and the forward at 16 x 8 x 512 x 512, the instantiation with the runtime class count.  A repetition is `--launches` back-to-back
calls of one leg between two device events; the legs alternate; median and spread (max - min) of the per-call time over `--reps`
repetitions.  Byte bounds at 6 TB/s: the Dice forward reads 4 C + 12 bytes per pixel (every channel, target 8, weight 4), its
backward reads the same and writes 4 C: 8 C + 12.

Accuracy: at the first shape, (alpha, beta, eps) in {(.5, .5, 1), (.3, .7, 1e-6), (0, 1, 1)}, the worst ratio of the error of the
sums, the coefficients, the loss and a gradient element to the bound of tests/dice_ref.py.

Train-step legs: bf16 16 x 1 x 512 x 512, inplanes 16, FlatAdam(lr 1e-5, weight_decay 1e-4, max_grad_norm=1.0,
skip_nonfinite=True) with PixelWiseNLLLoss (the step as it was) and with WeightedSumLoss of NLL + 0.5 Dice, two models from the
same seed; a repetition is `--steps` steps between two synchronisations, ms per step.  The difference holds the Dice pair, the NLL
pair staying, and what autograd adds around them: the scaling of the Dice term, the sum of the two losses, and the add of the two
gradient images (12 C bytes per pixel)."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

B, H, W = 16, 512, 512
SHAPES = [(16, 3, 512, 512), (16, 3, 512, 832), (16, 8, 512, 512)]
HBM = 6.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from ubresnet_amd import _dice as K
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _loss as F
    from ubresnet_amd import ops, synthetic
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training import PixelWiseDiceLoss, WeightedSumLoss
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    dev = torch.device("cuda:0")
    lines = ["# us per call, %d back-to-back calls between two device events; median (spread = max - min) over %d alternating repetitions; "
             "x bound = time / (bytes / 6 TB/s)" % (a.launches, a.reps)]
    pair = {}
    for (N, C, Hh, Ww) in SHAPES:
        first = (N, C, Hh, Ww) in SHAPES[:2]
        g = torch.Generator().manual_seed(N * Ww + C)
        logp = torch.log_softmax(4.0 * torch.randn(N, C, Hh, Ww, generator=g), dim=1).to(dev)
        lab = torch.from_numpy(np.concatenate([synthetic.make_batch(N, Hh, 512, 1000 + k)[1] for k in range((Ww + 511) // 512)], axis=2)[:, :, :Ww].copy()).to(dev)
        wgt = torch.ones(N, Hh, Ww, device=dev)
        pixels = N * Hh * Ww
        background = float((lab == 0).float().mean())
        ws = torch.empty(K.WORKSPACE_BYTES // 8, dtype=torch.float64, device=dev)
        ctl = torch.zeros(K.CTL_WORDS, dtype=torch.float64, device=dev)
        fws = torch.empty(F.WORKSPACE_BYTES // 8, dtype=torch.float64, device=dev)
        fctl = torch.zeros(F.CTL_WORDS, dtype=torch.float64, device=dev)
        loss = torch.zeros((), device=dev)
        one = torch.ones((), device=dev)
        gp = torch.empty_like(logp)
        acc = torch.zeros(L.STAT_SLOTS + 1, dtype=torch.float64, device=dev)
        s = L.stream_ptr()

        def dfwd(alpha=0.5, beta=0.5, eps=1.0):
            return lambda: K.dice_fwd(logp.data_ptr(), lab.data_ptr(), wgt.data_ptr(), None, N, C, Hh, Ww, -100, alpha, beta, eps, True,
                                      ws.data_ptr(), ctl.data_ptr(), loss.data_ptr(), s)

        def dbwd():
            K.dice_bwd(one.data_ptr(), ctl.data_ptr(), logp.data_ptr(), lab.data_ptr(), wgt.data_ptr(), N, C, Hh, Ww, -100, gp.data_ptr(), s)

        def composite():
            x = logp.clone().requires_grad_(True)
            oh = torch.nn.functional.one_hot(lab, C).permute(0, 3, 1, 2).float()

            def f():
                x.grad = None
                p = x.exp()
                wp = wgt[:, None] * p
                tp, fp, fn = (wp * oh).sum((0, 2, 3)), (wp * (1 - oh)).sum((0, 2, 3)), (wgt[:, None] * (1 - p) * oh).sum((0, 2, 3))
                (1 - (tp + 1) / (tp + 0.5 * fp + 0.5 * fn + 1)).mean().backward()
            return f

        legs = {"ubk_dice_fwd": (dfwd(), (4.0 * C + 12.0) * pixels)}
        if first:
            legs["ubk_dice_bwd"] = (dbwd, (8.0 * C + 12.0) * pixels)
            legs["ubl_focal_fwd gamma 2"] = (lambda: F.focal_fwd(logp.data_ptr(), lab.data_ptr(), wgt.data_ptr(), None, N, C, Hh, Ww, -100, 2.0,
                                                                 F.MEAN_PIXELS, fws.data_ptr(), fctl.data_ptr(), loss.data_ptr(), s), 16.0 * pixels)
            legs["ubl_focal_bwd gamma 2"] = (lambda: F.focal_bwd(one.data_ptr(), fctl.data_ptr(), logp.data_ptr(), lab.data_ptr(), wgt.data_ptr(), None,
                                                                 N, C, Hh, Ww, -100, 2.0, gp.data_ptr(), s), (16.0 + 4.0 * C) * pixels)
            legs["ubr_pixelwise_nll_fwd"] = (lambda: ops.pixelwise_nll_fwd(logp, lab, wgt, None, -100, acc, bad=acc[L.STAT_SLOTS:]), 16.0 * pixels)
            legs["ubr_pixelwise_nll_bwd"] = (lambda: ops.pixelwise_nll_bwd(one, lab, wgt, None, -100, (N, C, Hh, Ww), gp), (12.0 + 4.0 * C) * pixels)
            legs["torch composite fwd+bwd"] = (composite(), None)
        else:
            legs["ubk_dice_bwd"] = (dbwd, (8.0 * C + 12.0) * pixels)
        times = {k: [] for k in legs}
        for fn, _ in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, (fn, _) in legs.items():
                n = a.launches if not name.startswith("torch") else max(1, a.launches // 10)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / n)
        tag = "%dx%dx%dx%d" % (N, C, Hh, Ww)
        lines.append("# %s: %d pixels, %.1f %% background; grid %d workgroups of %d lanes, %d pixels per trip; forward instantiation: %s"
                     % (tag, pixels, 100 * background, K.grid(pixels), K.BLOCK, K.TRIP_PIXELS,
                        "C = %d in registers" % C if C <= K.REG_CLASSES else "runtime C"))
        md = {k: statistics.median(t) for k, t in times.items()}
        sp = {k: max(t) - min(t) for k, t in times.items()}
        for name, (_, nbytes) in legs.items():
            bound = "" if nbytes is None else "  %5.2f x bound (%.1f us)" % (md[name] / (nbytes / HBM * 1e6), nbytes / HBM * 1e6)
            lines.append("%-14s %-28s %9.2f us (spread %.2f)%s   runs: %s" % (tag, name, md[name], sp[name], bound, " ".join("%.2f" % v for v in times[name])))
        dice = md["ubk_dice_fwd"] + md["ubk_dice_bwd"]
        pair[tag] = dice
        if first:
            nll = md["ubr_pixelwise_nll_fwd"] + md["ubr_pixelwise_nll_bwd"]
            focal = md["ubl_focal_fwd gamma 2"] + md["ubl_focal_bwd gamma 2"]
            pair[(tag, "nll")] = nll
            lines.append("%-14s Dice pair %9.2f us: x%.2f the focal pair (%.2f us), x%.2f the NLL pair (%.2f us); torch composite %.2f us: x%.1f the Dice pair"
                         % (tag, dice, dice / focal, focal, dice / nll, nll, md["torch composite fwd+bwd"], md["torch composite fwd+bwd"] / dice))
        if not a.no_accuracy and (N, C, Hh, Ww) == SHAPES[0]:
            import dice_ref as R
            hp, hl, hw_ = logp.cpu().numpy(), lab.cpu().numpy(), wgt.cpu().numpy()
            sums = R.sums(hp, hl, hw_, -100)
            lines.append("# accuracy at %s against tests/dice_ref.py (expf and expm1f taken as 2 ulp each): worst error / bound" % tag)
            for alpha, beta, eps in ((0.5, 0.5, 1.0), (0.3, 0.7, 1e-6), (0.0, 1.0, 1.0)):
                dfwd(alpha, beta, eps)()
                dbwd()
                torch.cuda.synchronize()
                c = K.read_ctl(ctl.cpu().numpy().tobytes())
                f = R.complete(sums, None, alpha, beta, eps, True)
                want, lim, ok = R.backward(1.0, f)
                hot = np.broadcast_to(ok[:, None], want.shape)
                err = np.abs(gp.cpu().numpy().astype(np.float64) - want)[hot]

                def worst(got, ref, bound):
                    e = np.abs(np.asarray(got[:C]) - ref)
                    return float(np.where(e == 0, 0.0, e / bound).max())
                lines.append("accuracy alpha %-4g beta %-4g eps %-6g gradient %.3f   sums %.3f   T %.3f   K1 %.3f   K0 %.3f   loss %.3f   counts %s" % (
                    alpha, beta, eps, float((err / lim[hot]).max()),
                    max(worst(c["tp"], f["tp"], f["d_tp"]), worst(c["fp"], f["fp"], f["d_fp"]), worst(c["fn"], f["fn"], f["d_fn"])),
                    worst(c["T"], f["T"], f["lim_T"]), worst(c["k1"], f["K1"], f["lim_K1"]), worst(c["k0"], f["K0"], f["lim_K0"]),
                    abs(c["loss"] - f["loss"]) / f["lim_loss"], "exact" if (c["valid"], c["pixels"][:C]) == (f["valid"], f["pixels"]) else "WRONG"))
        del logp, lab, wgt, gp
    if not a.no_train:
        x, lab, wgt = synthetic.make_batch(B, H, W, seed0=1000)
        x, lab, wgt = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(wgt).to(dev)
        runs = {}
        for name, crit in (("PixelWiseNLLLoss", PixelWiseNLLLoss()),
                           ("NLL + 0.5 PixelWiseDiceLoss", WeightedSumLoss([(1.0, PixelWiseNLLLoss()), (0.5, PixelWiseDiceLoss())]))):
            torch.manual_seed(1234)
            model = UResNet(num_classes=3, input_channels=1, inplanes=16).to(dev)
            model.compute_dtype = torch.bfloat16
            model.train()
            runs[name] = (model, FlatAdam(model, lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True), crit)

        def step(name):
            model, opt, crit = runs[name]
            loss = crit.forward(model.forward(x), lab, wgt)
            opt.zero_grad()
            loss.backward()
            opt.step()
        for name in runs:
            for _ in range(5):
                step(name)
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.reps):
            for name in runs:
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(name)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
        lines.append("# train step, bf16 %d x 1 x %d x %d, inplanes 16, guarded FlatAdam; ms per step, %d steps between two synchronisations; "
                     "median (spread) over %d alternating repetitions; the NLL leg is the step as it was" % (B, H, W, a.steps, a.reps))
        for name in runs:
            t = times[name]
            lines.append("train %-28s %8.3f ms (spread %.3f)   runs: %s" % (name, statistics.median(t), max(t) - min(t), " ".join("%.3f" % v for v in t)))
        n, f = times["PixelWiseNLLLoss"], times["NLL + 0.5 PixelWiseDiceLoss"]
        gap = (statistics.median(f) - statistics.median(n)) * 1e3
        s0, s1 = (max(n) - min(n)) * 1e3, (max(f) - min(f)) * 1e3
        tag = "%dx%dx%dx%d" % SHAPES[0]
        lines.append("# (NLL + Dice) - NLL: difference of the medians %+.1f us per step against spreads %.1f / %.1f us: %s the two spreads; the Dice "
                     "pair alone is %.1f us at %s fp32 (the step's criterion runs at that shape); the remainder, %+.1f us, is what autograd adds: the "
                     "scaled term, the sum of the losses and the add of the two gradient images" % (
                         gap, s0, s1, "outside" if abs(gap) > s0 + s1 else "inside", pair[tag], tag, gap - pair[tag]))
        for name in runs:
            runs[name][2].flush()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
