#!/usr/bin/env python3
"""The focal-loss library (libubresnet_loss.so) against the NLL pair of libubresnet_hip.so and against what a user could write
with torch, alone on the device and inside a train step, alternated in one process.

    python tools/lossbench.py [--launches N] [--reps R] [--steps S] [--no-train] [--no-accuracy] [--out FILE]

Kernel legs, fp32, at 16 x 3 x 512 x 512 and 16 x 3 x 512 x 832 (a log-softmax of seeded logits, a synthetic target that is
mostly background, unit weights): ubl_focal_fwd and ubl_focal_bwd at gamma = 0, 2 and 2.5 ("pixels" mode), ubr_pixelwise_nll_fwd
and ubr_pixelwise_nll_bwd, each alone (the pair is their sum), and the torch composite under autograd, forward and backward:

    lpt = logp.gather(1, t[:, None])[:, 0];  loss = (-(1 - lpt.exp()) ** gamma * lpt * w).sum() / w.numel()

A repetition is `--launches` back-to-back calls of one leg between two device events; the legs alternate; median and spread
(max - min) of the per-call time over `--reps` repetitions.  Byte bounds at 6 TB/s: the forward reads 16 B per pixel (target 8,
weight 4, the gathered log-probability 4) -- 44 B if every gathered value cost a 32-byte sector of its own, which neighbouring
pixels of one class share; the backward reads the same and writes 4 C bytes: 16 + 4 C.

Accuracy: at the first shape, gamma = 0.5, 1, 2, 2.5, 5 in "weights" mode, the worst ratio of the error of a gradient element and
of the loss sum to the bound of tests/loss_ref.py.

Train-step legs: bf16 16 x 1 x 512 x 512, inplanes 16, FlatAdam(lr 1e-5, weight_decay 1e-4, max_grad_norm=1.0,
skip_nonfinite=True) with PixelWiseNLLLoss and with PixelWiseFocalLoss(gamma=2), two models from the same seed; a repetition is
`--steps` steps between two synchronisations, ms per step.  The NLL leg is the step as it was before the library existed."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

B, H, W = 16, 512, 512
SHAPES = [(16, 3, 512, 512), (16, 3, 512, 832)]
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
    from ubresnet_amd import _lib as L
    from ubresnet_amd import _loss as K
    from ubresnet_amd import ops, synthetic
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training import PixelWiseFocalLoss
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    dev = torch.device("cuda:0")
    lines = ["# us per call, %d back-to-back calls between two device events; median (spread = max - min) over %d alternating repetitions; "
             "x bound = time / (bytes / 6 TB/s)" % (a.launches, a.reps)]
    pair = {}
    for (N, C, Hh, Ww) in SHAPES:
        g = torch.Generator().manual_seed(N * Ww)
        logp = torch.log_softmax(4.0 * torch.randn(N, C, Hh, Ww, generator=g), dim=1).to(dev)
        lab = torch.from_numpy(np.concatenate([synthetic.make_batch(N, Hh, 512, 1000 + k)[1] for k in range((Ww + 511) // 512)], axis=2)[:, :, :Ww].copy()).to(dev)
        wgt = torch.ones(N, Hh, Ww, device=dev)
        pixels = N * Hh * Ww
        background = float((lab == 0).float().mean())
        ws = torch.empty(K.WORKSPACE_BYTES // 8, dtype=torch.float64, device=dev)
        ctl = torch.zeros(K.CTL_WORDS, dtype=torch.float64, device=dev)
        loss = torch.zeros((), device=dev)
        one = torch.ones((), device=dev)
        gp = torch.empty_like(logp)
        acc = torch.zeros(L.STAT_SLOTS + 1, dtype=torch.float64, device=dev)
        s = L.stream_ptr()

        def ffwd(gamma):
            return lambda: K.focal_fwd(logp.data_ptr(), lab.data_ptr(), wgt.data_ptr(), None, N, C, Hh, Ww, -100, gamma, K.MEAN_PIXELS,
                                       ws.data_ptr(), ctl.data_ptr(), loss.data_ptr(), s)

        def fbwd(gamma):
            return lambda: K.focal_bwd(one.data_ptr(), ctl.data_ptr(), logp.data_ptr(), lab.data_ptr(), wgt.data_ptr(), None, N, C, Hh, Ww, -100,
                                       gamma, gp.data_ptr(), s)

        def composite(gamma):
            x = logp.clone().requires_grad_(True)

            def f():
                x.grad = None
                lpt = x.gather(1, lab[:, None])[:, 0]
                ((-(1.0 - lpt.exp()) ** gamma * lpt * wgt).sum() / wgt.numel()).backward()
            return f

        fb, bb = 16.0 * pixels, (16.0 + 4.0 * C) * pixels
        legs = {}
        for gamma in (0.0, 2.0, 2.5):
            legs["ubl_focal_fwd gamma %g" % gamma] = (ffwd(gamma), fb)
            legs["ubl_focal_bwd gamma %g" % gamma] = (fbwd(gamma), bb)
        legs["ubr_pixelwise_nll_fwd"] = (lambda: ops.pixelwise_nll_fwd(logp, lab, wgt, None, -100, acc, bad=acc[L.STAT_SLOTS:]), fb)
        legs["ubr_pixelwise_nll_bwd"] = (lambda: ops.pixelwise_nll_bwd(one, lab, wgt, None, -100, (N, C, Hh, Ww), gp), (12.0 + 4.0 * C) * pixels)
        legs["torch composite fwd+bwd gamma 2"] = (composite(2.0), None)
        legs["torch composite fwd+bwd gamma 2.5"] = (composite(2.5), None)
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
        lines.append("# %s: %d pixels, %.1f %% background; focal grid %d workgroups of %d lanes, %d pixels per trip; the NLL backward reads no "
                     "log-probability: its bound is 12 + 4 C bytes per pixel" % (tag, pixels, 100 * background, K.grid(pixels), K.BLOCK, K.TRIP_PIXELS))
        md = {k: statistics.median(t) for k, t in times.items()}
        sp = {k: max(t) - min(t) for k, t in times.items()}
        for name, (_, nbytes) in legs.items():
            bound = "" if nbytes is None else "  %5.2f x bound (%.1f us)" % (md[name] / (nbytes / HBM * 1e6), nbytes / HBM * 1e6)
            lines.append("%-14s %-36s %9.2f us (spread %.2f)%s   runs: %s" % (tag, name, md[name], sp[name], bound, " ".join("%.2f" % v for v in times[name])))
        nll = md["ubr_pixelwise_nll_fwd"] + md["ubr_pixelwise_nll_bwd"]
        for gamma in (0.0, 2.0, 2.5):
            p = md["ubl_focal_fwd gamma %g" % gamma] + md["ubl_focal_bwd gamma %g" % gamma]
            pair[(tag, gamma)] = p
            lines.append("%-14s pair gamma %-4g %9.2f us against the NLL pair %.2f us: x%.2f" % (tag, gamma, p, nll, p / nll))
        pair[(tag, "nll")] = nll
        for gamma in (2.0, 2.5):
            p = pair[(tag, gamma)]
            lines.append("%-14s torch composite gamma %-4g %9.2f us: x%.1f the focal pair" % (tag, gamma, md["torch composite fwd+bwd gamma %g" % gamma],
                                                                                         md["torch composite fwd+bwd gamma %g" % gamma] / p))
        if not a.no_accuracy and (N, C, Hh, Ww) == SHAPES[0]:
            import loss_ref as R
            hp, hl, hw_ = logp.cpu().numpy(), lab.cpu().numpy(), wgt.cpu().numpy()
            lines.append("# accuracy at %s, \"weights\" mode, against tests/loss_ref.py (expf, expm1f, exp2f, log2f taken as 2 ulp each): worst error / "
                         "bound; literal: the same errors against the bound with the coefficient of |ln q| set to 1" % tag)
            for gamma in (0.5, 1.0, 2.0, 2.5, 5.0):
                K.focal_fwd(logp.data_ptr(), lab.data_ptr(), wgt.data_ptr(), None, N, C, Hh, Ww, -100, gamma, K.MEAN_WEIGHTS, ws.data_ptr(),
                            ctl.data_ptr(), loss.data_ptr(), s)
                fbwd(gamma)()
                torch.cuda.synchronize()
                c = K.read_ctl(ctl.cpu().numpy().tobytes())
                f = R.forward(hp, hl, hw_, None, -100, gamma, "weights")
                want, lim, hot = R.backward(1.0, f, gamma, C)
                err = np.abs(gp.cpu().numpy().astype(np.float64) - want)[hot]
                keep = R.C_LN
                R.C_LN = 1.0
                try:
                    f1 = R.forward(hp, hl, hw_, None, -100, gamma, "weights")
                    lim1 = R.backward(1.0, f1, gamma, C)[1]
                finally:
                    R.C_LN = keep
                lines.append("accuracy gamma %-4g gradient %.3f (literal %.3f)   loss sum %.3f (literal %.3f)   counts %s" % (
                    gamma, float((err / lim[hot]).max()), float((err / lim1[hot]).max()), abs(c["loss_sum"] - f["loss_sum"]) / f["lim_sum"],
                    abs(c["loss_sum"] - f1["loss_sum"]) / f1["lim_sum"], "exact" if (c["valid"], c["class_pixels"][:C]) == (f["valid"], f["class_pixels"]) else "WRONG"))
        del logp, lab, wgt, gp
    if not a.no_train:
        x, lab, wgt = synthetic.make_batch(B, H, W, seed0=1000)
        x, lab, wgt = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(wgt).to(dev)
        runs = {}
        for name, crit in (("PixelWiseNLLLoss", PixelWiseNLLLoss()), ("PixelWiseFocalLoss gamma 2", PixelWiseFocalLoss(gamma=2.0))):
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
        n, f = times["PixelWiseNLLLoss"], times["PixelWiseFocalLoss gamma 2"]
        gap = (statistics.median(f) - statistics.median(n)) * 1e3
        s0, s1 = (max(n) - min(n)) * 1e3, (max(f) - min(f)) * 1e3
        tag = "%dx%dx%dx%d" % SHAPES[0]
        kernels = pair[(tag, 2.0)] - pair[(tag, "nll")]
        lines.append("# focal - NLL: difference of the medians %+.1f us per step against spreads %.1f / %.1f us: %s the two spreads; the kernel pairs "
                     "differ by %+.1f us at %s fp32 (the step's criterion runs at that shape)%s" % (
                         gap, s0, s1, "outside" if abs(gap) > s0 + s1 else "inside", kernels, tag,
                         "" if abs(gap) <= s0 + s1 else ("; accounted for by the kernels" if abs(gap - kernels) <= s0 + s1 else "; NOT attributed")))
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
