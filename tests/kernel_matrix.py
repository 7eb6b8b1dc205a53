"""The kernel matrix: one row per compiled kernel of libubresnet_hip.so, each holding the smallest valid call that makes the host-side
dispatch pick that instantiation.  tests/test_cpu_kernel_matrix.py checks that the rows' symbols equal the symbol table of the built
library (tools/kernel_symbols.py); tests/test_gpu_kernel_matrix.py runs every row on the GPU against the float64 references of
tests/kref.py with the library's launch log (ubr_launch_log) switched on.  Importable without a GPU.

A row is a dict: id, symbols (every kernel the call launches), entry (the C entry point), op, dtype, args, env.  op "conv" / "wgrad":
a call record for replay_conv / replay_wgrad of test_gpu_kernels_exact.py; "stream": a case for the REPLAY table of
test_gpu_stream_exact.py, built by that module's case builders (args = (builder, keyword arguments)); "check": an existing exact
check of another test module called as a function (args = (module, function, arguments)).
Rows with `env` set a switch the library reads once per process, so they run in a fresh child: python -m tests.kernel_matrix ID.

How the shapes are chosen (from plan_tile / plan_pc / try_thin / launch_cfg and wgrad_plan / wdispatch, not by trial):

conv_igemm_kernel<T, FW, NT, TWF, PIPE>: tile_hint = the tile's index + 1; TH x TW = (4 FW / TWF) x (16 TWF) pixels, TN = 16 NT
  channels.  Two images of (2 TH - 1) x (2 TW - 3) pixels: 2 x 2 tiles, the last one ragged both ways (which is also what makes
  try_thin decline on the tiles it shares).  3x3 taps.  PIPE = false: Cin = one 16-byte unit (UPB = 1, one cin block; nine units
  in K-steps of four leave a partial last step); the output is Cout = TN - 4 channels at offset 4 of a buffer TN + 8 wide, so the
  last channel group is cut and no 16-byte store is possible.  PIPE = true (NT = 4): Cin = 8 units (UPB = 4, nblk = 2), xf, bias and
  statistics on, a dense output of TN channels.
conv_thin_kernel<T, FW, NT, TWF, UPB, XF, LSM, ROW7, EXT>: same hints; extents are whole tiles (2 TH x 2 TW, try_thin declines
  otherwise), Cin = UPB units (one cin block).  Cout = TN at channel offset 8 of a buffer TN + 16 wide (16-bit stores need whole
  aligned octets).  XF: the BatchNorm-on-load operand.  EXT 1: bnb (BatchNorm-backward sums); EXT 2: addend + addend_mask.  LSM: the
  log-softmax epilogue with 3 classes.  ROW7: the 49 taps of a 7x7 window over 16 channels on the 16 x 32 tile, 16-bit types.
  The 16 x 32 tile has no UPB = 4 form: 16 * 32 * 4 halo items exceed try_thin's 256 * 6 register slots for any tap set.
conv_pc_kernel<T, FW, TWF, STEPS>: tile_hint 101..104; Cin = 4 units, Cout = 60 of 64 in a 72-wide buffer; (2 TH - 1) x (2 TW - 3)
  pixels (OW = 61 >= 32 for TWF = 2); 9 taps (3x3), 4 taps (phase (0,0) of a k4 s2 transposed conv) and 1 tap for STEPS 9 / 4 / 0.
wgrad_kernel<T, MA, NB, TPG, NSPLIT, BIGX, PC>: two images, a 10 x 40 gradient grid (two 32-pixel tile columns, the second ragged;
  rows beyond the grid in the last tile row), channels the smallest multiples of 16 that give MA and NB (16 / 32, 64 x 64 for
  the N-split forms), taps 1x1 / 2x2 / 3x3 / 5x5 for TPG 1 / 4 / 9 / 25.  BIGX needs a halo beyond the narrow slots: 3x3 with
  dilation 2 (NB = 1) or 3 (NB = 2).  <2, 2, 9>: 64 x 64 channels with dilation 4, whose halo the N-split form cannot stage even
  one row at a time.  <2, 4, 9, true> without the producer / consumer form (16-bit) needs UBR_WGRAD_PC=0, <4, 4, 9, true>
  UBR_WGRAD_MA9=4.  Every row runs as one launch (ubr_wgrad + ubr_wgrad_reduce: wgrad_reduce_flat_kernel for the <= 8 slabs of
  these grids) and through ubr_wgrad_reduce_batched; one row per dtype has a 20-row grid, 12 slabs, and lands on wgrad_reduce_kernel.
  wgrad_variant() restates wgrad_plan / wdispatch so that the CPU test can check every row's claim without a GPU.
Streaming kernels (csrc/ubr_elem.hip): one row per combination of the template switches -- dtype; bypass or identity; one or two
  gradient operands (the second a channel slice of a buffer twice as wide); ReLU or not; mask bytes or the block output as gate;
  reduce or apply; with or without `red`; stride 1 or 2, xf, arg-max and xcopy for the max-pool.  C = 48 channels (6 or 12
  16-byte units: not a power of two, so the sums take the atomic flush) and 2 x 13 x 21 = 546 pixels, which leave the last trip of
  every grid partial; the max-pool rows that need even extents (xcopy, the stride-2 backward forms) use 14 x 22.  The stride-2
  max-pool backward replay runs the saved-arg-max and the re-scanning kernel, so those rows declare both.
Head, parameter-side and legacy entry points: the exact checks the suite already has, at their smallest case: the stem (ubr_stem_forward
  / ubr_stem_wgrad, one row per dtype and Cout 16 / 32), ubr_pack_weights and ubr_pack_weights_batched, the BatchNorm fold and
  finalizes, the flat optimizer steps, tile crop / stitch, the loss kernels, stem_expand, logsoftmax_bwd and ubr_aspp_front."""
import os
import sys

DTYPES = ("float", "bf16_t", "f16_t")
CPU = {"float": 4, "bf16_t": 8, "f16_t": 8}
TORCH_DT = {"float": "float32", "bf16_t": "bfloat16", "f16_t": "float16"}
OPS = ("conv", "wgrad", "stream", "check")
# the switches of csrc/ubr_wgrad.hip (read with getenv, once per process) that rows set
ENV_SWITCHES = ("UBR_WGRAD_PC", "UBR_WGRAD_MA9")
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TILES = ((8, 1, 2), (4, 1, 2), (4, 2, 2), (4, 4, 2), (2, 4, 1), (1, 4, 1), (2, 2, 1), (2, 1, 1), (1, 2, 1), (1, 1, 1))   # kCfgs
PC_TILES = ((4, 2), (2, 2), (4, 1), (2, 1))                                                                              # kPc


def family(sym):
    return sym.split("<")[0]


def _b(v):
    return "true" if v else "false"


# ------------------------------------------------------------------------------------------------------------------
# ubr_conv
# ------------------------------------------------------------------------------------------------------------------
def _conv_rows():
    rows = []
    for T in DTYPES:
        cpu = CPU[T]
        for i, (FW, NT, TWF) in enumerate(TILES):
            TH, TW, TN = 4 * FW // TWF, 16 * TWF, 16 * NT
            rag = dict(N=2, OH=2 * TH - 1, OW=2 * TW - 3, k=3, tile_hint=i + 1)
            rows.append(dict(symbols=("conv_igemm_kernel<%s, %d, %d, %d, false>" % (T, FW, NT, TWF),), op="conv", dtype=T,
                             args=dict(rag, Cin=cpu, Cout=TN - 4, ywidth=TN + 8, yoff=4)))
            if NT == 4:
                rows.append(dict(symbols=("conv_igemm_kernel<%s, %d, %d, %d, true>" % (T, FW, NT, TWF),), op="conv", dtype=T,
                                 args=dict(rag, Cin=8 * cpu, Cout=TN, xf=True, bias=True, stats=True)))
            if NT <= 2 and TWF == 2:
                whole = dict(N=2, OH=2 * TH, OW=2 * TW, k=3, tile_hint=i + 1, Cout=TN, ywidth=TN + 16, yoff=8)
                for UPB in (2, 4):
                    if FW == 8 and UPB == 4:
                        continue
                    name = "conv_thin_kernel<%s, %d, %d, %d, %d, %%s, %%s, %%s, %%d>" % (T, FW, NT, TWF, UPB)
                    base = dict(whole, Cin=UPB * cpu)
                    for xf in (False, True):
                        rows.append(dict(symbols=(name % (_b(xf), "false", "false", 0),), op="conv", dtype=T, args=dict(base, xf=xf, bias=True, stats=True)))
                    rows.append(dict(symbols=(name % ("false", "false", "false", 1),), op="conv", dtype=T, args=dict(base, bnb=True)))
                    rows.append(dict(symbols=(name % ("false", "false", "false", 2),), op="conv", dtype=T, args=dict(base, addend=True, mask=True)))
                    if (FW, NT, UPB) == (4, 1, 2):
                        for xf in (False, True):
                            rows.append(dict(symbols=(name % (_b(xf), "true", "false", 0),), op="conv", dtype=T,
                                             args=dict(N=2, OH=2 * TH, OW=2 * TW, k=3, tile_hint=i + 1, Cin=2 * cpu, Cout=3, xf=xf, bias=True, logsoftmax=True)))
                if (FW, NT) == (8, 1) and T != "float":
                    name = "conv_thin_kernel<%s, 8, 1, 2, 2, %%s, %%s, true, %%d>" % T
                    seven = dict(whole, k=7, Cin=16)
                    for xf in (False, True):
                        rows.append(dict(symbols=(name % (_b(xf), "false", 0),), op="conv", dtype=T, args=dict(seven, xf=xf, bias=True, stats=True)))
                        rows.append(dict(symbols=(name % (_b(xf), "true", 0),), op="conv", dtype=T,
                                         args=dict(N=2, OH=2 * TH, OW=2 * TW, k=7, tile_hint=1, Cin=16, Cout=3, xf=xf, bias=True, logsoftmax=True)))
                    rows.append(dict(symbols=(name % ("false", "false", 1),), op="conv", dtype=T, args=dict(seven, bnb=True)))
                    rows.append(dict(symbols=(name % ("false", "false", 2),), op="conv", dtype=T, args=dict(seven, addend=True, mask=True)))
        for i, (FW, TWF) in enumerate(PC_TILES):
            TH, TW = 4 * FW // TWF, 16 * TWF
            for steps, k in ((9, 3), (4, "phase"), (0, 1)):
                rows.append(dict(symbols=("conv_pc_kernel<%s, %d, %d, %d>" % (T, FW, TWF, steps),), op="conv", dtype=T,
                                 args=dict(N=2, OH=2 * TH - 1, OW=2 * TW - 3, k=k, tile_hint=101 + i, Cin=4 * cpu, Cout=60, ywidth=72, yoff=4,
                                           xf=steps == 9, bias=True, stats=steps != 4, addend=steps == 4, act=3 if steps == 4 else 0)))
    for r in rows:
        r["entry"], r["env"] = "ubr_conv", None
    return rows


# ------------------------------------------------------------------------------------------------------------------
# ubr_wgrad: the planner restated (wgrad_plan / wdispatch of csrc/ubr_wgrad.hip)
# ------------------------------------------------------------------------------------------------------------------
def _wtaps(k, dil):
    pad = dil * (k // 2)
    return [(ky * dil - pad, kx * dil - pad, ky * k + kx) for ky in range(k) for kx in range(k)]


def _xslots(nsplit, tpg, nb, cpu, bigx, ma):
    tall = nsplit and tpg == 9 and ma == 2
    n = 12 if bigx else 11 if tall else 7 if nsplit else 5 if tpg == 25 else (3 if nb == 1 else 6)
    return n * (8 // cpu)


def wgrad_variant(T, N, GH, GW, Cin, Cout, k, dil=1, S=1, exclusive=False, env=None):
    """-> (kernel symbol, nsplit) wgrad_plan / wdispatch choose, or (None, reason)"""
    env = env or {}
    cpu = CPU[T]
    taps = _wtaps(k, dil)
    ntaps = len(taps)
    dys, dxs = [t[0] for t in taps], [t[1] for t in taps]
    ey, ex = max(dys) - min(dys), max(dxs) - min(dxs)
    TPG = 1 if ntaps <= 1 else 4 if ntaps <= 4 else 9 if ntaps <= 9 else 25
    MA, NB = (2 if Cout % 32 == 0 else 1), (2 if Cin % 32 == 0 else 1)
    if TPG == 25:
        MA = NB = 1
    if TPG == 9 and MA == 2 and NB == 2:
        NB = 1
    nsm, TH = 0, (8 if S == 1 else 4)
    if TPG <= 9 and Cout % 64 == 0 and Cin % 64 == 0:
        MA, NB, nsm = (int(env.get("UBR_WGRAD_MA9", 2)) if TPG == 9 else 4), 4, 1
        TH = (8 if (TPG == 9 and MA == 2) else 4) if S == 1 else 2
    th0, bigx = TH, 0
    while True:
        xs = _xslots(nsm != 0, TPG, NB, cpu, bigx != 0, MA)
        ux = NB * 16 // cpu
        HH, HW = (TH - 1) * S + 1 + ey, 31 * S + 1 + ex
        if HH * HW * ux <= 256 * xs:
            break
        if not exclusive and not bigx and not nsm and MA == 1 and TPG == 9:
            bigx = 1
        elif TH > 1:
            TH //= 2
        elif nsm:
            nsm, MA, NB, TH = 0, 2, 2, (8 if S == 1 else 4)
        elif NB > 1:
            NB, bigx, TH = 1, 0, min(th0, 4)
        elif MA > 1 and TPG == 9:
            MA, TH = 1, min(th0, 4)
        else:
            return None, "halo does not fit"
    ntiles = -(-GW // 32) * -(-GH // TH) * N
    gy, gz = (Cout // (MA * 16)) * (Cin // (NB * 16)), -(-ntaps // TPG)
    target = max(1, (768 if exclusive else 128 if nsm else 256) // (gy * gz))
    target = min(target, max(1, (64 << 20) // (ntaps * Cout * Cin * 4)))
    nsplit = min(ntiles, target)
    pc = False
    if bigx and not nsm and MA == 1 and TPG == 9:
        pass
    elif cpu == 8 and int(env.get("UBR_WGRAD_PC", 1)) and not bigx and nsm and (MA, NB, TPG) == (2, 4, 9):
        pc = True
    elif nsm:
        if bigx or (MA, TPG) not in ((4, 1), (4, 4), (2, 9), (4, 9)):
            return None, "no kernel"
    elif bigx or (TPG == 25 and (MA, NB) != (1, 1)) or MA > 2 or NB > 2:
        return None, "no kernel"
    return "wgrad_kernel<%s, %d, %d, %d, %s, %s, %s>" % (T, MA, NB, TPG, _b(nsm), _b(bigx), _b(pc)), nsplit


def _wgrad_rows():
    rows = []
    K = {1: 1, 4: 2, 9: 3, 25: 5}
    for T in DTYPES:
        cases = []
        for tpg in (1, 4, 9):
            for ma in (1, 2):
                for nb in (1, 2):
                    if (ma, nb, tpg) == (2, 2, 9):
                        cases.append(((2, 2, 9, False, False, False), dict(Cin=64, Cout=64, k=3, dil=4), None))
                    else:
                        cases.append(((ma, nb, tpg, False, False, False), dict(Cin=16 * nb, Cout=16 * ma, k=K[tpg]), None))
        cases.append(((1, 1, 25, False, False, False), dict(Cin=16, Cout=16, k=5), None))
        cases.append(((1, 1, 9, False, True, False), dict(Cin=16, Cout=16, k=3, dil=2), None))
        cases.append(((1, 2, 9, False, True, False), dict(Cin=32, Cout=16, k=3, dil=3), None))
        cases.append(((4, 4, 1, True, False, False), dict(Cin=64, Cout=64, k=1), None))
        cases.append(((4, 4, 4, True, False, False), dict(Cin=64, Cout=64, k=2), None))
        if T == "float":
            cases.append(((2, 4, 9, True, False, False), dict(Cin=64, Cout=64, k=3), None))
        else:
            cases.append(((2, 4, 9, True, False, True), dict(Cin=64, Cout=64, k=3), None))
            cases.append(((2, 4, 9, True, False, False), dict(Cin=64, Cout=64, k=3), {"UBR_WGRAD_PC": "0"}))
        cases.append(((4, 4, 9, True, False, False), dict(Cin=64, Cout=64, k=3), {"UBR_WGRAD_MA9": "4"}))
        for (ma, nb, tpg, ns, bx, pc), a, env in cases:
            sym = "wgrad_kernel<%s, %d, %d, %d, %s, %s, %s>" % (T, ma, nb, tpg, _b(ns), _b(bx), _b(pc))
            args = dict(dict(N=2, GH=10, GW=40, xf=nb == 2 or ns), **a)
            slabs = wgrad_variant(T, 2, 10, 40, a["Cin"], a["Cout"], a["k"], a.get("dil", 1), env=env)[1]     # (one-row tiles: 40 slabs for <2, 2, 9>)
            rows.append(dict(symbols=(sym, "wgrad_reduce_flat_kernel" if slabs <= 8 else "wgrad_reduce_kernel", "wgrad_reduce_batched_kernel"),
                             op="wgrad", dtype=T, args=args, env=env))
        # a taller grid: 12 slabs, summed by wgrad_reduce_kernel in the single-launch form
        rows.append(dict(symbols=("wgrad_kernel<%s, 1, 1, 9, false, false, false>" % T, "wgrad_reduce_kernel", "wgrad_reduce_batched_kernel"),
                         op="wgrad", dtype=T, args=dict(N=2, GH=20, GW=40, Cin=16, Cout=16, k=3), env=None, tag="12slabs"))
    for r in rows:
        r["entry"] = "ubr_wgrad"
    return rows


# ------------------------------------------------------------------------------------------------------------------
# streaming kernels (csrc/ubr_elem.hip) and the head / parameter-side kernels
# ------------------------------------------------------------------------------------------------------------------
SHP, SHP_EVEN, C2 = (2, 13, 21, 48), (2, 14, 22, 48), 96


def _stream_rows():
    rows = []

    def add(T, sym, entry, builder, **kw):
        rows.append(dict(symbols=tuple(sym) if isinstance(sym, (tuple, list)) else (sym,), op="stream", dtype=T, entry=entry,
                         args=(builder, dict(kw, dt=T)), env=None))

    for T in DTYPES:
        for byp in (False, True):
            for msk in (False, True):
                add(T, "tail_fwd_kernel<%s, %s, %s>" % (T, _b(byp), _b(msk)), "ubr_block_tail_fwd",
                    "tail_fwd", shape=SHP, byp=byp, mask=msk)
            for g2 in (False, True):
                for msk in (False, True):
                    for apply in (False, True):
                        add(T, "tail_bwd_kernel<%s, %s, %s, %s, %s>" % (T, _b(apply), _b(byp), _b(g2), _b(msk)),
                            "ubr_block_tail_bwd",
                            "_tail_bwd", kind="apply" if apply else "reduce", shape=SHP, byp=byp, go2_ps=C2 if g2 else None, go2_off=48 if g2 else 0, mask=msk)
                add(T, "tail_bwd_frozen_kernel<%s, %s, %s>" % (T, _b(byp), _b(g2)), "ubr_block_tail_bwd", "_tail_frozen",
                    shape=SHP, byp=byp, go2_ps=C2 if g2 else None, go2_off=48 if g2 else 0)
        for g2 in (False, True):
            for relu in (False, True):
                for apply in (False, True):
                    add(T, "bn_bwd_kernel<%s, %s, %s, %s>" % (T, _b(apply), _b(g2), _b(relu)), "ubr_bn_bwd",
                        "_bn_bwd", kind="apply" if apply else "reduce", shape=SHP, relu=relu, ga2=g2)
                for red in (False, True):
                    add(T, "bn_bwd_frozen_kernel<%s, %s, %s, %s>" % (T, _b(g2), _b(relu), _b(red)), "ubr_bn_bwd", "_bn_frozen",
                        shape=SHP, relu=relu, ga2=g2, red=red)
        add(T, "channel_sum_kernel<%s>" % T, "ubr_channel_sum", "channel_sum", shape=SHP)
        for S in (1, 2):
            for xf in (False, True):
                for am in (False, True):
                    for xc in ((False, True) if S == 2 else (False,)):
                        add(T, "maxpool_fwd_kernel<%s, %d, %s, %s, %s>" % (T, S, _b(xf), _b(am), _b(xc)), "ubr_maxpool_fwd", "_pool", bwd=False,
                            shape=SHP_EVEN if xc else SHP, stride=S, xf=xf, argmax=am, xcopy=xc, slice_ps=C2, slice_off=48)
        add(T, ("maxpool_bwd_s2_amax_kernel<%s>" % T, "maxpool_bwd_s2_kernel<%s>" % T), "ubr_maxpool_bwd", "_pool", bwd=True, shape=SHP_EVEN, stride=2, argmax=True)
        add(T, "maxpool_bwd_kernel<%s>" % T, "ubr_maxpool_bwd", "_pool", bwd=True, shape=SHP, stride=1, xf=False)
        add(T, "stem_expand_kernel<%s>" % T, "ubr_stem_expand", "stem_expand", shape=(2, 13, 21, 32))
        add(T, "logsoftmax_bwd_kernel<%s>" % T, "ubr_logsoftmax_bwd", "logsoftmax_bwd", shape=(2, 13, 21, 16), classes=3)
    add("float", "nll_bwd_kernel", "ubr_pixelwise_nll_bwd", "nll_bwd", shape=(2, 3, 13, 21))
    return rows


def _check_rows():
    rows = []

    def add(T, sym, entry, module, fn, *args):
        rows.append(dict(symbols=tuple(sym), op="check", dtype=T, entry=entry, args=(module, fn, args), env=None))

    P = "test_gpu_param_exact"
    for T in DTYPES:
        for Cout in (16, 32):
            sym = ["stem_wgrad_kernel<%s, %d>" % (T, Cout), "stem_wgrad_reduce_kernel", "stem_fwd_kernel<%s>" % T]
            add(T, sym, "ubr_stem_wgrad", "test_gpu_ops", "_stem_exact", "DT", 2, 3, 21, 37, Cout)
        add(T, ["pack_kernel<%s>" % T, "pack_batched_kernel<%s>" % T], "ubr_pack_weights", P, "test_pack_edge_extents_on_both_entry_points",
            "PACK_EDGES[M3-K20-t9-A]", "DT", "CAPSYS")
        add(T, ["aspp_front_kernel<%s>" % T], "ubr_aspp_front", "test_gpu_aspp_front_exact", "test_aspp_front_exact", (1, 5, 3, 64), "DT")
    add("float", ["bn_fold_batched_kernel"], "ubr_bn_fold_batched", P, "test_bn_fold_extents_null_bias_zero_variance_and_cancellation", "CAPSYS")
    add("float", ["bn_finalize_kernel"], "ubr_bn_finalize", P, "run_bn_finalize", 48, 546.0, 0.1, True, 1e-5)
    add("float", ["bn_eval_affine_kernel"], "ubr_bn_eval_affine", P, "run_bn_eval_affine", 48, 1e-5)
    add("float", ["bn_bwd_finalize_kernel"], "ubr_bn_bwd_finalize", P, "run_bn_bwd_finalize", 48, 546.0, True, True, True)
    add("float", ["bn_bwd_finalize_frozen_kernel"], "ubr_bn_bwd_finalize_frozen", P, "run_bn_bwd_finalize", 48, None, True, True, False, True)
    add("float", ["cast_f64_kernel"], "ubr_cast_f64_to_f32", P, "run_cast", 147, 160, 8, 0.5, True)
    add("float", ["adam_kernel"], "ubr_adam_step", P, "test_adam_step_is_within_its_running_error_bound", 1020, 2, 1e-4, 1e-3, 1.0, "CAPSYS")
    add("float", ["sgd_kernel"], "ubr_sgd_step", P, "test_sgd_step_is_within_its_running_error_bound", 1020, 0.9, 0.5, 1, 0, 1.0, "CAPSYS")
    add("float", ["crop_tiles_kernel", "stitch_tiles_kernel"], "ubr_crop_tiles", P, "test_crop_and_stitch_move_exactly_the_pixels_of_the_descriptors",
        "overhang-40x70", 1, "CAPSYS")
    add("float", ["nll_fwd_kernel", "confusion_kernel"], "ubr_pixelwise_nll_fwd", "test_gpu_stream_exact", "test_nll_counts_bad_labels_and_confusion_is_exact")
    return rows


def _shape(r):
    a = r["args"]
    if r["op"] == "stream":
        return "%s %s" % ("x".join(map(str, a[1]["shape"])), " ".join("%s=%s" % (k, v) for k, v in sorted(a[1].items()) if k not in ("shape", "dt") and v not in (None, False, 0)))
    if r["op"] == "check":
        return "%s(%s)" % (a[1].replace("test_", "")[:28], ", ".join(str(x) for x in a[2] if x not in ("DT", "CAPSYS")))
    if r["op"] == "conv":
        return "N%d %dx%d Cin%d Cout%d k%s hint%d" % (a["N"], a["OH"], a["OW"], a["Cin"], a["Cout"], a["k"], a["tile_hint"])
    return "N%d %dx%d Cin%d Cout%d k%d dil%d" % (a["N"], a["GH"], a["GW"], a["Cin"], a["Cout"], a["k"], a.get("dil", 1))


def _make_rows():
    rows = _conv_rows() + _wgrad_rows() + _stream_rows() + _check_rows()
    for r in rows:
        s = r["symbols"][0].replace("_kernel<", "-").replace(">", "").replace(", ", "-")
        r["id"] = s + ("-" + r["tag"] if r.get("tag") else "") + ("-env" if r["env"] else "")
        r["shape"] = _shape(r)
    return rows


ROWS = _make_rows()
BY_ID = {r["id"]: r for r in ROWS}


# ------------------------------------------------------------------------------------------------------------------
# running a row (GPU): the replay functions and checks of test_gpu_kernels_exact.py on a record built from the row
# ------------------------------------------------------------------------------------------------------------------
def record(row):
    """the row as a call record of test_gpu_kernels_exact.py (replay_conv / replay_wgrad)"""
    import torch
    import kref
    import test_gpu_kernels_exact as X
    from ubresnet_amd import ops
    dt = {"float": torch.float32, "bf16_t": torch.bfloat16, "f16_t": torch.float16}[row["dtype"]]
    a = row["args"]
    cpu = kref.CPU[dt]
    if row["op"] == "wgrad":
        k, dil, N, GH, GW, Cin, Cout = a["k"], a.get("dil", 1), a["N"], a["GH"], a["GW"], a["Cin"], a["Cout"]
        taps = tuple(_wtaps(k, dil))
        rec = dict(x=X._Fake((N, GH, GW, Cin), dt).tv(), g=X._Fake((N, GH, GW, Cout), dt).tv(), taps=taps, dst=Cout * Cin * k * k,
                   sm=Cin * k * k, sk=k * k, Cout_valid=Cout, Cin_valid=Cin, S=1, iy0=0, ix0=0,
                   xf=("affine", (0.0,) * Cin) if a.get("xf") else None, accumulate=False, dst_offset=0, exclusive=False, defer=True)
        return {"op": "wgrad", "a": rec, "kernel": row["symbols"][0]}
    N, OH, OW, Cin, Cout = a["N"], a["OH"], a["OW"], a["Cin"], a["Cout"]
    if a["k"] == "phase":
        taps, nimg = tuple(ops.transposed_phase_taps(4, 1, 1, 2, 0, 0)), 16
    else:
        taps, nimg = tuple(ops.conv_taps(a["k"], 1, a["k"] // 2)), a["k"] * a["k"]
    if a.get("logsoftmax"):
        y = X._Fake((N, Cout, OH, OW), torch.float32)
    else:
        w = a.get("ywidth", Cout)
        y = X._Fake((N, OH, OW, Cout), dt, stride=(OH * OW * w, OW * w, w, 1), off=a.get("yoff", 0))
    dense = lambda: X._Fake((N, OH, OW, Cout), dt).tv()
    want_stats = a.get("stats") or a.get("bnb")
    rec = dict(x=X._Fake((N, OH, OW, Cin), dt).tv(), wp=(nimg, Cin // cpu, (Cout + 15) // 16 * 16, cpu), y=y.tv(), taps=taps, Cout=Cout, S=1,
               iy0=0, ix0=0, xf=("affine", (0.0,) * Cin) if a.get("xf") else None, bias=("bias", Cout) if a.get("bias") else None,
               addend=dense() if a.get("addend") else None, stats=("stats", 2 * Cout * kref.STAT_SLOTS) if want_stats else None,
               logsoftmax=bool(a.get("logsoftmax")), tile_hint=a["tile_hint"], act=a.get("act", 0),
               addend_mask=("addend_mask", N * OH * OW * (Cout // cpu)) if a.get("mask") else None,
               bnb=("bnb", dense()) if a.get("bnb") else None, stats_slots=0)
    return {"op": "conv", "a": rec, "kernel": row["symbols"][0]}


def launch_log(on=None):
    """on True / False: clear the library's launch log and switch it on / off; None: the set of normalized names it holds"""
    import ctypes as C
    import kernel_symbols
    from ubresnet_amd import _lib as L
    lib = L.lib()
    if on is not None:
        L.check(lib.ubr_launch_log(1 if on else 0), "launch_log")
        return None
    n = lib.ubr_launch_log_read(None, 0)
    buf = C.create_string_buffer(n)
    lib.ubr_launch_log_read(buf, n)
    return set(kernel_symbols.normalize(buf.value.decode().split("\n")))


class _NoCapture:
    """stands in for pytest's capsys where an existing check prints its table row"""
    def disabled(self):
        import contextlib
        return contextlib.nullcontext()


def _run_conv_wgrad(row):
    import test_gpu_kernels_exact as X
    from ubresnet_amd import ops
    orig = {"conv": ops.conv, "phases": ops.conv_phases, "wgrad": ops.wgrad}
    res, kern, _, _ = X.replay(record(row), orig)       # asserts that the library names the row's first symbol
    assert kern == row["symbols"][0], "the library names %s, the row declares %s" % (kern, row["symbols"][0])
    return res


def _run_stream(row):
    import torch
    import test_gpu_stream_exact as S
    builder, kw = row["args"]
    kw = dict(kw)
    dt = getattr(torch, TORCH_DT[kw.pop("dt")])
    shape = kw.pop("shape")
    if builder == "tail_fwd":
        rec = S._case("block_tail_fwd", c2=S._v(shape, dt), sc=S._v(shape, dt), mean_b=True if kw["byp"] else None,
                      out=S._v(shape, dt, C2, 48), relu_mask=True if kw["mask"] else None)
    elif builder == "channel_sum":
        rec = S._case("channel_sum", g=S._v(shape, dt, C2, 48))
    elif builder == "stem_expand":
        rec = S._case("stem_expand", out=S._v(shape, dt))
    elif builder == "logsoftmax_bwd":
        rec = S._case("logsoftmax_bwd", logp=("t", "torch.float32", (shape[0], kw["classes"], shape[1], shape[2])), g_logits=S._v(shape, dt))
    elif builder == "nll_bwd":
        rec = S._case("pixelwise_nll_bwd", classw=True, ignore_index=-100, shape=shape)
    else:
        rec = getattr(S, builder)(shape=shape, dt=dt, **kw)
    return S.REPLAY[rec["op"]](rec["a"], rec["op"])[0]


def _run_check(row):
    import importlib
    import torch
    module, fn, args = row["args"]
    m = importlib.import_module(module)
    real = []
    for x in args:
        if x == "DT":
            x = getattr(torch, TORCH_DT[row["dtype"]])
        elif x == "CAPSYS":
            x = _NoCapture()
        elif isinstance(x, str) and x.startswith("PACK_EDGES["):
            x = [c for c in m.PACK_EDGES if c[0] == x[11:-1]][0]
        real.append(x)
    getattr(m, fn)(*real)          # raises on a mismatch
    return "exact"


def run_row(row):
    """run the row's call with the launch log on: the outputs against the fp64 reference by the replay or check the row names (bit for
    bit, sums exact or within kref's bound, sentinels untouched), and the log against the row's symbols.  -> (result, milliseconds)"""
    import time
    import torch
    run = {"conv": _run_conv_wgrad, "wgrad": _run_conv_wgrad, "stream": _run_stream, "check": _run_check}[row["op"]]
    launch_log(True)
    t0 = time.perf_counter()
    try:
        res = run(row)
        torch.cuda.synchronize()
        logged = launch_log()
    finally:
        launch_log(False)
    ms = 1e3 * (time.perf_counter() - t0)
    assert logged == set(row["symbols"]), "launched %s, the row declares %s" % (sorted(logged), sorted(row["symbols"]))
    return res, ms


def _main(argv):
    repo = os.path.dirname(HERE)
    if repo not in sys.path:
        sys.path.insert(0, repo)
    row = BY_ID[argv[1]]
    for k, v in (row["env"] or {}).items():
        assert os.environ.get(k) == v, "%s must be %s in this process" % (k, v)
    res, ms = run_row(row)
    print("RESULT %s %.1f" % (res, ms))
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv))
