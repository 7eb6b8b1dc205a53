"""Stage checks in the storage types: a launch tap over ubresnet_amd.ops, a per-launch fp64 replay of what the tap recorded, and a
dataflow check of the recorded tape against the launch graph the module's own dataflow demands.  A helper module for the tests
(imported by name, like kref.py; not a conftest).

  * Tap wraps the operator entry points the stage functions of ubresnet_amd.engine call.  Every call becomes a Launch: the op name
    and its arguments by parameter name; a tensor argument becomes a TRec (address, shape, strides, dtype, a host copy taken
    BEFORE the call, and for the op's outputs a host copy -- of the view and of its whole storage -- taken after a synchronize).
  * replay() recomputes every launch in fp64 from ITS OWN recorded inputs with the references of kref.py and compares the recorded
    outputs with kref's bounds.  Nothing compounds from launch to launch.
  * Graph is the expected launch graph, written down from BasicBlock / DoubleResNet / ConvTransposeLayer / the ASPP level (expect_block_fwd, ...),
    never from the tape: which buffer feeds which launch, which BatchNorm site's vectors are the on-load affine of which conv and
    weight gradient, which packed image and gradient view a launch names, which reduction slice goes with which site, how long
    the ReLU mask is in this dtype.  Graph.match() binds the tape to it edge by edge.
  * expect_stem_pool_*, expect_head_*, expect_uresnet and expect_aspp_net compose these into the stem, the head and the whole
    passes: which channel slice of which concat buffer an encoder level writes and a decoder level reads, which gradient slice a
    level is owed, the per-plane image / addend / dst_offset of the stem launches, the arena affines of ASPP_ResNet's decoder,
    the fresh NCHW output.  The harness's cost does not grow with storage size x launches (BIG_STORAGE below).
  * emulate() stands in for the kernels on the CPU (each launch writes its reference rounded once to the stored type, kref.round_to),
    so that the tap, the replay, the graphs and the chain can be exercised without a device.  Its error ratios are at most
    about 1 by construction: they show the plumbing, never that a bound is right (the device run measures that).
"""
import inspect
import math

import torch

import kref
from ubresnet_amd import ops as OPS

U32 = kref.U32

# op -> the parameters a launch writes (after flattening: an Affine `xf` becomes xf.sub ..., a bn_fwd_fin descriptor fin2.stats ...)
OUTS = {
    "conv": ("y", "stats"),
    "conv_phases": ("y_full",),
    "wgrad": (),                 # the slabs; the gradient view is final after the stage's flush (check_gradients)
    "bn_finalize": ("scale", "shift", "mean", "invstd", "rmean", "rvar", "nbt"),
    "bn_eval_affine": ("scale", "shift", "mean", "invstd"),
    "block_tail_fwd": ("out", "relu_mask"),
    "block_tail_fwd_fin": ("out", "relu_mask") + tuple("%s.%s" % (f, v) for f in ("fin2", "fin_b")
                                                       for v in ("scale", "shift", "mean", "invstd", "rmean", "rvar", "nbt")),
    "block_tail_bwd_reduce": ("red2", "red_b"),
    "block_tail_bwd_apply": ("g_c2", "g_sc"),
    "block_tail_bwd_apply_fin": ("g_c2", "g_sc", "dgamma2", "dbeta2", "dgamma_b", "dbeta_b"),
    "block_tail_bwd_frozen": ("g_c2", "g_sc", "red2", "red_b"),
    "bn_bwd_reduce": ("red",),
    "bn_bwd_apply": ("gc",),
    "bn_bwd_apply_fin": ("gc", "dgamma", "dbeta"),
    "bn_bwd_frozen": ("gc", "red"),
    "bn_bwd_finalize": ("dgamma", "dbeta", "k1", "k2"),
    "bn_bwd_finalize_frozen": ("dgamma", "dbeta", "k1", "k2"),
    "maxpool_fwd": ("pooled", "xcopy", "argmax"),
    "maxpool_bwd": ("gx",),
    "channel_sum": ("red",),
    "cast_f64_to_f32": ("dst",),
    "stem_expand": ("out",),             # the engine keeps these two off a plan's tape (_untaped); they are ops entry points all the same
    "logsoftmax_bwd": ("g_logits",),
}
WRAPPED = tuple(OUTS) + ("bn_fwd_fin",)


def _deep(v):
    """nested lists as nested tuples"""
    return tuple(_deep(q) for q in v) if isinstance(v, (list, tuple)) else v


def _host(t):
    return t.detach().to("cpu", copy=True)


def _storage(t):
    """the whole storage under a view, as a flat host tensor of the view's dtype"""
    n = t.untyped_storage().nbytes() // t.element_size()
    return _host(torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage(), 0, (n,)))


# A storage of more than this many bytes (the flat gradient buffer of a whole network, the reduction arenas) is not copied to the
# host twice per launch that writes into it: the bytes outside the launch's output views are compared ON THE DEVICE, before
# against after, at record time, and the record keeps the verdict (TRec.outside) and ONE host copy of the storage as it was when
# the tape first saw it (TRec.base_init, shared by every record of that storage).  Smaller storages keep both host copies.
BIG_STORAGE = 1 << 20


def _flat_dev(t):
    """the whole storage under a view as a flat tensor of the view's dtype, where it lives"""
    n = t.untyped_storage().nbytes() // t.element_size()
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage(), 0, (n,))


class TRec:
    """a tensor argument as one launch saw it"""

    def __init__(self, t, out, inits=None):
        self.ptr, self.shape, self.stride, self.dtype = t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype
        self.before = _host(t)
        self.after = None
        self.base, self.off = t.untyped_storage().data_ptr(), t.storage_offset()
        self.big = bool(out) and inits is not None and t.untyped_storage().nbytes() > BIG_STORAGE
        self.base_before = _storage(t) if out and not self.big else None
        self.base_after = None
        self.base_init, self.outside = None, None
        if self.big:
            key = (self.base, t.untyped_storage().nbytes(), t.dtype)
            if key not in inits:
                inits[key] = _storage(t)
            self.base_init = inits[key]
        self._t = t if out else None

    def finish(self):
        self.after, self.base_after, self._t = _host(self._t), (None if self.big else _storage(self._t)), None

    def init(self):
        """the storage before the launch (small storages), or as the tape first saw it"""
        return self.base_before if self.base_before is not None else self.base_init

    def nbytes(self):
        return kref.TV.make(self.shape, self.stride, self.dtype, 0, self.ptr).extent() * self.before.element_size()


class Launch:
    def __init__(self, op, args):
        self.op, self.args = op, args

    def __repr__(self):
        return "<%s %s>" % (self.op, " ".join("%s=%s" % (k, "x".join(map(str, v.shape)) if isinstance(v, TRec) else v)
                                             for k, v in self.args.items() if v is not None and k != "taps"))


_FIN = ("stats", "gamma", "beta", "rmean", "rvar", "nbt", "scale", "shift", "mean", "invstd")


class Tap:
    """with pytest's monkeypatch: every wrapped ops entry point records a Launch into .tape, in call order"""

    def __init__(self, monkeypatch, sync=None):
        self.tape = []
        self._fins = {}
        self._inits = {}        # (storage address, bytes, dtype) -> host copy of a big storage as the tape first saw it
        self._sync = sync if sync is not None else (torch.cuda.synchronize if torch.cuda.is_available() else (lambda: None))
        for name in WRAPPED:
            monkeypatch.setattr(OPS, name, self._wrap(name, getattr(OPS, name)))

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapper(*args, **kwargs):
            ba = sig.bind(*args, **kwargs)
            ba.apply_defaults()
            if name == "bn_fwd_fin":        # a descriptor, not a launch: remember which tensors it names
                d = fn(*args, **kwargs)
                p, bn = ba.arguments, ba.arguments["bn"]
                track = bn.track_running_stats and bn.running_mean is not None
                self._fins[id(d)] = (d, dict(stats=p["stats"], gamma=bn.weight, beta=bn.bias, rmean=bn.running_mean if track else None,
                                             rvar=bn.running_var if track else None, nbt=bn.num_batches_tracked if track else None,
                                             scale=p["scale"], shift=p["shift"], mean=p["mean"], invstd=p["invstd"],
                                             momentum=bn.momentum, eps=bn.eps))
                return d
            flat = {}
            for k, v in ba.arguments.items():
                if isinstance(v, OPS.Affine):
                    for f in ("sub", "scale", "shift", "lo"):
                        flat["%s.%s" % (k, f)] = getattr(v, f)
                elif id(v) in self._fins and self._fins[id(v)][0] is v:
                    for f, t in self._fins[id(v)][1].items():
                        flat["%s.%s" % (k, f)] = t
                elif k in ("xf", "fin2", "fin_b"):
                    for f in (("sub", "scale", "shift", "lo") if k == "xf" else _FIN):
                        flat["%s.%s" % (k, f)] = None
                elif isinstance(v, (torch.Tensor, int, float, bool, type(None))):
                    flat[k] = v
                elif k in ("taps", "phases"):
                    flat[k] = _deep(v)
                # (workspaces, streams, deferred-reduction batches: not part of the record)
            outs = OUTS[name]
            self._sync()
            rec = {k: TRec(v, k in outs, self._inits) if isinstance(v, torch.Tensor) else v for k, v in flat.items()}
            big = {}          # storage address -> (its bytes before the launch, on the device; the map of what the launch may write)
            for k in outs:
                if isinstance(rec.get(k), TRec) and rec[k].big:
                    t = flat[k]
                    if rec[k].base not in big:
                        big[rec[k].base] = (_flat_dev(t).clone(), torch.zeros(_flat_dev(t).numel(), dtype=torch.bool, device=t.device), t)
                    big[rec[k].base][1].as_strided(t.shape, t.stride(), t.storage_offset()).fill_(True)
            r = fn(*args, **kwargs)
            self._sync()
            verdict = {}
            for base, (before, written, t) in big.items():
                bad = (kref.bits(_flat_dev(t)) != kref.bits(before)) & ~written
                verdict[base] = (int(bad.sum()), int(bad.nonzero()[0]) if bool(bad.any()) else -1)
            for k in outs:
                if isinstance(rec.get(k), TRec):
                    rec[k].finish()
                    if rec[k].big:
                        rec[k].outside = verdict[rec[k].base]
            self.tape.append(Launch(name, rec))
            return r
        wrapper.__wrapped__ = fn
        return wrapper


# ------------------------------------------------------------------------------------------------------------------
# references: op -> {output parameter: expectation}.  `a` holds the launch's arguments with tensors as host tensors (the values
# BEFORE the call); `post` the values after it where the launch was recorded (None while emulating).
#   ("within", ref, lim)        |got - ref| <= lim per element (lim == 0: equality)
#   ("bits", t)                 the bits of t
#   ("either", t0, t1)          element for element the bits of t0 or of t1 (kref.bn_finalize_ref's two evaluations)
#   ("stripes", ref, lim, n)    a striped fp64 accumulator [slots][len(ref)]: what the launch ADDED, summed over the stripes, within lim;
#                               n > 0: stripes from n on stay as they were
# ------------------------------------------------------------------------------------------------------------------
def _xf(a, k="xf"):
    if a.get(k + ".scale") is None:
        return None
    return tuple(a["%s.%s" % (k, f)] for f in ("sub", "scale", "shift", "lo"))


_stored = kref.stored_bound
_conv_stats = kref.conv_stats_bound


def ref_conv(a, post):
    x, y, taps, Cout = a["x"], a["y"], a["taps"], a["Cout"]
    assert a["bnb"] is None, "replay covers the forms the stage functions launch"
    dt, Cin = x.dtype, x.shape[3]
    N, OH, OW = (y.shape[0], y.shape[2], y.shape[3]) if a["logsoftmax"] else (y.shape[0], y.shape[1], y.shape[2])
    W = kref.unpack_weights(a["wp"], Cin, Cout)
    xf = _xf(a)
    geo = dict(S=a["S"], iy0=a["iy0"], ix0=a["ix0"])
    ref, ab = kref.conv_ref(x, W, taps, Cout, OH, OW, xf=xf, bias=a["bias"], addend=a["addend"], addend_mask=a["addend_mask"],
                            act=a["act"], **geo)
    K = len(taps) * Cin + (a["bias"] is not None) + (a["addend"] is not None)
    pre = kref.C_ACC * K * U32 * ab
    if xf is not None:
        pre = pre + kref.conv_ref(kref.xf_operand_err(x, xf, dt), W.abs(), taps, Cout, OH, OW, want_abs=False, **geo)[0]
    if a["logsoftmax"]:
        # the head: the fp32 logits never reach memory; the epilogue's log-softmax of them is stored as fp32 NCHW
        assert a["stats"] is None and a["addend"] is None and not a["act"] and y.dtype == torch.float32
        lsm, lim = kref.logsoftmax_bound(ref, pre)
        return {"y": ("within", lsm.permute(0, 3, 1, 2).contiguous(), lim.permute(0, 3, 1, 2).contiguous())}
    out = {"y": ("within", ref, _stored(ref, pre, dt))}
    if a["stats"] is not None:
        s, l = _conv_stats(ref, pre, N, OH, OW)
        out["stats"] = ("stripes", s, l, a["stats_slots"])
    return out


def ref_conv_phases(a, post):
    x, yf, Cout, phases = a["x"], a["y_full"], a["Cout"], a["phases"]
    dt, Cin = x.dtype, x.shape[3]
    OH, OW = yf.shape[1] // 2, yf.shape[2] // 2
    W = kref.unpack_weights(a["wp"], Cin, Cout)
    xf = _xf(a)
    ref, ab = kref.conv_phases_ref(x, W, phases, Cout, OH, OW, xf=xf, bias=a["bias"], addend_full=a["addend_full"])
    K = max(len(p[2]) for p in phases) * Cin + (a["bias"] is not None) + (a["addend_full"] is not None)
    pre = kref.C_ACC * K * U32 * ab
    if xf is not None:
        pre = pre + kref.conv_phases_ref(kref.xf_operand_err(x, xf, dt), W.abs(), phases, Cout, OH, OW)[0]
    assert bool(torch.isfinite(ref).all()), "the four phases cover the output"
    return {"y_full": ("within", ref, _stored(ref, pre, dt))}


def ref_wgrad(a):
    """-> (dW fp64 [ntaps][Cout][Cin], lim): fp32 sums over K = N*GH*GW pixels in any order (slabs included), fp32 store"""
    x, g = a["x"], a["g"]
    xf = _xf(a)
    geo = dict(S=a["S"], iy0=a["iy0"], ix0=a["ix0"])
    ref, ab = kref.wgrad_ref(x, g, a["taps"], xf=xf, **geo)
    if x.dtype == torch.float16:
        # f16 subnormal operands enter the matrix cores at the nominal exponent 2^-14 (kref.nominal_abs: the derivation): the
        # sum of |terms| the accumulation error is charged on takes them at that magnitude.  Nothing changes for normal operands.
        ab = kref.wgrad_ref(kref.nominal_abs(kref._xform(x, xf), x.dtype), kref.nominal_abs(g, g.dtype), a["taps"], want_abs=False, **geo)[0]
    K = g.shape[0] * g.shape[1] * g.shape[2]
    pre = kref.C_ACC * K * U32 * ab
    if xf is not None:
        pre = pre + kref.wgrad_ref(kref.xf_operand_err(x, xf, x.dtype), g.double().abs(), a["taps"], want_abs=False, **geo)[0]
    return ref, _stored(ref, pre, torch.float32)


def _finalize(stats, slots, count, gamma, beta, eps, rmean, rvar, momentum, nbt):
    C = gamma.numel()
    s = kref.stripe_sum(stats.reshape(-1), slots, 2 * C, 2 * C)
    mom = kref.f32(momentum)
    e = [kref.bn_finalize_ref(s[:C], s[C:], float(count), gamma, beta, eps, rmean, rvar, mom, fused=f) for f in (False, True)]
    out = {n: ("either", e[0][i], e[1][i]) for i, n in enumerate(("scale", "shift", "mean", "invstd"))}
    if rmean is not None:
        out["rmean"], out["rvar"] = ("either", e[0][4], e[1][4]), ("either", e[0][5], e[1][5])
    if nbt is not None:
        out["nbt"] = ("bits", nbt + 1)
    return out


def ref_bn_finalize(a, post):
    return _finalize(a["stats"], kref.STAT_SLOTS, a["count"], a["gamma"], a["beta"], a["eps"], a["rmean"], a["rvar"], a["momentum"], a["nbt"])


def ref_bn_eval_affine(a, post):
    (inv, li), (sc, ls) = kref.bn_eval_affine_bound(a["gamma"], a["rvar"], a["eps"])
    return {"invstd": ("within", inv, li), "scale": ("within", sc, ls),
            "shift": ("bits", a["beta"].clone()), "mean": ("bits", a["rmean"].clone())}


def _tail_fwd(a, v2, vb):
    c2, sc = a["c2"], a["sc"]
    dt = c2.dtype
    ref, lim = kref.tail_fwd_bound(c2, v2[0], v2[1], v2[2], sc, dt, *(vb if vb is not None else (None, None, None)))
    out = {"out": ("within", ref, lim)}
    if a["relu_mask"] is not None:
        out["relu_mask"] = ("mask", kref.CPU[dt])          # the bits of the STORED output, whatever it is
    return out


def ref_block_tail_fwd(a, post):
    vb = (a["mean_b"], a["scale_b"], a["shift_b"]) if a["mean_b"] is not None else None
    return _tail_fwd(a, (a["mean2"], a["scale2"], a["shift2"]), vb)


def ref_block_tail_fwd_fin(a, post):
    out, vec = {}, {}
    for f in ("fin2", "fin_b"):
        if a[f + ".stats"] is None:
            vec[f] = None
            continue
        g = lambda n: a["%s.%s" % (f, n)]
        e = _finalize(g("stats"), kref.RED_SLOTS, a["count"], g("gamma"), g("beta"), g("eps"), g("rmean"), g("rvar"), g("momentum"), g("nbt"))
        for n, v in e.items():
            out["%s.%s" % (f, n)] = v
        # the elementwise part reads the vectors the launch itself made: checked above, taken as stored
        vec[f] = tuple(post["%s.%s" % (f, n)] if post is not None else e[n][1] for n in ("mean", "scale", "shift"))
    out.update(_tail_fwd(a, vec["fin2"], vec["fin_b"]))
    return out


def _tail_bwd(a):
    c2 = a["c2"]
    dt = c2.dtype
    if a.get("relu_mask") is not None:
        pos = kref.mask_unpack(a["relu_mask"], c2.shape, kref.CPU[dt])
    else:
        pos = a["out"].double() > 0
    gz, gy2, xh2, xhb = kref.tail_bwd_ref(a["go"], a["go2"], pos, c2, a["scale2"], a["shift2"], a["mean2"], a["invstd2"],
                                          a["cb"], a["mean_b"], a["invstd_b"])
    bn, terms, _ = kref.affine_terms(c2, a["mean2"], a["scale2"], a["shift2"])
    return dt, gz, gy2, xh2, xhb, kref.gate_open(bn, terms) & (gz != 0), 1 if a["go2"] is not None else 0


def ref_block_tail_bwd_reduce(a, post):
    dt, gz, gy2, xh2, xhb, opn, extra = _tail_bwd(a)
    C = gz.shape[-1]
    L = kref.reduce_chain(gz.numel() // C, C, dt)
    # (an open gate: the term the kernel summed is gz or 0; reduce_bound adds |term| of the reference's branch, so hand it gz there)
    gyo = torch.where(opn, gz, gy2)
    s, sx, l1, l2 = kref.reduce_bound(gy2, xh2, L, None, extra)
    _, _, o1, o2 = kref.reduce_bound(gyo * opn, xh2, 0, opn, 0)
    out = {"red2": ("stripes", torch.cat([s, sx]), torch.cat([l1 + o1, l2 + o2]), kref.RED_SLOTS)}
    if a["cb"] is not None:
        s, sx, l1, l2 = kref.reduce_bound(gz, xhb, L, None, extra)
        out["red_b"] = ("stripes", torch.cat([s, sx]), torch.cat([l1, l2]), kref.RED_SLOTS)
    return out


def _tail_apply(a, k2v, kbv, kx):
    dt, gz, gy2, xh2, xhb, opn, extra = _tail_bwd(a)
    ref, lim = kref.apply_bound(gy2, xh2, a["scale2"], k2v[0], k2v[1], dt, extra + kx)
    lim = lim + opn * (a["scale2"].double().abs() * gz.abs()) * (1 + kref.UNIT_ROUNDOFF[dt])
    out = {"g_c2": ("within", ref, lim)}
    if a["g_sc"] is not None:
        if a["cb"] is not None:
            out["g_sc"] = ("within",) + kref.apply_bound(gz, xhb, a["scale_b"], kbv[0], kbv[1], dt, extra + kx)
        else:       # the gated gradient itself: exact with one operand, one fp32 sum and a store with two
            out["g_sc"] = ("within", gz, (kref.bound(gz, gz.abs(), dt, 1) + kref.TINY[dt] * (gz != 0)) * extra)
    return out


def ref_block_tail_bwd_apply(a, post):
    return _tail_apply(a, (a["k1_2"], a["k2_2"]), (a["k1_b"], a["k2_b"]), 0)


def ref_block_tail_bwd_apply_fin(a, post):
    C = a["c2"].shape[-1]
    dg, db, k1, k2 = kref.bn_bwd_finalize_ref(a["red2"], C, float(a["count"]), slots=kref.RED_SLOTS)
    out = {"dgamma2": ("bits", dg), "dbeta2": ("bits", db)}
    kb = None
    if a["cb"] is not None:
        dgb, dbb, k1b, k2b = kref.bn_bwd_finalize_ref(a["red_b"], C, float(a["count"]), slots=kref.RED_SLOTS)
        out["dgamma_b"], out["dbeta_b"], kb = ("bits", dgb), ("bits", dbb), (k1b, k2b)
    out.update(_tail_apply(a, (k1, k2), kb, 1))
    return out


def _bn_bwd(a):
    c = a["c"]
    gy, xh = kref.bn_bwd_ref(a["ga"], a["ga2"], c, a["scale"], a["shift"], a["mean"], a["invstd"], bool(a["relu"]))
    g = a["ga"].double() if a["ga2"] is None else a["ga"].double() + a["ga2"].double()
    bn, terms, _ = kref.affine_terms(c, a["mean"], a["scale"], a["shift"])
    opn = (kref.gate_open(bn, terms) & (g != 0)) if a["relu"] else torch.zeros_like(bn, dtype=torch.bool)
    return c.dtype, g, gy, xh, opn, 1 if a["ga2"] is not None else 0


def ref_bn_bwd_reduce(a, post):
    dt, g, gy, xh, opn, extra = _bn_bwd(a)
    C = g.shape[-1]
    L = kref.reduce_chain(g.numel() // C, C, dt)
    s, sx, l1, l2 = kref.reduce_bound(gy, xh, L, None, extra)
    _, _, o1, o2 = kref.reduce_bound(g * opn, xh, 0, opn, 0)
    return {"red": ("stripes", torch.cat([s, sx]), torch.cat([l1 + o1, l2 + o2]), kref.RED_SLOTS)}


def _bn_apply(a, k1, k2, kx):
    dt, g, gy, xh, opn, extra = _bn_bwd(a)
    ref, lim = kref.apply_bound(gy, xh, a["scale"], k1, k2, dt, extra + kx)
    return {"gc": ("within", ref, lim + opn * (a["scale"].double().abs() * g.abs()) * (1 + kref.UNIT_ROUNDOFF[dt]))}


def ref_bn_bwd_apply(a, post):
    return _bn_apply(a, a["k1"], a["k2"], 0)


def ref_bn_bwd_apply_fin(a, post):
    C = a["c"].shape[-1]
    dg, db, k1, k2 = kref.bn_bwd_finalize_ref(a["red"], C, float(a["count"]), slots=kref.RED_SLOTS)
    out = {"dgamma": ("bits", dg), "dbeta": ("bits", db)}
    out.update(_bn_apply(a, k1, k2, 1))
    return out


def ref_bn_bwd_finalize(a, post):
    assert not a["accumulate"]
    dg, db, k1, k2 = kref.bn_bwd_finalize_ref(a["red"], a["Cn"], float(a["count"]))
    return {"dgamma": ("bits", dg), "dbeta": ("bits", db), "k1": ("bits", k1), "k2": ("bits", k2)}


def _scaled(gy, scale, dt, extra, opn, g):
    """g_c = scale * g_y of a frozen site: one product (+ `extra` of g_y), then the store; an open gate adds the whole term"""
    sc = scale.double()
    ref = sc * gy
    lim = kref.bound(ref, ref.abs(), dt, 1 + extra) + kref.TINY[dt] * (ref != 0)
    if opn is not None:
        lim = lim + opn * (sc.abs() * g.abs()) * (1 + kref.UNIT_ROUNDOFF[dt])
    return ("within", ref, lim)


def ref_block_tail_bwd_frozen(a, post):
    a = dict(a, out=None)
    dt, gz, gy2, xh2, xhb, opn, extra = _tail_bwd(a)
    C = gz.shape[-1]
    L = kref.reduce_chain(gz.numel() // C, C, dt)
    out = {"g_c2": _scaled(gy2, a["scale2"], dt, extra, opn, gz)}
    s, sx, l1, l2 = kref.reduce_bound(gy2, xh2, L, None, extra)
    _, _, o1, o2 = kref.reduce_bound(torch.where(opn, gz, gy2) * opn, xh2, 0, opn, 0)
    out["red2"] = ("stripes", torch.cat([s, sx]), torch.cat([l1 + o1, l2 + o2]), kref.RED_SLOTS)
    if a["cb"] is not None:
        out["g_sc"] = _scaled(gz, a["scale_b"], dt, extra, None, None)
        s, sx, l1, l2 = kref.reduce_bound(gz, xhb, L, None, extra)
        out["red_b"] = ("stripes", torch.cat([s, sx]), torch.cat([l1, l2]), kref.RED_SLOTS)
    elif a["g_sc"] is not None:
        out["g_sc"] = ("within", gz, (kref.bound(gz, gz.abs(), dt, 1) + kref.TINY[dt] * (gz != 0)) * extra)
    return out


def ref_bn_bwd_frozen(a, post):
    dt, g, gy, xh, opn, extra = _bn_bwd(a)
    C = g.shape[-1]
    out = {"gc": _scaled(gy, a["scale"], dt, extra, opn, g)}
    if a["red"] is not None:
        L = kref.reduce_chain(g.numel() // C, C, dt)
        s, sx, l1, l2 = kref.reduce_bound(gy, xh, L, None, extra)
        _, _, o1, o2 = kref.reduce_bound(g * opn, xh, 0, opn, 0)
        out["red"] = ("stripes", torch.cat([s, sx]), torch.cat([l1 + o1, l2 + o2]), kref.RED_SLOTS)
    return out


def ref_bn_bwd_finalize_frozen(a, post):
    dg, db, k1, k2 = kref.bn_bwd_finalize_ref(a["red"], a["Cn"], None)
    out = {"dgamma": ("bits", dg), "dbeta": ("bits", db)}
    if a["k1"] is not None:
        out["k1"], out["k2"] = ("bits", k1), ("bits", k2)
    return out


def ref_maxpool_fwd(a, post):
    """The ASPP level pools stored values: no transform on load, no copy, no argmax; a maximum of stored values is one of them.
    The stem pools relu(bn1(c0)) formed on load, copies the transformed pixels into the skip half of cat1 and keeps each window's
    arg-max tap (kref.pool_xf_bound: the derivation)."""
    xf = _xf(a)
    if xf is None:
        assert a["xcopy"] is None and a["argmax"] is None
        pooled, _, _ = kref.maxpool_ref(a["x"], None, a["stride"])
        return {"pooled": ("within", pooled, torch.zeros_like(pooled))}
    assert a["stride"] == 2 and a["xcopy"] is not None, "the stem's form"
    pooled, lim_p, am, t, lim_t = kref.pool_xf_bound(a["x"], xf, a["stride"], a["x"].dtype)
    out = {"pooled": ("within", pooled, lim_p), "xcopy": ("within", t, lim_t)}
    if a["argmax"] is not None:
        out["argmax"] = ("amax", am, t, lim_t, pooled)
    return out


def _check_pool(i, L, exp, what):
    """the stem pool's outputs against each other: pooled is one of the STORED xcopy values -- the one at the recorded arg-max tap,
    which lies inside the image and whose fp64 value is within twice its own bound of the fp64 window maximum; without an arg-max,
    the maximum of the stored window"""
    pooled, xcopy, stride = L.args["pooled"].after, L.args["xcopy"].after, L.args["stride"]
    same = lambda p, q: (kref.bits(p) == kref.bits(q)) | ((p == 0) & (q == 0))
    if "argmax" in exp:
        _, am_ref, t, lim_t, best = exp["argmax"]
        am = L.args["argmax"].after
        got, inside = kref.window_take(xcopy, am, stride)
        assert bool(inside.all()), "%s: %d arg-max bytes name no pixel of the image" % (what, int((~inside).sum()))
        assert bool(same(pooled, got).all()), "%s: pooled differs from the stored xcopy at the recorded arg-max in %d elements" % (
            what, int((~same(pooled, got)).sum()))
        tv, _ = kref.window_take(t, am, stride)
        lv, _ = kref.window_take(lim_t, am, stride)
        bad = (best - tv) > 2 * lv
        assert not bool(bad.any()), "%s: %d recorded arg-max taps are not a maximum of their window within twice their bound" % (what, int(bad.sum()))
    else:
        got, _, _ = kref.maxpool_ref(xcopy, None, stride)
        assert bool(same(pooled, kref.round_to(got, pooled.dtype)).all()), "%s: pooled is not the maximum of the stored window" % what


def ref_maxpool_bwd(a, post):
    """gx = g_extra + the window gradients whose (first) maximum is this pixel: at most 10 terms summed in fp32, then the store.
    A launch that was handed an arg-max is replayed with the RECORDED one (the forward's check has vetted it): near-ties may have
    resolved either way, and the backward must follow the forward's choice."""
    x = a["x"]
    if a["argmax"] is not None:
        am = a["argmax"].long()
    else:
        _, am, _ = kref.maxpool_ref(x, _xf(a), a["stride"])
    hw = (x.shape[1], x.shape[2])
    ref = kref.maxpool_bwd_ref(a["g_pooled"], am, hw, a["stride"], a["g_extra"])
    ab = kref.maxpool_bwd_ref(a["g_pooled"].double().abs(), am, hw, a["stride"], a["g_extra"].double().abs() if a["g_extra"] is not None else None)
    return {"gx": ("within", ref, kref.bound(ref, ab, x.dtype, 9) + kref.TINY[x.dtype] * (ab > 0))}


def ref_channel_sum(a, post):
    """per-thread fp32 chains of ceil(npix * CU / (256 * workgroups)) pixels (grid: pick_blocks(npix, CU, 1024)), fp64 from there"""
    g = a["g"]
    C = g.shape[-1]
    npix, CU = g.numel() // C, C // kref.CPU[g.dtype]
    blocks = kref.pick_blocks(npix, CU, 1024)
    L = (npix * CU + 256 * blocks - 1) // (256 * blocks)
    s, _, a1, _ = kref.reduce_ref(g.double())
    return {"red": ("stripes", s, (kref.gamma(L) + 2.0 ** -50) * a1, 0)}


def ref_cast_f64_to_f32(a, post):
    assert not a["accumulate"]
    n = a["n"]
    return {"dst": ("bits", kref.cast_ref(a["src"], n if a["stride"] is None else a["stride"], a["slots"], n, a["scale"]))}


def ref_stem_expand(a, post):
    """a copy with a column shift: one rounding of the caller's fp32 pixel to the stored type, zeros elsewhere"""
    return {"out": ("bits", kref.round_to(kref.stem_expand_ref(a["x_nchw"]), a["out"].dtype))}


def ref_logsoftmax_bwd(a, post):
    """g_l = g - p * sum_c g with p = exp(logp) of the recorded log-probabilities, into 16 channels of which [ncls, 16) are zero
    bits.  kref.logsoftmax_bwd_ref's bound, and half a subnormal spacing of the stored type where the result is not zero (TINY: a
    nearly certain pixel's p * s reaches the subnormal range of f16)."""
    g, lp, out = a["g_logp"].double(), a["logp"].double(), a["g_logits"]
    ref, lim = kref.logsoftmax_bwd_ref(g, lp.exp(), out.dtype)
    lim = lim + kref.TINY[out.dtype] * (ref != 0)
    pad = (0, out.shape[-1] - ref.shape[-1])
    return {"g_logits": ("within", torch.nn.functional.pad(ref, pad), torch.nn.functional.pad(lim, pad))}


REFS = {"stem_expand": ref_stem_expand, "logsoftmax_bwd": ref_logsoftmax_bwd, "maxpool_fwd": ref_maxpool_fwd, "maxpool_bwd": ref_maxpool_bwd, "channel_sum": ref_channel_sum, "cast_f64_to_f32": ref_cast_f64_to_f32,
        "block_tail_bwd_frozen": ref_block_tail_bwd_frozen, "bn_bwd_frozen": ref_bn_bwd_frozen,
        "bn_bwd_finalize_frozen": ref_bn_bwd_finalize_frozen, "conv": ref_conv, "conv_phases": ref_conv_phases, "bn_finalize": ref_bn_finalize, "bn_eval_affine": ref_bn_eval_affine,
        "block_tail_fwd": ref_block_tail_fwd, "block_tail_fwd_fin": ref_block_tail_fwd_fin,
        "block_tail_bwd_reduce": ref_block_tail_bwd_reduce, "block_tail_bwd_apply": ref_block_tail_bwd_apply,
        "block_tail_bwd_apply_fin": ref_block_tail_bwd_apply_fin, "bn_bwd_reduce": ref_bn_bwd_reduce,
        "bn_bwd_apply": ref_bn_bwd_apply, "bn_bwd_apply_fin": ref_bn_bwd_apply_fin, "bn_bwd_finalize": ref_bn_bwd_finalize}


# ------------------------------------------------------------------------------------------------------------------
# replay
# ------------------------------------------------------------------------------------------------------------------
def _ratio(err, lim):
    """worst |err| / lim; an error where lim is 0 counts as infinite"""
    err, lim = err.reshape(-1), lim.reshape(-1).expand(err.numel()) if lim.numel() == 1 else lim.reshape(-1)
    r = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def _stripe_delta(rec, n):
    slots = kref.STAT_SLOTS
    b = rec.before.reshape(-1)[:slots * n].view(slots, n)
    a = rec.after.reshape(-1)[:slots * n].view(slots, n)
    return a, b, (a - b).sum(0)


def _either(got, e0, e1, what):
    bad = (kref.bits(got) != kref.bits(e0)) & (kref.bits(got) != kref.bits(e1))
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, expected %r (or %r with the multiply-adds fused)"
                             % (what, int(bad.sum()), bad.numel(), i, float(got[i]), float(e0[i]), float(e1[i])))


def check_launch(i, L):
    """one launch against fp64 of its own recorded inputs -> worst observed error / bound over its bounded outputs"""
    if L.op == "wgrad":
        return None
    if L.op not in REFS:
        raise AssertionError("launch %d: no fp64 reference for %s" % (i, L.op))
    a = {k: (v.before if isinstance(v, TRec) else v) for k, v in L.args.items()}
    post = {k: v.after for k, v in L.args.items() if isinstance(v, TRec) and v.after is not None}
    exp = REFS[L.op](a, post)
    worst = 0.0
    for name in OUTS[L.op]:
        rec = L.args.get(name)
        if not isinstance(rec, TRec):
            assert name not in exp, "launch %d %s: output %s expected but not passed" % (i, L.op, name)
            continue
        assert name in exp, "launch %d %s: output %s has no reference" % (i, L.op, name)
        e, what = exp[name], "launch %d %s.%s" % (i, L.op, name)
        got = rec.after
        assert got.dtype == rec.dtype
        if e[0] == "within":
            assert tuple(got.shape) == tuple(e[1].shape), "%s: shape %s, reference %s" % (what, tuple(got.shape), tuple(e[1].shape))
            kref.assert_within(got, e[1], e[2], what)
            worst = max(worst, _ratio((got.double() - e[1]).abs(), e[2]))
        elif e[0] == "bits":
            kref.assert_bits(got.reshape(-1)[:e[1].numel()], e[1].reshape(-1), what=what)
        elif e[0] == "either":
            _either(got.reshape(-1)[:e[1].numel()], e[1].reshape(-1), e[2].reshape(-1), what)
        elif e[0] == "stripes":
            n = e[1].numel()
            af, bf, d = _stripe_delta(rec, n)
            kref.assert_within(d, e[1], e[2], what)
            worst = max(worst, _ratio((d - e[1]).abs(), e[2]))
            if e[3]:
                assert torch.equal(af[e[3]:], bf[e[3]:]), "%s: wrote beyond the %d stripes in use" % (what, e[3])
        elif e[0] == "mask":
            out = L.args["out"].after
            n = out.numel() // e[1]
            assert got.numel() >= n, "%s: %d mask bytes for %d channel units" % (what, got.numel(), n)
            assert torch.equal(got[:n], kref.mask_pack(out.float() > 0, e[1])), "%s: not the bits of the stored output" % what
            assert torch.equal(got[n:], rec.before[n:]), "%s: wrote past the mask" % what
        elif e[0] != "amax":        # (the arg-max bytes: _check_pool below)
            raise AssertionError("%s: unknown expectation %r" % (what, e[0]))
    if L.op == "maxpool_fwd" and "xcopy" in exp:
        _check_pool(i, L, exp, "launch %d maxpool_fwd" % i)
    _check_untouched(i, L)
    return worst


def _check_untouched(i, L):
    """every byte of the storages the launch wrote into, outside its output views, is as it was"""
    groups = {}
    for name in OUTS[L.op]:
        rec = L.args.get(name)
        if isinstance(rec, TRec) and rec.after is not None:
            if rec.base_after is None:          # a big storage: compared on the device when the launch was recorded
                assert rec.outside is not None, "launch %d %s.%s: no record of the bytes around the view" % (i, L.op, name)
                assert rec.outside[0] == 0, "launch %d %s: wrote %d elements outside its output view(s); first at %d" % (
                    i, L.op, rec.outside[0], rec.outside[1])
                continue
            g = groups.setdefault(rec.base, (rec, torch.zeros(rec.base_before.numel(), dtype=torch.bool)))
            g[1].as_strided(rec.shape, rec.stride, rec.off).fill_(True)
    for rec, written in groups.values():
        kref.assert_untouched(rec.base_after, rec.base_before, written, "launch %d %s" % (i, L.op))


def replay(tape):
    """-> {op: (launches, worst observed error / bound)}; raises on the first launch outside its bound"""
    stat = {}
    for i, L in enumerate(tape):
        r = check_launch(i, L)
        n, w = stat.get(L.op, (0, 0.0))
        stat[L.op] = (n + 1, max(w, r or 0.0))
    return stat


def chain(tape, flat):
    """The chain of per-launch fp64 replays, each rounded ONCE to its stored type (kref.round_to): launch k reads what the chain's
    launches before it wrote (and the recorded bytes for everything else), its rounded reference goes into a shadow of the
    storage it writes.  An element is `exact` where its launch's bound is zero both on the chain's operands and on the device's
    own and the two references agree (all of its terms are zero, or it is a copy: channel padding, the zero tiles of the inputs,
    gradients gated off by a mask); other outputs written as bits (finalizes, casts) are exact as the per-launch check left them.
    -> {storage address: (shadow values, exact map)}; weight gradients go into the shadow of `flat`."""
    shadow = {}

    def get(rec, init):
        # (a buffer freed during the stage hands its address to a later one: a storage of another size or type is a new storage)
        if rec.base not in shadow or shadow[rec.base][0].numel() != init.numel() or shadow[rec.base][0].dtype != init.dtype:
            shadow[rec.base] = [init.clone(), torch.zeros(init.numel(), dtype=torch.bool)]
        return shadow[rec.base]
    view = lambda t, r: t.as_strided(r.shape, r.stride, r.off)
    fbase = flat.untyped_storage().data_ptr()
    shadow[fbase] = [torch.zeros(flat.untyped_storage().nbytes() // 4), torch.zeros(flat.untyped_storage().nbytes() // 4, dtype=torch.bool)]
    for L in tape:
        recs = {k: v for k, v in L.args.items() if isinstance(v, TRec)}
        aB = {k: (v.before if isinstance(v, TRec) else v) for k, v in L.args.items()}
        aA = dict(aB)
        for k, r in recs.items():
            if r.base in shadow and r.before.dtype == shadow[r.base][0].dtype and r.off + r.nbytes() // r.before.element_size() <= shadow[r.base][0].numel():
                aA[k] = view(shadow[r.base][0], r).clone()
        if L.op == "wgrad":
            (rA, lA), (rB, lB) = ref_wgrad(aA), ref_wgrad(aB)
            d = L.args["dst"]       # (scattered into the window of its own parameter, not into a vector as long as the buffer)
            o, n = (d.ptr - fbase) // 4, d.before.numel()
            sc = (n, L.args["taps"], L.args["sm"], L.args["sk"], L.args["Cout_valid"], L.args["Cin_valid"], L.args["dst_offset"])
            val, t = kref.wgrad_scatter(rA, *sc)
            ex, _ = kref.wgrad_scatter(((lA == 0) & (lB == 0) & (rA == rB)).double(), *sc)
            shadow[fbase][0][o:o + n][t] = val[t].float()
            shadow[fbase][1][o:o + n][t] = ex[t] > 0
            continue
        post = {k: v.after for k, v in recs.items() if v.after is not None}
        eA, eB = REFS[L.op](aA, post), REFS[L.op](aB, post)
        for name in OUTS[L.op]:
            r = L.args.get(name)
            if not isinstance(r, TRec) or r.after is None:
                continue
            val, ex = get(r, r.init())
            e, f = eA[name], eB[name]
            if e[0] == "within":
                view(val, r).copy_(kref.round_to(e[1], r.dtype) if r.dtype != torch.float64 else e[1])
                view(ex, r).copy_((e[2] == 0) & (f[2] == 0) & (e[1] == f[1]))
            else:
                view(val, r).copy_(r.after)
                view(ex, r).fill_(e[0] == "bits")
    return shadow


def check_chain(tape, flat, finals):
    """the stage's outputs and its gradient buffer, as they stand at the END of the stage, equal the chain wherever it is exact
    -> exact elements compared"""
    shadow = chain(tape, flat)
    n = 0
    for t in list(finals) + [flat]:
        base = t.untyped_storage().data_ptr()
        if base not in shadow:
            continue
        val, ex = shadow[base]
        dev = _storage(t)
        assert dev.dtype == val.dtype and dev.numel() == val.numel(), "the chain's last writer of this storage is not the stage's output"
        bad = (kref.bits(dev) != kref.bits(val)) & ex & ~((dev == 0) & (val == 0))
        assert not bool(bad.any()), "end of stage: %d elements differ from the chain of rounded replays where its bound is zero; first at %d" % (
            int(bad.sum()), int(bad.nonzero()[0]))
        n += int(ex.sum())
    return n


def check_gradients(tape, flat, flat_ptr):
    """the flat gradient buffer after the stage's flush: every weight gradient against the fp64 replay of its launches (scattered
    as ubr_wgrad_reduce does), the BatchNorm gradients as their launches left them, everything else still zero; all finite.
    -> (weight gradients checked, worst error / bound)"""
    flat = flat.detach().cpu()
    n = flat.numel()
    touched, other = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    nw, worst = 0, 0.0
    for i, L in enumerate(tape):
        a = L.args
        if L.op == "wgrad":
            # no two launches write one element (asserted), so each launch is compared on its own, inside the window of the
            # parameter it names: the cost does not grow with the length of the buffer
            dW, lW = ref_wgrad({k: (v.before if isinstance(v, TRec) else v) for k, v in a.items()})
            o, m = (a["dst"].ptr - flat_ptr) // 4, a["dst"].before.numel()
            assert 0 <= o and o + m <= n and 0 <= a["dst_offset"] < m and not a["accumulate"], "launch %d wgrad: destination outside the gradient buffer" % i
            sc = (m, a["taps"], a["sm"], a["sk"], a["Cout_valid"], a["Cin_valid"], a["dst_offset"])
            r, t = kref.wgrad_scatter(dW, *sc)
            l, _ = kref.wgrad_scatter(lW, *sc)
            assert not bool((t & touched[o:o + m]).any()), "launch %d wgrad: two launches write one weight gradient element" % i
            touched[o:o + m] |= t
            kref.assert_within(flat[o:o + m][t], r[t], l[t], "launch %d: weight gradient" % i)
            worst = max(worst, _ratio((flat[o:o + m].double() - r).abs()[t], l[t]))
            nw += 1
        else:
            for name in OUTS[L.op]:
                rec = a.get(name)
                if isinstance(rec, TRec) and rec.dtype == torch.float32 and flat_ptr <= rec.ptr < flat_ptr + 4 * n:
                    o = (rec.ptr - flat_ptr) // 4
                    kref.assert_bits(flat[o:o + rec.after.numel()], rec.after.reshape(-1), what="launch %d %s.%s at the end of the stage" % (i, L.op, name))
                    other[o:o + rec.after.numel()] = True
    assert bool(torch.isfinite(flat).all()), "gradient buffer not finite"
    rest = ~(touched | other)
    assert not bool((kref.bits(flat)[rest] != 0).any()), "gradient buffer written outside the stage's parameters"
    return nw, worst


# ------------------------------------------------------------------------------------------------------------------
# CPU stand-in for the kernels
# ------------------------------------------------------------------------------------------------------------------
def emulate(monkeypatch, eng):
    """patch ubresnet_amd.ops (BEFORE a Tap wraps it) so that every launch writes its fp64 reference rounded once to the stored
    type, and the engine's weight packing so that it runs on the host"""
    def put(t, e, a):
        if e[0] == "within":
            t.copy_(kref.round_to(e[1], t.dtype) if t.dtype != torch.float64 else e[1])
        elif e[0] in ("bits", "either"):
            t.view(-1)[:e[1].numel()].copy_(e[1].reshape(-1))
        elif e[0] == "stripes":
            t.reshape(-1)[:e[1].numel()].add_(e[1])
        elif e[0] == "mask":
            n = a["out"].numel() // e[1]
            t[:n] = kref.mask_pack(a["out"].float() > 0, e[1])
        elif e[0] == "amax":
            t.copy_(e[1].to(torch.uint8))

    def make(name):
        sig = inspect.signature(getattr(OPS, name))

        def fn(*args, **kwargs):
            ba = sig.bind(*args, **kwargs)
            ba.apply_defaults()
            a = {}
            for k, v in ba.arguments.items():
                if isinstance(v, OPS.Affine):
                    a.update({"%s.%s" % (k, f): getattr(v, f) for f in ("sub", "scale", "shift", "lo")})
                elif isinstance(v, dict):
                    a.update({"%s.%s" % (k, f): t for f, t in v.items()})
                elif k in ("xf", "fin2", "fin_b") and v is None:
                    a.update({"%s.%s" % (k, f): None for f in (("sub", "scale", "shift", "lo") if k == "xf" else _FIN)})
                else:
                    a[k] = v
            if name == "wgrad":
                dW, _ = ref_wgrad(a)
                dst = a["dst"].view(-1)
                r, t = kref.wgrad_scatter(dW, dst.numel(), a["taps"], a["sm"], a["sk"], a["Cout_valid"], a["Cin_valid"], a["dst_offset"])
                dst[t] = r[t].float()
                return
            exp = REFS[name](a, None)
            order = sorted(exp, key=lambda k: exp[k][0] == "mask")      # the mask reads the stored output
            for k in order:
                put(a[k], exp[k], a)
        fn = torch.no_grad()(fn)
        fn.__wrapped__ = getattr(OPS, name)        # (inspect.signature reports the operator's own parameters)
        return fn
    for name in list(REFS) + ["wgrad"]:
        monkeypatch.setattr(OPS, name, make(name))

    def fwd_fin(stats, bn, scale, shift, mean, invstd):
        return dict(stats=stats, gamma=bn.weight, beta=bn.bias, rmean=bn.running_mean, rvar=bn.running_var, nbt=bn.num_batches_tracked,
                    scale=scale, shift=shift, mean=mean, invstd=invstd, momentum=bn.momentum, eps=bn.eps)
    monkeypatch.setattr(OPS, "bn_fwd_fin", fwd_fin)
    monkeypatch.setattr(OPS, "zero_", lambda t: t.zero_())
    from ubresnet_amd import _lib
    monkeypatch.setattr(_lib, "require_cuda", lambda t, what: None)      # (Engine._check_input: the whole-network passes)

    def pack_all(dt, device, group, stream=None):
        images = {}
        cpu = kref.CPU[dt]
        for grp, k, w, soff, M, Kv, Kpad, sm, sk, ntaps, tstride in eng._plan_items():
            Kp = Kpad if Kpad is not None else (Kv + cpu - 1) // cpu * cpu
            img = kref.pack_ref(w.detach(), M, (M + 15) // 16 * 16, Kv, Kp, sm, sk, [t * tstride for t in range(ntaps)], dt, src_offset=soff)
            old = eng._images.get(k)         # (an image keeps its address from pass to pass, as the engine's pack plan does)
            images[k] = old.copy_(img) if old is not None and old.shape == img.shape and old.dtype == img.dtype else img
        eng._images = images
    monkeypatch.setattr(eng, "pack_all", pack_all)


# ------------------------------------------------------------------------------------------------------------------
# the expected launch graph
# ------------------------------------------------------------------------------------------------------------------
_ESZ = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2, torch.float64: 8, torch.uint8: 1, torch.int64: 8}


class Sym:
    """a tensor of the expected graph: known from outside (ptr given), or a buffer the stage allocates (bound to the address its
    first launch names), or a view `off` bytes into another symbol"""

    def __init__(self, name, shape, dtype, ptr=None, base=None, off=0, stride=None, min_shape=False):
        self.name, self.shape, self.dtype, self.ptr, self.base, self.off = name, tuple(shape), dtype, ptr, base, off
        self.stride, self.min_shape = (tuple(stride) if stride is not None else None), min_shape

    def addr(self):
        if self.base is not None:
            b = self.base.addr()
            return None if b is None else b + self.off
        return self.ptr

    def bind(self, ptr):
        """-> the symbol that took the address (the root of a chain of views)"""
        if self.base is not None:
            return self.base.bind(ptr - self.off)
        self.ptr = ptr
        return self

    def why_not(self, rec):
        """None when the recorded tensor can be this symbol, else the reason"""
        if not isinstance(rec, TRec):
            return "%s: not a tensor (%r)" % (self.name, rec)
        if rec.dtype != self.dtype:
            return "%s: dtype %s, expected %s" % (self.name, rec.dtype, self.dtype)
        if self.min_shape:
            if len(rec.shape) != 1 or rec.shape[0] < self.shape[0]:
                return "%s: %s elements, at least %d expected" % (self.name, rec.shape, self.shape[0])
        elif rec.shape != self.shape:
            return "%s: shape %s, expected %s" % (self.name, rec.shape, self.shape)
        if self.stride is not None and rec.stride != self.stride:
            return "%s: strides %s, expected %s" % (self.name, rec.stride, self.stride)
        p = self.addr()
        if p is not None and p != rec.ptr:
            return "%s: address %#x, expected %#x" % (self.name, rec.ptr, p)
        return None


class Graph:
    def __init__(self):
        self.nodes = []

    def ext(self, name, t, min_shape=False):
        """a tensor known from outside the stage: a torch tensor or a TRec"""
        return Sym(name, t.shape, t.dtype, ptr=t.data_ptr() if isinstance(t, torch.Tensor) else t.ptr,
                   stride=t.stride() if isinstance(t, torch.Tensor) else t.stride, min_shape=min_shape)

    def new(self, name, shape, dtype):
        return Sym(name, shape, dtype)

    def view(self, name, base, off_elems, shape, stride=None):
        return Sym(name, shape, base.dtype, base=base, off=off_elems * _ESZ[base.dtype], stride=stride)

    def node(self, op, writes=(), **args):
        self.nodes.append((op, args, tuple(writes)))

    def match(self, tape):
        """bind every expected launch to exactly one recorded launch (any order that respects the edges), every recorded launch to
        one expected launch; then: a buffer is written before it is read, and a reader sees the bytes its last writer left"""
        for sym in getattr(self, "_bound", ()):        # (a graph matched before: what that match bound is free again)
            sym.ptr = None
        self._bound = []
        free = list(range(len(tape)))
        at = []
        for op, args, writes in self.nodes:
            why, hit = [], None
            for i in free:
                L = tape[i]
                if L.op != op:
                    continue
                r = self._fits(L, args)
                if r is None:
                    hit = i
                    break
                why.append("launch %d: %s" % (i, r))
            if hit is None:
                raise AssertionError("no recorded %s launch is the expected %s(%s)\n  %s" % (
                    op, op, ", ".join("%s=%s" % (k, v.name if isinstance(v, Sym) else v) for k, v in args.items() if k != "taps"),
                    "\n  ".join(why) if why else "(none of that op left)"))
            for k, v in args.items():
                if isinstance(v, Sym) and v.addr() is None:
                    self._bound.append(v.bind(tape[hit].args[k].ptr))
            free.remove(hit)
            at.append(hit)
        assert not free, "recorded launches the module's dataflow does not ask for: %s" % [tape[i] for i in free]
        # edges: per address range, the last writer before each reader
        by_name, by_view, by_index = {}, {}, {}     # (tape index, lo, hi, TRec, name) by the symbol's name and by (address, shape, strides)
        for (op, args, writes), i in zip(self.nodes, at):
            for k in writes:
                rec = tape[i].args.get(k)
                if isinstance(rec, TRec):
                    w = (i, rec.ptr, rec.ptr + rec.nbytes(), rec, args[k].name if isinstance(args.get(k), Sym) else k)
                    by_name.setdefault(w[4], []).append(w)
                    by_view.setdefault((rec.ptr, rec.shape, rec.stride), []).append(w)
                    by_index.setdefault(i, []).append(w)
        for (op, args, writes), i in zip(self.nodes, at):
            for k, v in args.items():
                rec = tape[i].args.get(k)
                if not isinstance(v, Sym) or not isinstance(rec, TRec) or k in writes:
                    continue
                named = [w[0] for w in by_name.get(v.name, ()) if w[0] != i]      # (an in-place addend is read and written by one launch)
                if named:
                    assert min(named) < i, "%s launch %d reads %s before launch %d writes it" % (op, i, v.name, min(named))
                last = [w for w in by_view.get((rec.ptr, rec.shape, rec.stride), ()) if w[0] < i]
                if last:
                    w = max(last, key=lambda w: w[0])
                    assert w[4] == v.name, "%s launch %d reads %s, but launch %d last wrote %s there" % (op, i, v.name, w[0], w[4])
                    if w[3].after is not None:
                        exp = self._overlaid(w, i, by_index)
                        if exp is not None:
                            kref.assert_bits(rec.before, exp, what="%s launch %d reads %s: not the bytes launch %d wrote" % (op, i, v.name, w[0]))
        return at

    @staticmethod
    def _overlaid(w, i, by_index):
        """what the writer `w` left, with the writes of launches between it and the reader `i` INTO PARTS of the same memory laid
        over it (a stride-2 bypass's 1x1 data gradient adds onto one phase of g_x in place; the next block then reads all of g_x).
        None where such a part cannot be placed (the writer's view is not contiguous): that edge's bytes are then held by the
        per-launch replays on both sides alone"""
        exp = None
        for j in range(w[0] + 1, i):
            for w2 in by_index.get(j, ()):
                if w2[1] < w[2] and w2[2] > w[1] and w2[3].dtype == w[3].dtype:
                    r, r2 = w[3], w2[3]
                    esz = r.before.element_size()
                    if not r.after.is_contiguous() or tuple(r.after.stride()) != r.stride or w2[1] < w[1] or w2[2] > w[2]:
                        return None
                    exp = r.after.clone() if exp is None else exp
                    exp.view(-1).as_strided(r2.shape, r2.stride, (r2.ptr - r.ptr) // esz).copy_(r2.after)
        return w[3].after if exp is None else exp

    @staticmethod
    def _fits(L, args):
        for k, v in args.items():
            got = L.args.get(k)
            if isinstance(v, Sym):
                r = v.why_not(got)
                if r is not None:
                    return "%s = %s" % (k, r)
            elif v is None:
                if got is not None:
                    return "%s given, none expected" % k
            elif isinstance(v, (list, tuple)):
                if _deep(got) != _deep(v):
                    return "%s differs" % k
            elif got != v or isinstance(got, TRec):
                return "%s = %r, expected %r" % (k, got, v)
        return None


def _site_syms(g, eng, bn, tag):
    s = eng.bn(bn)
    return {n: g.ext("%s.%s" % (tag, n), getattr(s, n)) for n in ("scale", "shift", "mean", "invstd")}, s


def _aff(d, prefix, syms):
    """an on-load affine as four arguments; syms = (sub, scale, shift, lo) or None"""
    for f, s in zip(("sub", "scale", "shift", "lo"), syms if syms is not None else (None,) * 4):
        d["%s.%s" % (prefix, f)] = s


def _relu_aff(g, eng, site, tag, dev):
    v, s = site
    return (v["mean"], v["scale"], v["shift"], g.ext(tag + ".zero", eng.const(dev, 0.0, s.C), min_shape=False))


def _finish(g, eng, bn, v, s, cnt, training, stats):
    """BatchNorm finalize of a site after its conv, as Engine._finish_bn: batch statistics in training, running ones otherwise"""
    m = bn
    if training and not s.frozen:
        g.node("bn_finalize", writes=("scale", "shift", "mean", "invstd"), stats=stats, count=cnt, gamma=g.ext("gamma", m.weight),
               beta=g.ext("beta", m.bias), rmean=g.ext("rmean", m.running_mean), rvar=g.ext("rvar", m.running_var),
               scale=v["scale"], shift=v["shift"], mean=v["mean"], invstd=v["invstd"])
    else:
        g.node("bn_eval_affine", writes=("scale", "shift", "mean", "invstd"), gamma=g.ext("gamma", m.weight), beta=g.ext("beta", m.bias),
               rmean=g.ext("rmean", m.running_mean), rvar=g.ext("rvar", m.running_var),
               scale=v["scale"], shift=v["shift"], mean=v["mean"], invstd=v["invstd"])


class BlockSyms:
    pass


def expect_block_fwd(g, eng, blk, tag, x, out, dt, training, fused, xf_in=None, save=True):
    """BasicBlock.forward: conv1 -> bn1 -> relu -> conv2 -> bn2 (+ bypass -> bnpass on x) -> relu(relu(bn2) + shortcut).
    x, out: Syms; xf_in: four Syms or None.  fused: the tail makes bn2's (and bnpass's) vectors itself from RED_SLOTS stripes."""
    N, H, W, Cin = x.shape
    _, OH, OW, Cout = out.shape
    S, cnt, dev = blk.stride, N * OH * OW, blk.conv1.weight.device
    b = BlockSyms()
    b.blk, b.tag, b.x, b.out, b.xf_in, b.dt = blk, tag, x, out, xf_in, dt
    b.bn1, b.bn2 = _site_syms(g, eng, blk.bn1, tag + ".bn1"), _site_syms(g, eng, blk.bn2, tag + ".bn2")
    b.bnb = _site_syms(g, eng, blk.bnpass, tag + ".bnpass") if blk.bypass is not None else None
    st = lambda site: g.ext("%s.stats%d" % (tag, 1 if site is b.bn1 else 2 if site is b.bn2 else 3), site[1].stats) if site[1].stats is not None else None
    b.c1 = g.new(tag + ".c1", (N, OH, OW, Cout), dt)
    b.c2 = g.new(tag + ".c2", (N, OH, OW, Cout), dt)
    b.cb = g.new(tag + ".cb", (N, OH, OW, Cout), dt) if blk.bypass is not None else None
    slots = kref.RED_SLOTS if fused else 0
    a = dict(x=x, wp=g.ext(tag + ".W1", eng.packed(blk.conv1.weight, "fwd")), y=b.c1, taps=OPS.conv_taps(3, 1, 1), Cout=Cout, S=S,
             stats=st(b.bn1), stats_slots=0, addend=None, bias=None)
    _aff(a, "xf", xf_in)
    g.node("conv", writes=("y", "stats"), **a)
    _finish(g, eng, blk.bn1, b.bn1[0], b.bn1[1], cnt, training, st(b.bn1))
    a = dict(x=b.c1, wp=g.ext(tag + ".W2", eng.packed(blk.conv2.weight, "fwd")), y=b.c2, taps=OPS.conv_taps(3, 1, 1), Cout=Cout, S=1,
             stats=st(b.bn2), stats_slots=slots, addend=None, bias=None)
    _aff(a, "xf", _relu_aff(g, eng, b.bn1, tag + ".bn1", dev))
    g.node("conv", writes=("y", "stats"), **a)
    if not fused:
        _finish(g, eng, blk.bn2, b.bn2[0], b.bn2[1], cnt, training, st(b.bn2))
    if blk.bypass is not None:
        a = dict(x=x, wp=g.ext(tag + ".Wb", eng.packed(blk.bypass.weight, "fwd")), y=b.cb, taps=OPS.conv_taps(1, 1, 0), Cout=Cout, S=S,
                 stats=st(b.bnb), stats_slots=slots, addend=None, bias=None)
        _aff(a, "xf", xf_in)
        g.node("conv", writes=("y", "stats"), **a)
        if not fused:
            _finish(g, eng, blk.bnpass, b.bnb[0], b.bnb[1], cnt, training, st(b.bnb))
    # the final ReLU's mask: one byte per 16-byte channel unit of the stored type
    b.mask = g.new(tag + ".mask", (cnt * (Cout // kref.CPU[dt]),), torch.uint8) if save else None
    sc = b.cb if blk.bypass is not None else x
    if fused:
        a = {"c2": b.c2, "sc": sc, "count": cnt, "out": out, "relu_mask": b.mask}
        for f, site, bn in (("fin2", b.bn2, blk.bn2), ("fin_b", b.bnb, blk.bnpass)):
            if site is None:
                a[f + ".stats"] = None
                continue
            a[f + ".stats"], a[f + ".gamma"], a[f + ".beta"] = st(site), g.ext("gamma", bn.weight), g.ext("beta", bn.bias)
            a[f + ".rmean"], a[f + ".rvar"] = g.ext("rmean", bn.running_mean), g.ext("rvar", bn.running_var)
            for n in ("scale", "shift", "mean", "invstd"):
                a["%s.%s" % (f, n)] = site[0][n]
        g.node("block_tail_fwd_fin", writes=("out", "relu_mask", "fin2.scale", "fin2.shift", "fin2.mean", "fin2.invstd",
                                              "fin_b.scale", "fin_b.shift", "fin_b.mean", "fin_b.invstd"), **a)
    else:
        v2, vb = b.bn2[0], b.bnb[0] if b.bnb is not None else None
        g.node("block_tail_fwd", writes=("out", "relu_mask"), c2=b.c2, mean2=v2["mean"], scale2=v2["scale"], shift2=v2["shift"], sc=sc,
               mean_b=vb["mean"] if vb else None, scale_b=vb["scale"] if vb else None, shift_b=vb["shift"] if vb else None,
               out=out, relu_mask=b.mask)
    return b


def _dgrad(g, eng, conv_mod, tag, gsym, gx, S, k, addend=None, addend_mask=None):
    """data gradient of Conv2d(k, stride S, pad k // 2): stride 1 one launch; stride 2 the four output phases"""
    wp = g.ext(tag, eng.packed(conv_mod.weight, "dgrad"))
    Cin = gx.shape[3]
    if S == 1:
        a = dict(x=gsym, wp=wp, y=gx, taps=OPS.conv_dgrad_taps_s1(k, 1, k // 2), Cout=Cin, S=1, addend=addend, addend_mask=addend_mask,
                 stats=None, bias=None)
        _aff(a, "xf", None)
        g.node("conv", writes=("y",), **a)
        return
    N, H, W, _ = gx.shape
    full = (H * W * Cin, W * Cin, Cin, 1)
    ph = [(ry, rx, OPS.transposed_phase_taps(k, 1, k // 2, 2, ry, rx)) for ry in range(2) for rx in range(2)]
    ph = [p for p in ph if p[2]]
    if k == 3 and addend_mask is None:
        a = dict(x=gsym, wp=wp, y_full=gx, taps=[t for p in ph for t in p[2]], phases=ph, Cout=Cin, addend_full=addend, bias=None)
        _aff(a, "xf", None)
        g.node("conv_phases", writes=("y_full",), **a)
        return
    for ry, rx, taps in ph:
        pv = lambda s, nm: g.view("%s[%d%d]" % (nm, ry, rx), s, ry * full[1] + rx * full[2], (N, H // 2, W // 2, Cin),
                                  (full[0], 2 * full[1], 2 * full[2], 1))
        a = dict(x=gsym, wp=wp, y=pv(gx, gx.name), taps=taps, Cout=Cin, S=1, addend=pv(addend, addend.name) if addend is not None else None,
                 addend_mask=None, stats=None, bias=None)
        _aff(a, "xf", None)
        g.node("conv", writes=("y",), **a)


def _bn_bwd_site(g, eng, site, bn, tag, ga, c, G, cnt, dt, fin_max):
    """a = relu(bn(c)) backward at a training site: reduce, then the apply pass (finalize fused up to fin_max channels)"""
    v, s = site
    C = s.C
    red = g.new(tag + ".red", (kref.STAT_SLOTS * 2 * C,), torch.float64)
    gc = g.new(tag + ".g_c", c.shape, dt)
    com = dict(ga=ga, ga2=None, c=c, scale=v["scale"], shift=v["shift"], mean=v["mean"], invstd=v["invstd"], relu=True)
    if s.frozen:      # running statistics are constants of the pass: one walk, dgamma / dbeta from its sums afterwards
        g.node("bn_bwd_frozen", writes=("gc", "red"), red=red, gc=gc, **com)
        g.node("bn_bwd_finalize_frozen", writes=("dgamma", "dbeta"), red=red, Cn=C, dgamma=g.ext(tag + ".dgamma", G(bn.weight)),
               dbeta=g.ext(tag + ".dbeta", G(bn.bias)), k1=None, k2=None)
        return gc
    g.node("bn_bwd_reduce", writes=("red",), red=red, **com)
    if C <= fin_max:
        g.node("bn_bwd_apply_fin", writes=("gc", "dgamma", "dbeta"), red=red, count=cnt, dgamma=g.ext(tag + ".dgamma", G(bn.weight)),
               dbeta=g.ext(tag + ".dbeta", G(bn.bias)), gc=gc, **com)
    else:
        k = g.new(tag + ".k", (2 * C,), torch.float32)
        k1, k2 = g.view(tag + ".k1", k, 0, (C,)), g.view(tag + ".k2", k, C, (C,))
        g.node("bn_bwd_finalize", writes=("dgamma", "dbeta", "k1", "k2"), red=red, count=cnt, Cn=C, dgamma=g.ext(tag + ".dgamma", G(bn.weight)),
               dbeta=g.ext(tag + ".dbeta", G(bn.bias)), accumulate=False, k1=k1, k2=k2)
        g.node("bn_bwd_apply", writes=("gc",), k1=k1, k2=k2, gc=gc, **com)
    return gc


def _wgrad(g, tag, x, gsym, taps, dst, sm, sk, Cout, Cin, S, xf, dst_offset=0, exclusive=False):
    a = dict(x=x, g=gsym, taps=taps, dst=dst, sm=sm, sk=sk, Cout_valid=Cout, Cin_valid=Cin, S=S, accumulate=False, dst_offset=dst_offset,
             exclusive=exclusive)
    _aff(a, "xf", xf)
    g.node("wgrad", **a)


def expect_block_bwd(g, eng, b, go, go2, G, need_gx=True, fin_max=None):
    """backward of the block whose forward symbols are `b` (training sites).  The saved tensors ARE the forward's symbols.
    -> the Sym of g_x (None when not needed)"""
    from ubresnet_amd import engine as E
    fin_max = E._FIN_MAX_C if fin_max is None else fin_max
    blk, tag, dt, x, out = b.blk, b.tag, b.dt, b.x, b.out
    N, OH, OW, Cout = b.c2.shape
    Cin, S, cnt, NS = x.shape[3], blk.stride, N * OH * OW, kref.STAT_SLOTS
    byp = b.cb is not None
    dev = blk.conv1.weight.device
    v2, vb = b.bn2[0], b.bnb[0] if byp else None
    # one reduction buffer per tail: bn2's stripes first, bnpass's behind them
    red = g.new(tag + ".red", (NS * (4 if byp else 2) * Cout,), torch.float64)
    red2 = g.view(tag + ".red2", red, 0, (NS * 2 * Cout,))
    redb = g.view(tag + ".redb", red, NS * 2 * Cout, (NS * 2 * Cout,)) if byp else None
    # sites that normalise with running statistics need no sum between go and the data gradients: all of the tail's sites
    # frozen -> one pass; one of two -> the two passes, the frozen site's k1 = k2 = 0
    fz2, fzb = b.bn2[1].frozen, byp and b.bnb[1].frozen
    onepass = fz2 and (fzb or not byp)
    if not onepass:
        g.node("block_tail_bwd_reduce", writes=("red2", "red_b"), go=go, go2=go2, out=out, c2=b.c2, scale2=v2["scale"], shift2=v2["shift"],
               mean2=v2["mean"], invstd2=v2["invstd"], cb=b.cb, mean_b=vb["mean"] if byp else None, invstd_b=vb["invstd"] if byp else None,
               red2=red2, red_b=redb, relu_mask=b.mask)
    fin = Cout <= fin_max and not fz2 and not fzb
    lazy = not byp and go2 is None and need_gx and (fin or onepass)
    g_c2 = g.new(tag + ".g_c2", b.c2.shape, dt)
    g_sc = None if lazy else g.new(tag + ".g_sc", b.c2.shape, dt)
    Gs = lambda p, n: g.ext("%s.d%s" % (tag, n), G(p))
    com = dict(go=go, go2=go2, c2=b.c2, scale2=v2["scale"], shift2=v2["shift"], mean2=v2["mean"], invstd2=v2["invstd"], cb=b.cb,
               scale_b=vb["scale"] if byp else None, mean_b=vb["mean"] if byp else None, invstd_b=vb["invstd"] if byp else None,
               g_c2=g_c2, g_sc=g_sc, relu_mask=b.mask)
    if onepass:
        g.node("block_tail_bwd_frozen", writes=("g_c2", "g_sc", "red2", "red_b"), red2=red2, red_b=redb, **com)
        for rd, bn, n in ((red2, blk.bn2, "2"),) + (((redb, blk.bnpass, "_b"),) if byp else ()):
            g.node("bn_bwd_finalize_frozen", writes=("dgamma", "dbeta"), red=rd, Cn=Cout, dgamma=Gs(bn.weight, "gamma" + n),
                   dbeta=Gs(bn.bias, "beta" + n), k1=None, k2=None)
    elif fin:
        g.node("block_tail_bwd_apply_fin", writes=("g_c2", "g_sc", "dgamma2", "dbeta2", "dgamma_b", "dbeta_b"), red2=red2, red_b=redb, count=cnt,
               dgamma2=Gs(blk.bn2.weight, "gamma2"), dbeta2=Gs(blk.bn2.bias, "beta2"),
               dgamma_b=Gs(blk.bnpass.weight, "gamma_b") if byp else None, dbeta_b=Gs(blk.bnpass.bias, "beta_b") if byp else None, **com)
    else:
        k = g.new(tag + ".k", (4 * Cout,), torch.float32)
        kv = [g.view("%s.k%d" % (tag, i), k, i * Cout, (Cout,)) for i in range(4)]
        for fz, rd, bn, n, k1, k2 in ((fz2, red2, blk.bn2, "2", kv[0], kv[1]),) + (((fzb, redb, blk.bnpass, "_b", kv[2], kv[3]),) if byp else ()):
            if fz:
                g.node("bn_bwd_finalize_frozen", writes=("dgamma", "dbeta", "k1", "k2"), red=rd, Cn=Cout, dgamma=Gs(bn.weight, "gamma" + n),
                       dbeta=Gs(bn.bias, "beta" + n), k1=k1, k2=k2)
            else:
                g.node("bn_bwd_finalize", writes=("dgamma", "dbeta", "k1", "k2"), red=rd, count=cnt, Cn=Cout, dgamma=Gs(bn.weight, "gamma" + n),
                       dbeta=Gs(bn.bias, "beta" + n), accumulate=False, k1=k1, k2=k2)
        g.node("block_tail_bwd_apply", writes=("g_c2", "g_sc"), out=out, k1_2=kv[0], k2_2=kv[1], k1_b=kv[2] if byp else None,
               k2_b=kv[3] if byp else None, **com)
    # conv2: its input is relu(bn1(c1)), re-formed on load from bn1's vectors
    _wgrad(g, tag, b.c1, g_c2, OPS.conv_taps(3, 1, 1), Gs(blk.conv2.weight, "W2"), Cout * 9, 9, Cout, Cout, 1, _relu_aff(g, eng, b.bn1, tag + ".bn1", dev))
    g_a1 = g.new(tag + ".g_a1", b.c1.shape, dt)
    _dgrad(g, eng, blk.conv2, tag + ".W2t", g_c2, g_a1, 1, 3)
    g_c1 = _bn_bwd_site(g, eng, b.bn1, blk.bn1, tag + ".bn1", g_a1, b.c1, G, cnt, dt, fin_max)
    # conv1 and the bypass read the block input through ITS affine (a virtual input), the one the forward was given
    _wgrad(g, tag, x, g_c1, OPS.conv_taps(3, 1, 1), Gs(blk.conv1.weight, "W1"), Cin * 9, 9, Cout, Cin, S, b.xf_in)
    if byp:
        _wgrad(g, tag, x, g_sc, OPS.conv_taps(1, 1, 0), Gs(blk.bypass.weight, "Wb"), Cin, 1, Cout, Cin, S, b.xf_in)
    if not need_gx:
        return None
    gx = g.new(tag + ".g_x", x.shape, dt)
    if byp:
        _dgrad(g, eng, blk.conv1, tag + ".W1t", g_c1, gx, S, 3)
        _dgrad(g, eng, blk.bypass, tag + ".Wbt", g_sc, gx, S, 1, addend=gx)
    elif lazy:
        _dgrad(g, eng, blk.conv1, tag + ".W1t", g_c1, gx, S, 3, addend=go, addend_mask=b.mask)
    else:
        _dgrad(g, eng, blk.conv1, tag + ".W1t", g_c1, gx, S, 3, addend=g_sc)
    return gx


def expect_double_fwd(g, eng, dbl, tag, x, out, dt, training, fused, xf_in=None):
    """DoubleResNet.forward: res2(res1(x)); `mid` is res1's output and res2's input"""
    mid = g.new(tag + ".mid", out.shape, dt)
    return (expect_block_fwd(g, eng, dbl.res1, tag + ".res1", x, mid, dt, training, fused, xf_in),
            expect_block_fwd(g, eng, dbl.res2, tag + ".res2", mid, out, dt, training, fused))


def expect_double_bwd(g, eng, bs, go, go2, G, need_gx=True, fin_max=None):
    g_mid = expect_block_bwd(g, eng, bs[1], go, go2, G, True, fin_max)
    return expect_block_bwd(g, eng, bs[0], g_mid, None, G, need_gx, fin_max)


_DECONV_PHASES = [(ry, rx, OPS.transposed_phase_taps(4, 1, 1, 2, ry, rx)) for ry in range(2) for rx in range(2)]


def expect_declayer_fwd(g, eng, dl, tag, x, cat, Cd, out, dt, training, fused, xf_x=None, xf_cat=None):
    """ConvTransposeLayer.forward: deconv(x) into channels [0, Cd) of the concat buffer (the skip half is there already), then res.
    xf_x / xf_cat: the affines (four Syms each) of a virtual deconv input / of virtual concat channels (ASPP_ResNet's dec_layer5 / 4)"""
    N, H2, W2, Cc = cat.shape
    up = g.view(tag + ".up", cat, 0, (N, H2, W2, Cd), (H2 * W2 * Cc, W2 * Cc, Cc, 1))
    a = dict(x=x, wp=g.ext(tag + ".Wd", eng.packed(dl.deconv.weight, "tfwd")), y_full=up, taps=[t for p in _DECONV_PHASES for t in p[2]],
             phases=_DECONV_PHASES, Cout=Cd, addend_full=None, bias=None)
    _aff(a, "xf", xf_x)
    g.node("conv_phases", writes=("y_full",), **a)
    return expect_double_fwd(g, eng, dl.res, tag + ".res", cat, out, dt, training, fused, xf_cat), x, cat, Cd, xf_x


def expect_declayer_bwd(g, eng, dl, tag, fw, go, G, dt):
    """-> (g_x, g_cat): four phase weight gradients of the transposed conv into ONE dW; its data gradient is the stride-2 conv of g_up"""
    bs, x, cat, Cd, xf_x = fw
    g_cat = expect_double_bwd(g, eng, bs, go, None, G)
    N, H2, W2, Cc = cat.shape
    Cin = x.shape[3]
    dW = g.ext(tag + ".dWd", G(dl.deconv.weight))
    full = (H2 * W2 * Cc, W2 * Cc, Cc, 1)
    for ry, rx, taps in _DECONV_PHASES:
        gv = g.view("%s.g_up[%d%d]" % (tag, ry, rx), g_cat, ry * full[1] + rx * full[2], (N, H2 // 2, W2 // 2, Cd), (full[0], 2 * full[1], 2 * full[2], 1))
        _wgrad(g, tag, x, gv, taps, dW, 16, Cd * 16, Cd, Cin, 1, xf_x)
    gx = g.new(tag + ".g_x", x.shape, dt)
    a = dict(x=g.view(tag + ".g_up", g_cat, 0, (N, H2, W2, Cd), full), wp=g.ext(tag + ".Wdt", eng.packed(dl.deconv.weight, "tdgrad")), y=gx,
             taps=OPS.conv_taps(4, 1, 1), Cout=Cin, S=2, addend=None, addend_mask=None, stats=None, bias=None)
    _aff(a, "xf", None)
    g.node("conv", writes=("y",), **a)
    return gx, g_cat


def expect_aspp_fwd(g, eng, layer, post, tag, e, cpost, arena, off_acat, off_post, dt, training):
    """ASPP.forward + ASPP_post.forward: four conv branches (1x1, 3x3 d1 / d3 / d5) with BatchNorm + ReLU and MaxPool2d(3, 1, 1), all
    of e, concatenated [B1 | B2 | B3 | B4 | pool]; then the 1x1 conv over the concat.  The concat is virtual: the branches' raw conv
    outputs and the pooled input share one buffer, and the 1x1 reads it through ONE affine whose channels [16 b, 16 b + 16) are
    branch b's BatchNorm + ReLU and whose pooled channels are the identity -- so site b's vectors ARE that slice of the affine."""
    N, h, w, Cn = e.shape
    Ca, cnt = 64 + Cn, N * h * w
    T = arena.shape[1]
    rows = [g.ext("%s.arena%d" % (tag, r), arena[r]) for r in range(4)]
    row = lambda r, off, n, nm: g.view("%s.%s" % (tag, nm), rows[r], off, (n,))
    a = BlockSyms()
    a.e, a.cpost, a.dt, a.layer, a.post, a.tag = e, cpost, dt, layer, post, tag
    a.acat = g.new(tag + ".acat", (N, h, w, Ca), dt)
    full = (h * w * Ca, w * Ca, Ca, 1)
    a.sl = lambda base, c0, n, nm: g.view("%s.%s" % (tag, nm), base, c0, (N, h, w, n), full)
    a.sites = []
    for b, (conv, bn, k, dil) in enumerate(layer.branches()):
        s = eng.bn(bn)
        o = off_acat + 16 * b
        v = dict(mean=row(0, o, 16, "B%d.mean" % b), scale=row(1, o, 16, "B%d.scale" % b), shift=row(2, o, 16, "B%d.shift" % b),
                 invstd=g.ext("%s.B%d.invstd" % (tag, b), s.invstd))
        a.sites.append((v, s))
        st = g.ext("%s.B%d.stats" % (tag, b), s.stats)
        c = dict(x=e, wp=g.ext("%s.WB%d" % (tag, b), eng.packed(conv.weight, "fwd")), y=a.sl(a.acat, 16 * b, 16, "acat.B%d" % b),
                 taps=OPS.conv_taps(k, dil, dil * (k // 2)), Cout=16, S=1, bias=g.ext("%s.bB%d" % (tag, b), conv.bias), stats=st, stats_slots=0, addend=None)
        _aff(c, "xf", None)
        g.node("conv", writes=("y", "stats"), **c)
        _finish(g, eng, bn, v, s, cnt, training, st)
    p = dict(x=e, pooled=a.sl(a.acat, 64, Cn, "acat.pool"), xcopy=None, stride=1, argmax=None)
    _aff(p, "xf", None)
    g.node("maxpool_fwd", writes=("pooled",), **p)
    a.xf = tuple(row(r, off_acat, Ca, "xf%d" % r) for r in range(4))
    s = eng.bn(post.ASPP_bn)
    a.psite = (dict(mean=row(0, off_post, Cn, "post.mean"), scale=row(1, off_post, Cn, "post.scale"), shift=row(2, off_post, Cn, "post.shift"),
                    invstd=g.ext(tag + ".post.invstd", s.invstd)), s)
    st = g.ext(tag + ".post.stats", s.stats)
    c = dict(x=a.acat, wp=g.ext(tag + ".Wp", eng.packed(post.ASPP_conv.weight, "fwd")), y=cpost, taps=OPS.conv_taps(1, 1, 0), Cout=Cn, S=1,
             bias=g.ext(tag + ".bp", post.ASPP_conv.bias), stats=st, stats_slots=0, addend=None)
    _aff(c, "xf", a.xf)
    g.node("conv", writes=("y", "stats"), **c)
    _finish(g, eng, post.ASPP_bn, a.psite[0], s, cnt, training, st)
    return a


def _bias_grad(g, tag, gsym, C, dst):
    """a conv bias gradient: the per-channel sum of the output gradient, striped in fp64, then cast"""
    red = g.new(tag + ".bred", (kref.STAT_SLOTS * C,), torch.float64)
    g.node("channel_sum", writes=("red",), g=gsym, red=red)
    g.node("cast_f64_to_f32", writes=("dst",), src=red, dst=dst, n=C, scale=1.0, accumulate=False, stride=None, slots=kref.STAT_SLOTS)


def expect_aspp_bwd(g, eng, a, g_post, g_base, G, fin_max=None):
    """-> g_e: the skip's share (g_base) + the pool's + the four branches', accumulated in place"""
    from ubresnet_amd import engine as E
    fin_max = E._FIN_MAX_C if fin_max is None else fin_max
    layer, post, tag, dt, e = a.layer, a.post, a.tag, a.dt, a.e
    N, h, w, Cn = e.shape
    Ca, cnt = 64 + Cn, N * h * w
    g_cpost = _bn_bwd_site(g, eng, a.psite, post.ASPP_bn, tag + ".post", g_post, a.cpost, G, cnt, dt, fin_max)
    _wgrad(g, tag, a.acat, g_cpost, OPS.conv_taps(1, 1, 0), g.ext(tag + ".dWp", G(post.ASPP_conv.weight)), Ca, 1, Cn, Ca, 1, a.xf)
    _bias_grad(g, tag + ".post", g_cpost, Cn, g.ext(tag + ".dbp", G(post.ASPP_conv.bias)))
    g_acat = g.new(tag + ".g_acat", a.acat.shape, dt)
    _dgrad(g, eng, post.ASPP_conv, tag + ".Wpt", g_cpost, g_acat, 1, 1)
    g_e = g.new(tag + ".g_e", e.shape, dt)
    p = dict(x=e, g_pooled=a.sl(g_acat, 64, Cn, "g_acat.pool"), g_extra=g_base, gx=g_e, stride=1, argmax=None)
    _aff(p, "xf", None)
    g.node("maxpool_bwd", writes=("gx",), **p)
    for b, (conv, bn, k, dil) in enumerate(layer.branches()):
        bt = "%s.B%d" % (tag, b)
        g_cb = _bn_bwd_site(g, eng, a.sites[b], bn, bt, a.sl(g_acat, 16 * b, 16, "g_acat.B%d" % b), a.sl(a.acat, 16 * b, 16, "acat.B%d" % b),
                            G, cnt, dt, fin_max)
        _wgrad(g, bt, e, g_cb, OPS.conv_taps(k, dil, dil * (k // 2)), g.ext(bt + ".dW", G(conv.weight)), Cn * k * k, k * k, 16, Cn, 1, None)
        _bias_grad(g, bt, g_cb, 16, g.ext(bt + ".db", G(conv.bias)))
        c = dict(x=g_cb, wp=g.ext(bt + ".Wt", eng.packed(conv.weight, "dgrad")), y=g_e, taps=OPS.conv_dgrad_taps_s1(k, dil, dil * (k // 2)), Cout=Cn, S=1,
                 addend=g_e, addend_mask=None, stats=None, bias=None)
        _aff(c, "xf", None)
        g.node("conv", writes=("y",), **c)
    return g_e


class _Level(torch.nn.Module):
    def __init__(self, Cn):
        super().__init__()
        from ubresnet_amd.models.ASPP_ResNet import ASPP, ASPP_post
        self.layer, self.post = ASPP(Cn), ASPP_post(64 + Cn, Cn)

    def _grad_completion_order(self, prefix):
        return self.post._grad_completion_order(prefix + "post.") + self.layer._grad_completion_order(prefix + "layer.")


def aspp_case(monkeypatch, dt, device, Cn, hw, emu=False):
    """one ASPP level as aspp_forward / aspp_backward run it: the arena [acat affine | post site], sites bound into it"""
    from ubresnet_amd.engine import Saved
    h, w = hw
    lvl = _Level(Cn)
    with torch.no_grad():
        for m in lvl.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.bias.copy_(torch.rand(m.bias.shape, generator=torch.Generator().manual_seed(3)) * 0.4 - 0.2)
    e = noise((2, h, w, Cn), dt, 41, device)
    cpost = torch.empty((2, h, w, Cn), dtype=dt, device=device)
    g_post, g_base = noise((2, h, w, Cn), dt, 42, device), noise((2, h, w, Cn), dt, 43, device)
    st = {}

    def build(eng, G):
        arena, offs = eng._affine_arena(Saved(), torch.device(device), [64 + Cn, Cn], [(0, 64), (64 + Cn, 64 + 2 * Cn)])
        for b, (_, bn, _, _) in enumerate(lvl.layer.branches()):
            eng._bind_site(eng.bn(bn), arena, offs[0] + 16 * b)
        eng._bind_site(eng.bn(lvl.post.ASPP_bn), arena, offs[1])
        st["arena"] = arena
        fwd = lambda: eng.aspp_level_fwd(lvl.layer, lvl.post, e, cpost, arena, offs[0], True, dt)
        bwd = lambda rec: eng.aspp_level_bwd(rec, g_post, g_base, G)

        def expect(g):
            a = expect_aspp_fwd(g, eng, lvl.layer, lvl.post, "aspp", g.ext("e", e), g.ext("cpost", cpost), arena, offs[0], offs[1], dt, True)
            expect_aspp_bwd(g, eng, a, g.ext("g_post", g_post), g.ext("g_base", g_base), G)
        return fwd, bwd, expect
    r = run_stage(monkeypatch, lvl, dt, device, True, build, emu)
    # the pooled channels of the virtual concat pass through the affine untouched, the branch channels through a ReLU
    L = next(L for L in r["tape"] if L.op == "conv" and L.args.get("xf.lo") is not None)
    xf = [L.args["xf." + f].before for f in ("sub", "scale", "shift", "lo")]
    assert torch.equal(xf[3][:64], torch.zeros(64)) and bool((xf[3][64:] == OPS.NEG_BIG).all()), "ReLU floor of the virtual concat"
    assert bool((xf[0][64:] == 0).all()) and bool((xf[1][64:] == 1).all()) and bool((xf[2][64:] == 0).all()), "pooled channels: identity"
    r["outputs"] = [cpost, r["res"]]
    return r


# ------------------------------------------------------------------------------------------------------------------
# stem, head and the whole networks
# ------------------------------------------------------------------------------------------------------------------
_STEM_TAPS = [(ky - 3, 0, ky) for ky in range(7)]
_STEM_WTAPS = [(ky - 3, 0, 7 * ky) for ky in range(7)]


def _chan_slice(g, name, base, c0, n):
    """channels [c0, c0 + n) of an NHWC symbol, with the strides of the whole buffer"""
    N, H, W, C = base.shape
    if c0 == 0 and n == C:          # (a one-plane image: the plane's 16 channels are the whole expanded tensor)
        return base
    return g.view(name, base, c0, (N, H, W, n), (H * W * C, W * C, C, 1))


def _stats_sym(g, tag, site):
    return g.ext(tag + ".stats", site[1].stats) if site[1].stats is not None else None


def expect_stem_pool_fwd(g, eng, m, tag, x, cat1, dt, training, save=True):
    """conv1 as Engine.stem_fwd runs it -- the caller's NCHW image expanded to 16 channels per plane (column shifts), then one 7-tap
    vertical conv per plane: plane 0 carries the bias, planes > 0 add onto c0 in place, the LAST plane takes bn1's statistics --
    bn1's finalize, and MaxPool2d(3, 2, 1) of relu(bn1(c0)) formed on load, which also copies the transformed pixels into the skip
    half of dec_layer1's concat buffer and (when saving) keeps each window's arg-max tap.  x: Sym of the NCHW image; cat1: Sym"""
    N, Cin, H, W = x.shape
    ip, dev = m.inplanes, m.conv1.weight.device
    s = BlockSyms()
    s.m, s.tag, s.dt, s.x = m, tag, dt, x
    s.bn1 = _site_syms(g, eng, m.bn1, tag + ".bn1")
    s.x16 = g.new(tag + ".x16", (N, H, W, 16 * Cin), dt)
    s.c0 = g.new(tag + ".c0", (N, H, W, ip), dt)
    g.node("stem_expand", writes=("out",), x_nchw=x, out=s.x16)
    st = _stats_sym(g, tag + ".bn1", s.bn1)
    for ci in range(Cin):
        a = dict(x=_chan_slice(g, "%s.x16[%d]" % (tag, ci), s.x16, 16 * ci, 16), wp=g.ext("%s.W1[%d]" % (tag, ci), eng.packed(m.conv1.weight, "stem%d" % ci)),
                 y=s.c0, taps=_STEM_TAPS, Cout=ip, S=1, bias=g.ext(tag + ".b1", m.conv1.bias) if ci == 0 else None,
                 addend=s.c0 if ci > 0 else None, addend_mask=None, stats=st if ci == Cin - 1 else None, stats_slots=0, logsoftmax=False)
        _aff(a, "xf", None)
        g.node("conv", writes=("y", "stats"), **a)
    _finish(g, eng, m.bn1, s.bn1[0], s.bn1[1], N * H * W, training, st)
    s.p0 = g.new(tag + ".p0", (N, H // 2, W // 2, ip), dt)
    s.amax = g.new(tag + ".amax", (N, H // 2, W // 2, ip), torch.uint8) if save else None
    s.xf = _relu_aff(g, eng, s.bn1, tag + ".bn1", dev)
    p = dict(x=s.c0, pooled=s.p0, xcopy=_chan_slice(g, tag + ".x0", cat1, ip, ip), stride=2, argmax=s.amax)
    _aff(p, "xf", s.xf)
    g.node("maxpool_fwd", writes=("pooled", "xcopy", "argmax"), **p)
    return s


def expect_stem_pool_bwd(g, eng, s, g_p0, g_x0, G, fin_max=None):
    """the pool's backward through the SAVED arg-max with the skip's gradient as g_extra, bn1's backward, one weight gradient per
    plane into conv1's dW at dst_offset = 49 * plane (row stride Cin * 49, the 7 column shifts as 7 `input channels` of stride 1),
    and the bias gradient"""
    from ubresnet_amd import engine as E
    fin_max = E._FIN_MAX_C if fin_max is None else fin_max
    m, tag, dt = s.m, s.tag, s.dt
    N, H, W, ip = s.c0.shape
    Cin = s.x16.shape[3] // 16
    g_a0 = g.new(tag + ".g_a0", s.c0.shape, dt)
    p = dict(x=s.c0, g_pooled=g_p0, g_extra=g_x0, gx=g_a0, stride=2, argmax=s.amax)
    _aff(p, "xf", s.xf)
    g.node("maxpool_bwd", writes=("gx",), **p)
    g_c0 = _bn_bwd_site(g, eng, s.bn1, m.bn1, tag + ".bn1", g_a0, s.c0, G, N * H * W, dt, fin_max)
    dW = g.ext(tag + ".dW1", G(m.conv1.weight))
    for ci in range(Cin):
        _wgrad(g, tag, _chan_slice(g, "%s.x16[%d]" % (tag, ci), s.x16, 16 * ci, 16), g_c0, _STEM_WTAPS, dW, Cin * 49, 1, ip, 7, 1, None,
               dst_offset=ci * 49, exclusive=True)
    _bias_grad(g, tag + ".b1", g_c0, ip, g.ext(tag + ".db1", G(m.conv1.bias)))


def expect_head_fwd(g, eng, m, tag, d1o, dt, training):
    """conv10 7x7 + bias + statistics -> bn10 -> conv11 7x7 over relu(bn10(c10)) formed on load + bias + the LogSoftmax epilogue into
    a NEW contiguous fp32 NCHW tensor"""
    N, H, W, ip = d1o.shape
    nk, ncls, dev = m.conv10.out_channels, m.conv11.out_channels, m.conv10.weight.device
    h = BlockSyms()
    h.m, h.tag, h.dt, h.d1o = m, tag, dt, d1o
    h.bn10 = _site_syms(g, eng, m.bn10, tag + ".bn10")
    h.c10 = g.new(tag + ".c10", (N, H, W, nk), dt)
    st = _stats_sym(g, tag + ".bn10", h.bn10)
    a = dict(x=d1o, wp=g.ext(tag + ".W10", eng.packed(m.conv10.weight, "fwd")), y=h.c10, taps=OPS.conv_taps(7, 1, 3), Cout=nk, S=1,
             bias=g.ext(tag + ".b10", m.conv10.bias), addend=None, stats=st, stats_slots=0, logsoftmax=False)
    _aff(a, "xf", None)
    g.node("conv", writes=("y", "stats"), **a)
    _finish(g, eng, m.bn10, h.bn10[0], h.bn10[1], N * H * W, training, st)
    h.logp = Sym(tag + ".logp", (N, ncls, H, W), torch.float32, stride=(ncls * H * W, H * W, W, 1))
    h.xf = _relu_aff(g, eng, h.bn10, tag + ".bn10", dev)
    a = dict(x=h.c10, wp=g.ext(tag + ".W11", eng.packed(m.conv11.weight, "fwd")), y=h.logp, taps=OPS.conv_taps(7, 1, 3), Cout=ncls, S=1,
             bias=g.ext(tag + ".b11", m.conv11.bias), addend=None, stats=None, logsoftmax=True)
    _aff(a, "xf", h.xf)
    g.node("conv", writes=("y",), **a)
    return h


def expect_head_bwd(g, eng, h, g_logp, G, fin_max=None):
    """-> the gradient of dec_layer1's output.  The logit gradient lives in 16 zero-padded channels: conv11's weight gradient reads
    ncls of them, its bias gradient is every 16th ... of a 16-wide channel sum (stride = 16), its data gradient runs over all 16"""
    from ubresnet_amd import engine as E
    fin_max = E._FIN_MAX_C if fin_max is None else fin_max
    m, tag, dt = h.m, h.tag, h.dt
    N, H, W, nk = h.c10.shape
    ip, ncls, NS = h.d1o.shape[3], h.logp.shape[1], kref.STAT_SLOTS
    g_l = g.new(tag + ".g_l", (N, H, W, 16), dt)
    g.node("logsoftmax_bwd", writes=("g_logits",), g_logp=g_logp, logp=h.logp, g_logits=g_l)
    T7 = OPS.conv_taps(7, 1, 3)
    _wgrad(g, tag, h.c10, g_l, T7, g.ext(tag + ".dW11", G(m.conv11.weight)), nk * 49, 49, ncls, nk, 1, h.xf)
    red = g.new(tag + ".bred", (NS * (16 + nk),), torch.float64)
    r11, r10 = g.view(tag + ".bred11", red, 0, (NS * 16,)), g.view(tag + ".bred10", red, NS * 16, (NS * nk,))
    g.node("channel_sum", writes=("red",), g=g_l, red=r11)
    g.node("cast_f64_to_f32", writes=("dst",), src=r11, dst=g.ext(tag + ".db11", G(m.conv11.bias)), n=ncls, scale=1.0, accumulate=False,
           stride=16, slots=NS)
    g_a10 = g.new(tag + ".g_a10", h.c10.shape, dt)
    _dgrad(g, eng, m.conv11, tag + ".W11t", g_l, g_a10, 1, 7)
    g_c10 = _bn_bwd_site(g, eng, h.bn10, m.bn10, tag + ".bn10", g_a10, h.c10, G, N * H * W, dt, fin_max)
    _wgrad(g, tag, h.d1o, g_c10, T7, g.ext(tag + ".dW10", G(m.conv10.weight)), ip * 49, 49, nk, ip, 1, None)
    g.node("channel_sum", writes=("red",), g=g_c10, red=r10)
    g.node("cast_f64_to_f32", writes=("dst",), src=r10, dst=g.ext(tag + ".db10", G(m.conv10.bias)), n=nk, scale=1.0, accumulate=False,
           stride=None, slots=NS)
    gd = g.new(tag + ".g_d1o", h.d1o.shape, dt)
    _dgrad(g, eng, m.conv10, tag + ".W10t", g_c10, gd, 1, 7)
    return gd


def _expect_net(g, eng, m, x, g_logp, G, dt, cats, bottom, enc, xf, mid_fwd, owed_of, g_x0_of):
    """the pass both networks share (Engine.uresnet_* / aspp_*): stem + pool, enc_layer1 .. 5 each writing its slice `enc[i]`,
    (ASPP levels: mid_fwd), dec_layer5 .. 1 from `bottom` through cats, the head; then the head's, the decoder's (dec_layer1 .. 5),
    the encoder's (5 .. 1, level i owed owed_of(gc, g_bottom)[i - 1]) and the stem's backward"""
    training = True
    fused = lambda blk, c: tail_fused(eng, blk, training, c)
    st = expect_stem_pool_fwd(g, eng, m, "stem", x, cats[0], dt, training)
    t, encs = st.p0, []
    for i in range(1, 6):
        dbl = getattr(m, "enc_layer%d" % i)
        encs.append(expect_double_fwd(g, eng, dbl, "enc%d" % i, t, enc[i - 1], dt, training, fused(dbl.res1, enc[i - 1].shape[3])))
        t = enc[i - 1]
    mid = mid_fwd() if mid_fwd is not None else None
    t, decs = bottom, [None] * 5
    for i in (5, 4, 3, 2, 1):
        dl, cat = getattr(m, "dec_layer%d" % i), cats[i - 1]
        co = dl.res.res2.conv2.out_channels
        out = g.new("dec%d.out" % i, cat.shape[:3] + (co,), dt)
        xf_x, xf_cat = xf.get(i, (None, None))
        decs[i - 1] = expect_declayer_fwd(g, eng, dl, "dec%d" % i, t, cat, dl.deconv.out_channels, out, dt, training, fused(dl.res.res1, co), xf_x, xf_cat)
        t = out
    hd = expect_head_fwd(g, eng, m, "head", t, dt, training)
    gr = expect_head_bwd(g, eng, hd, g_logp, G)
    gc = []
    for i in (1, 2, 3, 4, 5):
        gr, g_cat = expect_declayer_bwd(g, eng, getattr(m, "dec_layer%d" % i), "dec%d" % i, decs[i - 1], gr, G, dt)
        gc.append(g_cat)
    gr, owed = owed_of(gc, gr, mid)
    for i in (5, 4, 3, 2, 1):
        o = owed[i - 1]() if callable(owed[i - 1]) else owed[i - 1]
        gr = expect_double_bwd(g, eng, encs[i - 1], gr, o, G)
    expect_stem_pool_bwd(g, eng, st, gr, g_x0_of(gc), G)
    return hd.logp


def expect_uresnet(g, eng, m, x, g_logp, G, dt):
    """Engine.uresnet_forward / uresnet_backward.  cat_i = [deconv | skip]: enc_layer i writes channels [Cd, 2 Cd) of cat_{i+1}
    (enc_layer5 the bottom tensor), dec_layer i reads all of cat_i, and in backward enc_layer i is owed channels [Cd, 2 Cd) of
    dec_layer {i+1}'s g_cat.  -> the Sym of the log-probabilities"""
    N, _, H, W = x.shape
    ip = m.inplanes
    cats = [g.new("cat%d" % (i + 1), (N, H >> i, W >> i, (2 << i) * ip), dt) for i in range(5)]
    x5 = g.new("x5", (N, H >> 5, W >> 5, 32 * ip), dt)
    enc = [_chan_slice(g, "cat%d.skip" % (i + 1), cats[i], (1 << i) * ip, (1 << i) * ip) for i in (1, 2, 3, 4)] + [x5]

    def owed_of(gc, g_bottom, mid):
        return g_bottom, [_chan_slice(g, "dec%d.g_skip" % (i + 1), gc[i], (1 << i) * ip, (1 << i) * ip) for i in (1, 2, 3, 4)] + [None]
    return _expect_net(g, eng, m, x, g_logp, G, dt, cats, x5, enc, {}, None, owed_of, lambda gc: _chan_slice(g, "dec1.g_skip", gc[0], ip, ip))


def expect_aspp_net(g, eng, m, x, g_logp, G, dt, arena):
    """Engine.aspp_forward / aspp_backward.  cat4 / cat5 = [deconv | ASPP_post(e) | e] and the bottom tensor skip5 = [ASPP_post(e5) |
    e5]; the post convs' BatchNorm + ReLU and the identity of the other channels reach dec_layer5 / dec_layer4 as slices of the
    per-pass affine arena [acat3 | acat4 | acat5 | cat4 | cat5 | skip5]; each ASPP level's backward is issued right before the
    encoder level it feeds (level 5's before the encoder's)"""
    N, _, H, W = x.shape
    ip = m.inplanes
    C3, C4, C5 = 8 * ip, 16 * ip, 32 * ip
    sizes = [64 + C3, 64 + C4, 64 + C5, 3 * C3, 3 * C4, 2 * C5]
    offs = [sum(sizes[:i]) for i in range(6)]
    cats = [g.new("cat%d" % (i + 1), (N, H >> i, W >> i, c), dt) for i, c in enumerate([2 * ip, 4 * ip, 8 * ip, 3 * C3, 3 * C4])]
    skip5 = g.new("skip5", (N, H >> 5, W >> 5, 2 * C5), dt)
    enc = [_chan_slice(g, "cat2.skip", cats[1], 2 * ip, 2 * ip), _chan_slice(g, "cat3.skip", cats[2], 4 * ip, 4 * ip),
           _chan_slice(g, "cat4.skip", cats[3], 2 * C3, C3), _chan_slice(g, "cat5.skip", cats[4], 2 * C4, C4), _chan_slice(g, "skip5.e5", skip5, C5, C5)]
    posts = [_chan_slice(g, "cat4.post", cats[3], C3, C3), _chan_slice(g, "cat5.post", cats[4], C4, C4), _chan_slice(g, "skip5.post", skip5, 0, C5)]
    levels = eng._aspp_levels()
    rows = [g.ext("arena%d" % r, arena[r]) for r in range(4)]
    aff = lambda nm, off, n: tuple(g.view("%s.xf%d" % (nm, r), rows[r], off, (n,)) for r in range(4))
    xf = {5: (aff("dec5.x", offs[5], 2 * C5), aff("dec5.cat", offs[4], 3 * C4)), 4: (None, aff("dec4.cat", offs[3], 3 * C3))}

    def mid_fwd():
        return [expect_aspp_fwd(g, eng, layer, post, "aspp%d" % (3 + k), enc[2 + k], posts[k], arena, offs[k], o_post, dt, True)
                for k, ((layer, post), o_post) in enumerate(zip(levels, (offs[3] + C3, offs[4] + C4, offs[5])))]

    def owed_of(gc, gs5, mid):
        a3, a4, a5 = mid
        g_e5 = expect_aspp_bwd(g, eng, a5, _chan_slice(g, "dec5.g_post", gs5, 0, C5), _chan_slice(g, "dec5.g_e5", gs5, C5, C5), G)
        lvl = lambda a, gcat, nm, C: (lambda: expect_aspp_bwd(g, eng, a, _chan_slice(g, nm + ".g_post", gcat, C, C), _chan_slice(g, nm + ".g_e", gcat, 2 * C, C), G))
        return g_e5, [_chan_slice(g, "dec2.g_skip", gc[1], 2 * ip, 2 * ip), _chan_slice(g, "dec3.g_skip", gc[2], 4 * ip, 4 * ip),
                      lvl(a3, gc[3], "dec4", C3), lvl(a4, gc[4], "dec5c", C4), None]
    return _expect_net(g, eng, m, x, g_logp, G, dt, cats, skip5, enc, xf, mid_fwd, owed_of, lambda gc: _chan_slice(g, "dec1.g_skip", gc[0], ip, ip))


class _Stem(torch.nn.Module):
    def __init__(self, cin, ip):
        super().__init__()
        self.inplanes = ip
        self.conv1 = torch.nn.Conv2d(cin, ip, kernel_size=7, stride=1, padding=3, bias=True)
        self.bn1 = torch.nn.BatchNorm2d(ip)

    def _grad_completion_order(self):
        return [("bn1.weight", self.bn1.weight), ("bn1.bias", self.bn1.bias), ("conv1.weight", self.conv1.weight), ("conv1.bias", self.conv1.bias)]


class _Head(torch.nn.Module):
    def __init__(self, ip, nk, ncls):
        super().__init__()
        self.inplanes = ip
        self.conv10 = torch.nn.Conv2d(ip, nk, kernel_size=7, stride=1, padding=3, bias=True)
        self.bn10 = torch.nn.BatchNorm2d(nk)
        self.conv11 = torch.nn.Conv2d(nk, ncls, kernel_size=7, stride=1, padding=3, bias=True)

    def _grad_completion_order(self):
        return [("conv11.weight", self.conv11.weight), ("conv11.bias", self.conv11.bias), ("conv10.weight", self.conv10.weight),
                ("conv10.bias", self.conv10.bias), ("bn10.weight", self.bn10.weight), ("bn10.bias", self.bn10.bias)]


def nll_grad(shape, seed, device):
    """fp32 NCHW gradient of the log-probabilities in the shape PixelWiseNLLLoss's backward leaves: one class per pixel holds
    -(weight) (non-dyadic), the others zero; about a quarter of the pixels (ignored labels) are all zero"""
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    cls = torch.randint(0, C, (N, 1, H, W), generator=gen)
    w = -(torch.rand((N, 1, H, W), generator=gen) * 0.9 + 0.1) / 64.0
    w = w * (torch.rand((N, 1, H, W), generator=gen) >= 0.25)
    return torch.zeros(shape).scatter_(1, cls, w).contiguous().to(device)


def stem_case(monkeypatch, dt, device, N, cin, H, W, ip, training=True, emu=False):
    """Engine.stem_pool_fwd / stem_pool_bwd on their own: cat1 NaN-filled (only its skip half may change), g_x0 a channel slice of a
    wider buffer.  training = False: bn1 frozen, nothing saved, no arg-max, no backward"""
    from ubresnet_amd.engine import Saved
    m = _Stem(cin, ip)
    x = noise((N, cin, H, W), torch.float32, 51, device)
    cat1 = torch.full((N, H, W, 2 * ip), float("nan"), dtype=dt, device=device)
    g_p0 = noise((N, H // 2, W // 2, ip), dt, 52, device)
    g_x0 = noise((N, H, W, 2 * ip), dt, 53, device)[..., ip:]
    sv, st = Saved(), {}
    sv.dt = dt

    def build(eng, G):
        def fwd():
            eng._save = training
            st["p0"] = eng.stem_pool_fwd(m, x, cat1, training, dt, sv)
        bwd = (lambda _: eng.stem_pool_bwd(m, sv, g_p0, g_x0, G)) if training else None

        def expect(g):
            s = expect_stem_pool_fwd(g, eng, m, "stem", g.ext("x", x), g.ext("cat1", cat1), dt, training, save=training)
            if training:
                expect_stem_pool_bwd(g, eng, s, g.ext("g_p0", g_p0), g.ext("g_x0", g_x0), G)
        return fwd, bwd, expect
    r = run_stage(monkeypatch, m, dt, device, training, build, emu, kind="uresnet")
    assert bool(torch.isnan(cat1[..., :ip]).all()), "the deconv half of cat1 was written"
    r["outputs"] = [st["p0"], cat1[..., ip:]]
    return r


def head_case(monkeypatch, dt, device, N, H, W, ip, nk, ncls, freeze=(), emu=False):
    """Engine.head_fwd / head_bwd on their own, training mode (freeze: BatchNorm modules in eval mode)"""
    from ubresnet_amd.engine import Saved
    m = _Head(ip, nk, ncls)
    d1o = noise((N, H, W, ip), dt, 61, device)
    g_logp = nll_grad((N, ncls, H, W), 62, device)
    sv, st = Saved(), {}
    sv.x = d1o

    def build(eng, G):
        def fwd():
            st["out"] = eng.head_fwd(m, d1o, True, dt, sv)
        bwd = lambda _: eng.head_bwd(m, sv, g_logp, G)

        def expect(g):
            h = expect_head_fwd(g, eng, m, "head", g.ext("d1o", d1o), dt, True)
            expect_head_bwd(g, eng, h, g.ext("g_logp", g_logp), G)
        return fwd, bwd, expect
    r = run_stage(monkeypatch, m, dt, device, True, build, emu, freeze, kind="uresnet")
    check_head_records(r["tape"], ncls)
    r["outputs"] = [st["out"], r["res"]]
    return r


def check_head_records(tape, ncls):
    """the log-probabilities are a tensor of their own that no earlier launch has seen (fresh memory from every pass), and the
    padding channels [ncls, 16) of the logit gradient hold zero BITS"""
    i, L = next((i, L) for i, L in enumerate(tape) if L.op == "conv" and L.args["logsoftmax"])
    y = L.args["y"]
    assert y.off == 0 and y.base_before.numel() == y.before.numel(), "the log-probabilities are a view into a larger buffer"
    seen = {v.base for P in tape[:i] for v in P.args.values() if isinstance(v, TRec)}
    assert y.base not in seen, "the log-probabilities were written into memory an earlier launch of the pass used"
    gl = next(L for L in tape if L.op == "logsoftmax_bwd").args["g_logits"].after
    assert gl.shape[-1] == 16 and not bool((kref.bits(gl[..., ncls:]) != 0).any()), "padding channels of the logit gradient are not zero bits"


def net_case(monkeypatch, dt, device, which, emu=False):
    """a whole training pass, forward and backward, through Engine.forward_eager / backward_eager (never the plan), with the
    weight-gradient side stream off (as run_stage): UResNet(3 classes, 1 plane, inplanes 16) or ASPP_ResNet (3 planes) at 2 x 32 x 64,
    the smallest input the engine takes with H != W: the bottom level is 1 x 2"""
    import time
    from ubresnet_amd.engine import Engine
    monkeypatch.setenv("UBR_WGRAD_STREAM", "0")
    if which == "uresnet":
        from ubresnet_amd.models.ub_uresnet import UResNet
        m, cin = UResNet(num_classes=3, input_channels=1, inplanes=16), 1
    else:
        from ubresnet_amd.models.ASPP_ResNet import ASPP_ResNet
        m, cin = ASPP_ResNet(num_classes=3, in_channels=3, inplanes=16, showsizes=False), 3
    init_params(m, 7)
    m = m.to(device)
    m.train()
    eng = Engine(m, which)
    if emu:
        emulate(monkeypatch, eng)
    tap = Tap(monkeypatch)
    x = noise((2, cin, 32, 64), torch.float32, 71, device)
    g_logp = nll_grad((2, 3, 32, 64), 72, device)
    t0 = time.time()
    out, sv = eng.forward_eager(x, True, dt, True)
    flat, views = eng.backward_eager(sv, g_logp)
    tap._sync()
    t_run = time.time() - t0
    graph = Graph()
    G = lambda p: views[id(p)]
    gx, gg = graph.ext("x", x), graph.ext("g_logp", g_logp)
    if which == "uresnet":
        expect_uresnet(graph, eng, m, gx, gg, G, dt)
    else:
        expect_aspp_net(graph, eng, m, gx, gg, G, dt, sv.arena)
    check_head_records(tap.tape, 3)
    return dict(tape=tap.tape, graph=graph, flat=flat, eng=eng, res=None, sv=sv, outputs=[out], t_run=t_run)


# ------------------------------------------------------------------------------------------------------------------
# tape mutations: what a wiring bug would have recorded (the launches themselves are never touched)
# ------------------------------------------------------------------------------------------------------------------
def _copy_rec(r, **kw):
    c = TRec.__new__(TRec)
    c.__dict__.update(r.__dict__)
    c.__dict__.update(kw)
    return c


def mutate(tape, kind):
    """a copy of the tape with ONE record changed -> (tape, description)"""
    tape = [Launch(L.op, dict(L.args)) for L in tape]
    find = lambda pred: next(L for L in tape if pred(L))
    if kind == "swap_bn2_bnpass":
        L = find(lambda L: L.op.startswith("block_tail_bwd_apply") and L.args.get("cb") is not None)
        for p, q in (("scale2", "scale_b"), ("mean2", "mean_b"), ("invstd2", "invstd_b")):
            L.args[p], L.args[q] = L.args[q], L.args[p]
        return tape, "bn2's and bnpass's vectors swapped in the tail's apply pass"
    if kind == "xf_identity":
        L = find(lambda L: L.op == "conv" and L.args.get("xf.scale") is not None)
        C = L.args["xf.scale"].before.numel()
        for f, val in (("sub", 0.0), ("scale", 1.0), ("shift", 0.0), ("lo", kref.NEG_BIG)):
            r = L.args["xf." + f]
            L.args["xf." + f] = _copy_rec(r, before=torch.full((C,), val), ptr=r.ptr + 4096)
        return tape, "a conv's on-load affine replaced by the identity"
    if kind == "half_mask":
        L = find(lambda L: L.op.startswith("block_tail_fwd") and L.args.get("relu_mask") is not None)
        r = L.args["relu_mask"]
        n = r.shape[0] // 2
        L.args["relu_mask"] = _copy_rec(r, shape=(n,), before=r.before[:n].clone(), after=r.after[:n].clone())
        return tape, "the ReLU mask at half its length (the fp32 unit width in a 16-bit type)"
    if kind == "swap_red":
        L = find(lambda L: L.op.startswith("block_tail_bwd_apply_fin") and L.args.get("red_b") is not None)
        L.args["red2"], L.args["red_b"] = L.args["red_b"], L.args["red2"]
        return tape, "red2 and redb exchanged in the tail's apply pass"
    if kind == "dtype_fp32":
        L = find(lambda L: L.op == "conv")
        L.args["y"] = _copy_rec(L.args["y"], dtype=torch.float32)
        return tape, "a conv output recorded as fp32"
    # --- whole-network wiring (a whole-UResNet tape; the stem's second plane: the three-plane stem case's tape)
    if kind == "owed_from_level3":
        # the tails that take a second gradient operand are enc_layer4 .. 1's res2, in this order: levels 3 and 2 are the 2nd and 3rd
        Ls = [L for L in tape if L.op == "block_tail_bwd_reduce" and L.args.get("go2") is not None]
        assert len(Ls) == 4
        Ls[2].args["go2"] = Ls[1].args["go2"]
        return tape, "the skip gradient owed to enc_layer2 taken from the buffer owed to enc_layer3"
    if kind == "enc_slice_offset":
        L = find(lambda L: L.op.startswith("block_tail_fwd") and L.args["out"].stride[2] != L.args["out"].shape[3])
        r = L.args["out"]
        L.args["out"] = _copy_rec(r, ptr=r.ptr + 16 * r.before.element_size(), off=r.off + 16)
        return tape, "an encoder level's output one 16-channel unit further into its concat buffer"
    if kind == "stem_plane_offset":
        L = find(lambda L: L.op == "wgrad" and L.args["dst_offset"] == 49)
        L.args["dst_offset"] = 0
        return tape, "the stem's second-plane weight gradient at dst_offset 0"
    if kind == "head_xf_identity":
        L = find(lambda L: L.op == "conv" and L.args["logsoftmax"])
        for f, val in (("sub", 0.0), ("scale", 1.0), ("shift", 0.0), ("lo", kref.NEG_BIG)):
            r = L.args["xf." + f]
            L.args["xf." + f] = _copy_rec(r, before=torch.full((r.before.numel(),), val), ptr=r.ptr + 4096)
        return tape, "conv11's on-load affine (bn10 + ReLU) replaced by the identity"
    raise KeyError(kind)


MUTATIONS = ("swap_bn2_bnpass", "xf_identity", "half_mask", "swap_red", "dtype_fp32")
NET_MUTATIONS = ("owed_from_level3", "enc_slice_offset", "head_xf_identity")      # on a whole-UResNet tape
STEM_MUTATIONS = ("stem_plane_offset",)                                            # on the three-plane stem case's tape
VALUE_MUTATIONS = ("swap_bn2_bnpass", "xf_identity", "swap_red", "head_xf_identity")      # change recorded values: the replay alone sees them


# ------------------------------------------------------------------------------------------------------------------
# running a stage under the tap (as tests/test_gpu_blocks._run does: no side stream, one flush, the flat buffer read after it)
# ------------------------------------------------------------------------------------------------------------------
class _Wrap(torch.nn.Module):
    def __init__(self, mod):
        super().__init__()
        self.mod = mod

    def _grad_completion_order(self):
        return self.mod._grad_completion_order("mod.")


def noise(shape, dt, seed, device):
    """sparse noise with whole zero 16x16 tiles (kref.exact_operands' pattern) at realistic, non-dyadic magnitude"""
    m = kref.exact_operands(shape, torch.float32, density=0.4, seed=seed, zero_tiles=0.3)
    v = torch.rand(shape, generator=torch.Generator().manual_seed(seed + 1000)) * 0.9 + 0.1
    return (m * v).to(dt).to(device)


def init_params(mod, seed):
    """non-trivial gamma / beta / running statistics on every BatchNorm; channel 1 of each has gamma = 0"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.num_features
                m.weight.copy_(torch.rand(C, generator=g) + 0.5)
                m.weight[1] = 0.0
                m.bias.copy_(torch.rand(C, generator=g) * 0.6 - 0.3)
                m.running_mean.copy_(torch.rand(C, generator=g) * 0.2 - 0.1)
                m.running_var.copy_(torch.rand(C, generator=g) * 0.5 + 0.25)


def run_stage(monkeypatch, mod, dt, device, training, build, emu=False, freeze=(), kind="custom"):
    """build(eng, G) -> (fwd, bwd, expect): fwd() runs the stage forward and returns its record, bwd(rec) its backward;
    expect(graph) writes the expected launches.  -> dict(tape, stat, grads=(n, ratio), eng)"""
    from ubresnet_amd.engine import Engine, Saved
    init_params(mod, 7)
    mod = mod.to(device)
    mod.train(training)
    for name in freeze:            # a BatchNorm module in eval mode inside a training pass: the site uses its running statistics
        getattr(mod, name).eval()
    # (kind "uresnet": a module that carries conv1 / conv10 / conv11 itself, so that the engine packs the stem planes and conv11's
    # padded data-gradient image as it does for the networks)
    eng = Engine(_Wrap(mod), "custom") if kind == "custom" else Engine(mod, kind)
    if emu:
        emulate(monkeypatch, eng)
    tap = Tap(monkeypatch)
    sv = Saved()
    eng._alloc_pass_workspaces(sv, torch.device(device), training)
    eng._save = True
    dev = torch.device(device, 0) if device == "cuda" else torch.device(device)
    eng.pack_all(dt, dev, "fwd")
    eng.pack_all(dt, dev, "bwd")
    flat = torch.zeros(eng.grad_numel, device=device)
    views = {}
    for name, p in eng.grad_order:
        o = eng.grad_offsets[name]
        views[id(p)] = flat[o:o + p.numel()].view(p.shape)
    G = lambda p: views[id(p)]
    fwd, bwd, expect = build(eng, G)
    rec = fwd()
    res = bwd(rec) if bwd is not None else None
    eng._fin_flush()       # (dgamma / dbeta of frozen sites: the end of a stage, as Engine._stage_notifier does)
    eng._wg_flush()
    tap._sync()
    graph = Graph()
    expect(graph)
    return dict(tape=tap.tape, graph=graph, flat=flat, eng=eng, res=res, sv=sv)


def check_all(r):
    """dataflow, per-launch numerics, the gradient buffer -> {op: (launches, worst ratio)}"""
    r["graph"].match(r["tape"])
    stat = replay(r["tape"])
    nw, w = check_gradients(r["tape"], r["flat"], r["flat"].data_ptr())
    if nw:
        stat["wgrad"] = (nw, w)
    r["exact"] = check_chain(r["tape"], r["flat"], r["outputs"])
    return stat


def tail_fused(eng, blk, training, cout):
    """the tail makes bn2's (and bnpass's) vectors itself only when every one of them comes from batch statistics, and the
    vectors of both sites (2 x 3 x C floats = 24 C bytes) fit the 64 KiB of LDS a workgroup of tail_fwd_kernel may carve out
    (ubr_block_tail_fwd rejects a fused descriptor beyond that)"""
    sites = [eng.bn(blk.bn2)] + ([eng.bn(blk.bnpass)] if blk.bypass is not None else [])
    return training and not any(s.frozen for s in sites) and 24 * cout <= 64 * 1024


def block_case(monkeypatch, dt, device, cin, cout, stride, hw, training=True, go2=False, virtual=False, fin_max=None, backward=True,
               emu=False, freeze=()):
    from ubresnet_amd.models.common_layers import BasicBlock
    from ubresnet_amd import engine as E
    if fin_max is not None:
        monkeypatch.setattr(E, "_FIN_MAX_C", fin_max)
    H, W = hw
    blk = BasicBlock(cin, cout, stride)
    x = noise((2, H, W, cin), dt, 11, device)
    out = torch.empty((2, H // stride, W // stride, cout), dtype=dt, device=device)
    go = noise(tuple(out.shape), dt, 12, device)
    g2 = noise(tuple(out.shape), dt, 13, device) if go2 else None
    xf = None
    if virtual:
        gen = torch.Generator().manual_seed(5)
        xf = OPS.Affine(*[t.to(device) for t in (torch.rand(cin, generator=gen) * 0.2, torch.rand(cin, generator=gen) + 0.5,
                                                 torch.rand(cin, generator=gen) * 0.4 - 0.2, torch.zeros(cin))])

    def build(eng, G):
        fused = tail_fused(eng, blk, training, cout)
        fwd = lambda: eng.block_fwd(blk, x, out, training, dt, xf)
        bwd = (lambda rec: eng.block_bwd(rec, go, g2, G)) if backward else None

        def expect(g):
            xs = tuple(g.ext("xf_in." + f, getattr(xf, f)) for f in ("sub", "scale", "shift", "lo")) if xf is not None else None
            b = expect_block_fwd(g, eng, blk, "blk", g.ext("x", x), g.ext("out", out), dt, training, fused, xs)
            if backward:
                expect_block_bwd(g, eng, b, g.ext("go", go), g.ext("go2", g2) if go2 else None, G)
        return fwd, bwd, expect
    r = run_stage(monkeypatch, blk, dt, device, training, build, emu, freeze)
    r["outputs"] = [out] + ([r["res"]] if r["res"] is not None else [])
    return r


def double_case(monkeypatch, dt, device, cin, cout, stride, hw, need_gx=True, emu=False):
    from ubresnet_amd.models.common_layers import DoubleResNet
    H, W = hw
    dbl = DoubleResNet(cin, cout, stride)
    x = noise((2, H, W, cin), dt, 21, device)
    out = torch.empty((2, H // stride, W // stride, cout), dtype=dt, device=device)
    go = noise(tuple(out.shape), dt, 22, device)

    def build(eng, G):
        fwd = lambda: eng.double_fwd(dbl, x, out, True, dt)
        bwd = lambda recs: eng.double_bwd(recs, go, None, G, need_gx)

        def expect(g):
            bs = expect_double_fwd(g, eng, dbl, "dbl", g.ext("x", x), g.ext("out", out), dt, True, tail_fused(eng, dbl.res1, True, cout))
            expect_double_bwd(g, eng, bs, g.ext("go", go), None, G, need_gx)
        return fwd, bwd, expect
    r = run_stage(monkeypatch, dbl, dt, device, True, build, emu)
    r["outputs"] = [out] + ([r["res"]] if r["res"] is not None else [])
    return r


def declayer_case(monkeypatch, dt, device, cin, cd, cskip, cout, hw, emu=False):
    from ubresnet_amd.models.common_layers import ConvTransposeLayer
    H, W = hw
    ctl = ConvTransposeLayer(cin, cd, cout)
    assert cd + cskip == ctl.res.res1.conv1.in_channels
    x = noise((2, H, W, cin), dt, 31, device)
    cat = torch.full((2, 2 * H, 2 * W, cd + cskip), float("nan"), dtype=dt, device=device)
    cat[..., cd:] = noise((2, 2 * H, 2 * W, cskip), dt, 32, device)
    out = torch.empty((2, 2 * H, 2 * W, cout), dtype=dt, device=device)
    go = noise(tuple(out.shape), dt, 33, device)

    def build(eng, G):
        fwd = lambda: eng.declayer_fwd(ctl, x, cat, cd, out, True, dt)
        bwd = lambda rec: eng.declayer_bwd(rec, go, G)

        def expect(g):
            fw = expect_declayer_fwd(g, eng, ctl, "ctl", g.ext("x", x), g.ext("cat", cat), cd, g.ext("out", out), dt, True,
                                     tail_fused(eng, ctl.res.res1, True, cout))
            expect_declayer_bwd(g, eng, ctl, "ctl", fw, g.ext("go", go), G, dt)
        return fwd, bwd, expect
    r = run_stage(monkeypatch, ctl, dt, device, True, build, emu)
    r["outputs"] = [out, cat, r["res"][0], r["res"][1]]
    return r
