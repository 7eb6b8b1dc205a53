"""Graph executor for the U-ResNet family: drives the HIP kernels for forward and backward.

The reference expresses the network as torch.nn layer calls (models/ub_uresnet.py:88-147,
models/common_layers.py:39-58,127-132) and leaves scheduling to autograd.  Here the module tree
only OWNS parameters; this executor runs the fused schedule explicitly:

  * NHWC activations; skip connections are written straight into the channel slice of the
    decoder's concat buffer (torch.cat of models/common_layers.py:130 never materialises).
  * train-mode BatchNorm: the producing conv accumulates sum/sum-of-squares in its epilogue,
    a tiny finalize kernel makes (scale, shift), and the CONSUMER applies scale/shift/ReLU
    while loading its operand -- conv -> BN -> ReLU costs one write and one read.
  * frozen BatchNorm (a module in eval mode with running statistics, decided per module as nn.BatchNorm2d.forward does):
    the site's vectors come from the running statistics (nothing is accumulated or updated), and its backward is ONE
    pass, g_c = scale*g_y, with dgamma / dbeta summed on the side (UBR_PASS_FROZEN of ubr_bn_bwd and ubr_block_tail_bwd).
  * backward is scheduled by hand in reverse order; parameter gradients land in one flat fp32
    buffer laid out in completion order so data-parallel all-reduce can start per stage.
"""
from __future__ import annotations

import os
import struct
from typing import Callable, Dict, List, Optional

import torch

from . import _lib as L
from . import ops
from .ops import Affine

T3 = ops.conv_taps(3, 1, 1)
T1 = ops.conv_taps(1, 1, 0)
T7 = ops.conv_taps(7, 1, 3)
DG3 = ops.conv_dgrad_taps_s1(3, 1, 1)
DG1 = ops.conv_dgrad_taps_s1(1, 1, 0)
DG7 = ops.conv_dgrad_taps_s1(7, 1, 3)


# UBR_INFER_FOLD=0: eval forward on the training schedule (BatchNorm applied on load, separate block tails) -- for A/B tests
_INFER_FOLD = os.environ.get("UBR_INFER_FOLD", "1") != "0"
# BatchNorm-backward finalize fused into the apply pass (every workgroup re-sums the reduce pass's 8 stripes) up to this many
# channels.  Measured: isolated, the fused apply costs +0.3 ... +2 us over the plain one at every width (512 channels: 8.7 vs
# 8.4 us) against ~5 us of finalize launch; in the train step 64 vs all widths is within noise -- all widths, for the launches.
_FIN_MAX_C = 1024
# the four output phases of a transposed conv / of a stride-2 conv's data gradient in ONE launch when the layer has at least this
# many output channels (conv_igemm_kernel: a phase per blockIdx.z; conv_thin_kernel, Cin <= 32 without an addend: a phase loop over
# one staged halo)
_PHASE_MIN_C = 16


def wgrad_stream_enabled() -> bool:
    """UBR_WGRAD_STREAM=0 keeps the weight gradients (and the early repack of the backward weight images) on the compute
    stream.  Read per pass, not at import: tests and tools set it around single runs."""
    return os.environ.get("UBR_WGRAD_STREAM", "1") != "0"


def _phased(k, pad):
    """[(ry, rx, taps)] of the non-empty output phases of a stride-2 transposed conv, and their concatenation"""
    ph = [(ry, rx, ops.transposed_phase_taps(k, 1, pad, 2, ry, rx)) for ry in range(2) for rx in range(2)]
    ph = [p for p in ph if p[2]]
    return ph, [t for p in ph for t in p[2]]


_PH4 = _phased(4, 1)
_PH3 = _phased(3, 1)
assert len(_PH4[0]) == 4 and len(_PH3[0]) == 4      # (the one-launch paths below hand all four phases to ops.conv_phases)


def _phase(t, ry, rx):
    """stride-2 phase view of an NHWC tensor"""
    return t[:, ry::2, rx::2, :]


class BNSite:
    """Per-BatchNorm2d runtime vectors (views into the per-pass workspaces)."""
    __slots__ = ("mod", "C", "stats", "scale", "shift", "mean", "invstd", "red", "k1", "k2", "frozen")

    def __init__(self, mod):
        self.mod = mod
        self.C = mod.num_features
        self.frozen = False      # this pass normalises with the running statistics (set per pass, restored for its backward)


def _module_frozen(mod) -> bool:
    """nn.BatchNorm2d.forward hands training=False to F.batch_norm: module in eval mode and running statistics present"""
    return not mod.training and mod.running_mean is not None and mod.running_var is not None


class Saved:
    """What one forward pass keeps for backward."""
    pass


class Engine:
    def __init__(self, model, kind: str):
        self.model = model
        self.kind = kind  # "uresnet" | "aspp"
        self._plans: Dict[tuple, dict] = {}
        self._images: Dict[tuple, torch.Tensor] = {}
        self._const: Dict[tuple, torch.Tensor] = {}
        self.wws = ops.WgradWorkspace()
        self.side = None
        self._side_on = False
        self._evs, self._ev_next, self._main = [], 0, None
        self._red_buf, self._red_off, self._red_elems = None, 0, 0
        self._red_batch = ops.ReduceBatch(self.wws)    # slab sums of the weight gradients issued since the last _wg_flush
        self._fin_pending = []                         # frozen sites whose dgamma / dbeta wait for the next _fin_flush
        self._bwd_packed, self._pack_evs = None, None
        self._rec = None                      # plan being recorded (ubresnet_amd/plan.py)
        self._planned: Dict[tuple, object] = {}
        self.wws.pin = True                   # tapes bake workspace addresses: outgrown slabs stay allocated
        self.bn_sites: List[BNSite] = []
        self._bn_of: Dict[int, BNSite] = {}
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                s = BNSite(m)
                self.bn_sites.append(s)
                self._bn_of[id(m)] = s
        # gradient layout: parameters in the order their gradients complete in backward
        self.grad_order = list(model._grad_completion_order())
        self.grad_offsets = {}
        off = 0
        for name, p in self.grad_order:
            self.grad_offsets[name] = off
            off += (p.numel() + 3) // 4 * 4
        self.grad_numel = off

    # ------------------------------------------------------------------ helpers
    def bn(self, mod) -> BNSite:
        return self._bn_of[id(mod)]

    def any_training(self) -> bool:
        """some BatchNorm of the model would use batch statistics now"""
        return any(not _module_frozen(s.mod) for s in self.bn_sites)

    def frozen_pattern(self, training: bool) -> tuple:
        """per BatchNorm site: frozen in a pass started now.  training = False freezes every site that has running statistics"""
        if training:
            return tuple(_module_frozen(s.mod) for s in self.bn_sites)
        return tuple(s.mod.running_mean is not None and s.mod.running_var is not None for s in self.bn_sites)

    def const(self, device, value: float, n: int) -> torch.Tensor:
        key = (device, value)
        t = self._const.get(key)
        if t is None or t.numel() < n:
            t = torch.full((max(n, 2048),), value, dtype=torch.float32, device=device)
            self._const[key] = t
        return t

    def _new(self, shape, dtype=None, device=None):
        """every per-pass buffer: while a launch plan is being recorded the tensor is pinned to the plan (its device
        address is baked into the tape, and the caching allocator must not hand the block to anything else)"""
        t = torch.empty(shape, dtype=dtype, device=device)
        if self._rec is not None:
            self._rec.keep.append(t)
        return t

    @staticmethod
    def _fresh(shape, dtype=None, device=None):
        """tensors handed to the caller (the log-probabilities): new memory on every pass, planned or not"""
        return torch.empty(shape, dtype=dtype, device=device)

    def _untaped(self, fn):
        """ops whose operands are not owned by the plan (the caller's image, the loss gradient, the fresh output):
        run now, stay off the tape; a replayed pass calls them from Python around the replay"""
        if self._rec is None:
            return fn()
        self._rec.tape.pause()
        try:
            return fn()
        finally:
            self._rec.tape.resume()

    def _fork(self, a, b):
        if self._rec is not None and self._rec.nstreams > 1:
            self._rec.tape.fork(a, b)

    def relu_affine(self, site: BNSite) -> Affine:
        return Affine(site.mean, site.scale, site.shift, self.const(site.scale.device, 0.0, site.C))

    # ------------------------------------------------------------------ weight images
    # Every pass repacks ALL weight images with one batched launch per direction (forward images at the start
    # of forward, data-gradient images at the start of backward).  Nothing is cached across passes: fused
    # optimizers (torch._fused_adam_) update parameters without bumping their version counters, so a cache keyed
    # on `_version` silently trains on stale weights.
    def _plan_items(self):
        """[(group, key, param, src_offset, M, Kvalid, Kpad_or_None, sm, sk, ntaps, tap_stride)]"""
        m = self.model
        items = []
        conv1 = getattr(m, "conv1", None)
        conv11 = getattr(m, "conv11", None)
        for mod in m.modules():
            if isinstance(mod, torch.nn.ConvTranspose2d):
                w = mod.weight
                d0, d1, kh, kw = w.shape
                kk = kh * kw
                items.append(("fwd", (id(w), "tfwd"), w, 0, d1, d0, None, kk, d1 * kk, kk, 1))
                items.append(("bwd", (id(w), "tdgrad"), w, 0, d0, d1, None, d1 * kk, kk, kk, 1))
            elif isinstance(mod, torch.nn.Conv2d):
                w = mod.weight
                d0, d1, kh, kw = w.shape
                kk = kh * kw
                if mod is conv1 and self.kind != "custom":
                    for ci in range(d1):     # stem: packed[ky][kx (7 of 16)][co] = w[co][ci][ky][kx]
                        items.append(("fwd", (id(w), "stem%d" % ci), w, ci * 49, d0, 7, 16, d1 * 49, 1, 7, 7))
                    continue
                items.append(("fwd", (id(w), "fwd"), w, 0, d0, d1, None, d1 * kk, kk, kk, 1))
                if mod is conv11 and self.kind != "custom":   # K (= num_classes) zero-padded to the 16 channels of g_logits
                    items.append(("bwd", (id(w), "dgrad"), w, 0, d1, d0, 16, kk, d1 * kk, kk, 1))
                else:
                    items.append(("bwd", (id(w), "dgrad"), w, 0, d1, d0, None, kk, d1 * kk, kk, 1))
        if self.kind == "custom":             # test harnesses wrap single blocks: a 7x7 stem conv gets stem images too
            for mod in m.modules():
                if isinstance(mod, torch.nn.Conv2d) and mod.kernel_size == (7, 7) and mod.in_channels <= 4:
                    w = mod.weight
                    for ci in range(w.shape[1]):
                        items.append(("fwd", (id(w), "stem%d" % ci), w, ci * 49, w.shape[0], 7, 16, w.shape[1] * 49, 1, 7, 7))
        return items

    def _image_tables(self, dt, device, groups, scale_of=None, slot_of=None):
        """ubr_pack_item tables of this model's weight images -> (images {key: tensor}, {group: table bytes}, {group: items}).
        scale_of: {id(weight): per-output-channel scale folded into its image}; slot_of: {id(weight): preallocated image}"""
        cpu = L.chans_per_unit(dt)
        images, tables, counts = {}, {g: b"" for g in groups}, {g: 0 for g in groups}
        for group, k, w, soff, M, Kv, Kpad, sm, sk, ntaps, tstride in self._plan_items():
            if group not in tables:
                continue
            if not w.is_contiguous() or w.dtype != torch.float32 or w.device != device:
                raise RuntimeError("ubresnet_amd: parameters must be contiguous float32 on %s" % device)
            Mpad = (M + 15) // 16 * 16
            Kp = Kpad if Kpad is not None else (Kv + cpu - 1) // cpu * cpu
            shape = (ntaps, Kp // cpu, Mpad, cpu)
            dst = slot_of.get(id(w)) if slot_of else None
            if dst is None:
                dst = self._new(shape, dtype=dt, device=device)
            elif tuple(dst.shape) != shape:
                raise RuntimeError("ubresnet_amd: ASPP branch image %s does not fit its slot %s" % (shape, tuple(dst.shape)))
            images[k] = dst
            sc = scale_of.get(id(w)) if scale_of else None
            tables[group] += struct.pack("<QQqqqQiiiiii", w.data_ptr() + 4 * soff, dst.data_ptr(), sm, sk, tstride,
                                         sc.data_ptr() if sc is not None else 0, M, Mpad, Kv, Kp // cpu, ntaps, 0)
            counts[group] += 1
        return images, tables, counts

    @staticmethod
    def _device_table(table: bytes, device):
        return torch.frombuffer(bytearray(table), dtype=torch.uint8).to(device)

    def _pack_plan(self, dt, device):
        key = (dt, device)
        plan = self._plans.get(key)
        ptrs = tuple(p.data_ptr() for _, p in self.grad_order)
        if plan is not None and plan["ptrs"] == ptrs:
            return plan
        images, tables, counts = self._image_tables(dt, device, ("fwd", "bwd"))
        plan = {"ptrs": ptrs, "images": images, "counts": counts}
        for g in ("fwd", "bwd"):
            plan[g] = self._device_table(tables[g], device) if counts[g] else None
        self._plans[key] = plan
        return plan

    def pack_all(self, dt, device, group, stream=None):
        plan = self._pack_plan(dt, device)
        if plan["counts"][group]:
            st = L.stream_ptr() if stream is None else stream.cuda_stream
            L.check(L.lib().ubr_pack_weights_batched(L.dtype_id(dt), plan[group].data_ptr(), plan["counts"][group], st),
                    "pack_weights_batched")
        self._images = plan["images"]

    def _pack_bwd_early(self, dt, dev):
        """Training forward: the backward-orientation weight images are not needed before backward starts, so their
        repack runs on the side stream under the forward pass instead of at the head of the backward chain."""
        self._bwd_packed = None
        if dev.type != "cuda" or not wgrad_stream_enabled():
            return
        self._ensure_side(dev)
        if self._pack_evs is None:
            self._pack_evs = (torch.cuda.Event(), torch.cuda.Event())
        e0, e1 = self._pack_evs
        e0.record(torch.cuda.current_stream(dev))      # weights are final and every earlier reader of the images is queued
        self.side.wait_event(e0)
        self._fork(0, 1)
        self.pack_all(dt, dev, "bwd", stream=self.side)
        e1.record(self.side)
        self._bwd_packed = (dt, dev)

    def _pack_bwd(self, dt, dev):
        if self._bwd_packed == (dt, dev):
            torch.cuda.current_stream(dev).wait_event(self._pack_evs[1])
            self._fork(1, 0)
            self._bwd_packed = None
            self._images = self._pack_plan(dt, dev)["images"]
        else:
            self.pack_all(dt, dev, "bwd")

    def packed(self, param: torch.Tensor, orient: str) -> torch.Tensor:
        """packed image of a weight for this pass (written by pack_all)"""
        return self._images[(id(param), orient)]

    def _alloc_pass_workspaces(self, sv: Saved, device, training: bool):
        nf = sum(4 * s.C for s in self.bn_sites)
        sv.fws = self._new(nf, dtype=torch.float32, device=device)
        off = 0
        for s in self.bn_sites:
            s.scale = sv.fws[off:off + s.C]; off += s.C
            s.shift = sv.fws[off:off + s.C]; off += s.C
            s.mean = sv.fws[off:off + s.C]; off += s.C
            s.invstd = sv.fws[off:off + s.C]; off += s.C
        for s, fz in zip(self.bn_sites, self.frozen_pattern(training)):
            s.frozen = fz
        self._snapshot_sites(sv)
        NS = L.STAT_SLOTS
        nd = sum(2 * s.C for s in self.bn_sites if not s.frozen) * NS
        if nd:
            # (frozen sites accumulate no statistics: their producer convs get stats = None)
            sv.dws = self._new(nd, dtype=torch.float64, device=device)
            ops.zero_(sv.dws)
        off = 0
        for s in self.bn_sites:
            if s.frozen:
                s.stats = None
            else:
                s.stats = sv.dws[off:off + 2 * s.C * NS]; off += 2 * s.C * NS

    def _snapshot_sites(self, sv: Saved):
        sv.sites = [(s, s.scale, s.shift, s.mean, s.invstd, s.frozen) for s in self.bn_sites]

    def _rebind(self, sv: Saved):
        """point the BN sites at the vectors (and the mode) of the pass that is being back-propagated"""
        for s, scale, shift, mean, invstd, frozen in sv.sites:
            s.scale, s.shift, s.mean, s.invstd, s.frozen = scale, shift, mean, invstd, frozen

    def _finish_bn(self, site: BNSite, count: int, training: bool):
        m = site.mod
        if training and not site.frozen:
            mom = -1.0 if m.momentum is None else m.momentum     # None: cumulative moving average (factor 1 / num_batches_tracked)
            track = m.track_running_stats and m.running_mean is not None
            ops.bn_finalize(site.stats, count, m.weight, m.bias, m.running_mean if track else None,
                            m.running_var if track else None, m.num_batches_tracked if track else None,
                            mom, m.eps, site.scale, site.shift, site.mean, site.invstd)
        else:
            ops.bn_eval_affine(m.weight, m.bias, m.running_mean, m.running_var, m.eps, site.scale, site.shift, site.mean, site.invstd)

    # ------------------------------------------------------------------ BasicBlock
    def block_fwd(self, blk, x, out, training, dt, xf_in=None):
        """BasicBlock.forward (models/common_layers.py:39-58); x, out: NHWC views.
        xf_in: per-channel affine of a virtual input (only for blocks with a bypass conv)."""
        if xf_in is not None and blk.bypass is None:
            raise RuntimeError("identity-shortcut block cannot take a virtual (affine) input")
        N, H, W, Cin = x.shape
        S = blk.stride
        OH, OW = out.shape[1], out.shape[2]
        Cout = out.shape[3]
        dev = x.device
        bn1, bn2 = self.bn(blk.bn1), self.bn(blk.bn2)
        cnt = N * OH * OW
        c1 = self._new((N, OH, OW, Cout), dtype=dt, device=dev)
        ops.conv(x, self.packed(blk.conv1.weight, "fwd"), c1, T3, Cout, S=S, xf=xf_in, stats=bn1.stats)
        self._finish_bn(bn1, cnt, training)
        c2 = self._new((N, OH, OW, Cout), dtype=dt, device=dev)
        bnb = self.bn(blk.bnpass) if blk.bypass is not None else None
        # (a frozen site has nothing to finalise: a tail with one takes the plain tail kernel and per-site finish launches)
        fuse = training and not bn2.frozen and not (bnb is not None and bnb.frozen) and 24 * Cout <= 65536
        slots = L.RED_SLOTS if fuse else 0
        ops.conv(c1, self.packed(blk.conv2.weight, "fwd"), c2, T3, Cout, xf=self.relu_affine(bn1), stats=bn2.stats, stats_slots=slots)
        if not fuse:
            self._finish_bn(bn2, cnt, training)
        cb = None
        if blk.bypass is not None:
            cb = self._new((N, OH, OW, Cout), dtype=dt, device=dev)
            ops.conv(x, self.packed(blk.bypass.weight, "fwd"), cb, T1, Cout, S=S, xf=xf_in, stats=bnb.stats, stats_slots=slots)
            if not fuse:
                self._finish_bn(bnb, cnt, training)
        # the final ReLU's mask as one byte per 16-byte channel unit: the backward's two passes read it instead of `out`
        mask = None
        if self._save:
            mask = self._new((cnt * (Cout // L.chans_per_unit(dt)),), dtype=torch.uint8, device=dev)
        if fuse:
            f2 = ops.bn_fwd_fin(bn2.stats, blk.bn2, bn2.scale, bn2.shift, bn2.mean, bn2.invstd)
            fb = ops.bn_fwd_fin(bnb.stats, blk.bnpass, bnb.scale, bnb.shift, bnb.mean, bnb.invstd) if blk.bypass is not None else None
            ops.block_tail_fwd_fin(c2, f2, cb if blk.bypass is not None else x, fb, cnt, out, relu_mask=mask)
        elif blk.bypass is not None:
            ops.block_tail_fwd(c2, bn2.mean, bn2.scale, bn2.shift, cb, bnb.mean, bnb.scale, bnb.shift, out, relu_mask=mask)
        else:
            ops.block_tail_fwd(c2, bn2.mean, bn2.scale, bn2.shift, x, None, None, None, out, relu_mask=mask)
        if not self._save:
            return None
        rec = Saved()
        rec.blk, rec.x, rec.c1, rec.c2, rec.cb, rec.out, rec.xf_in = blk, x, c1, c2, cb, out, xf_in
        rec.mask = mask
        return rec

    # ------------------------------------------------------------------ backward reduction arena
    def _red_begin(self, dev):
        """one zeroed fp64 arena per backward pass for every striped reduction buffer (one memset instead of ~45)"""
        if self._red_elems == 0:
            NS = L.STAT_SLOTS
            tot = 0
            for s_ in self.bn_sites:
                tot += 2 * s_.C * NS
            self._red_elems = 2 * tot + 64 * NS * 8      # BN sites (block tails take 2 sites' worth) + head/stem/bias sums
        self._red_buf = self._new(self._red_elems, dtype=torch.float64, device=dev)
        ops.zero_(self._red_buf)
        self._red_off = 0

    def _red(self, n, dev):
        k = L.STAT_SLOTS * n
        if self._red_buf is None or self._red_off + k > self._red_buf.numel() or self._red_buf.device != dev:
            t = ops.stat_buffer(n, dev)             # outside a backward pass, or arena exhausted
            if self._rec is not None:
                self._rec.keep.append(t)
            return t
        t = self._red_buf[self._red_off:self._red_off + k]
        self._red_off += k
        return t

    # ------------------------------------------------------------------ weight-gradient side stream
    def _side_begin(self, dev):
        """Weight gradients depend on nothing downstream, so they run on a second HIP stream next to the
        dgrad / BatchNorm-backward chain: the low-resolution layers launch too few workgroups to fill 256 CUs
        on their own.  UBR_WGRAD_STREAM=0 serialises everything on one stream (clean per-kernel timings); the
        launch profiler otherwise times kernels under the same two-stream contention as the real step (and as
        rocprofv3 sees them)."""
        self._side_on = dev.type == "cuda" and wgrad_stream_enabled()
        if self._side_on:
            self._ensure_side(dev)
            self._main = torch.cuda.current_stream(dev)
            self._ev_next = 0

    def _ensure_side(self, dev):
        if self.side is not None:
            return
        # HIP maps normal-priority streams round-robin onto a few hardware queues; once RCCL has created its own
        # streams the side stream can land on the compute stream's queue and the two serialise (measured under
        # torchrun: 17.7 instead of 15.1 ms/step).  High-priority streams use separate queues, so in a
        # process-group job the side stream is created with high priority (costs 0.2 ms/step standalone).
        import torch.distributed as _dist
        in_job = _dist.is_available() and _dist.is_initialized()
        prio = int(os.environ.get("UBR_SIDE_PRIORITY", "-1" if in_job else "0"))
        self.side = torch.cuda.Stream(device=dev, priority=prio)

    def _wg_flush(self):
        """one launch for the slab sums of every weight gradient issued since the last flush (ops.ReduceBatch)"""
        self._red_batch.flush()

    def _fin_flush(self):
        """dgamma / dbeta of the frozen sites back-propagated since the last flush.  Their data gradients did not wait for
        the sums, so these launches sit at the end of a stage, behind the convs, instead of between a BatchNorm backward
        and its consumer."""
        for red, site, G in self._fin_pending:
            ops.bn_bwd_finalize_frozen(red, site.C, G(site.mod.weight), G(site.mod.bias))
        del self._fin_pending[:]

    def _fin_later(self, red, site, G):
        self._fin_pending.append((red, site, G))

    def _side_end(self, dev):
        self._fin_flush()
        self._wg_flush()
        if self._side_on:
            torch.cuda.current_stream(dev).wait_stream(self.side)
            self._fork(1, 0)
            self._side_on = False

    def _wg(self, x, g, *args, **kw):
        """weight gradient of one conv; its slab sum is deferred to the stage's _wg_flush"""
        kw["defer"] = self._red_batch
        if not self._side_on:
            return ops.wgrad(x, g, *args, **kw)
        # side stream waits for everything queued on the compute stream so far (x and g are produced there); the
        # launch goes straight to the side stream's handle -- no stream-context switch, one pooled event per call
        ev = self._event()
        ev.record(self._main)
        self.side.wait_event(ev)
        self._fork(0, 1)
        ops.wgrad(x, g, *args, stream=self.side, **kw)
        # the caching allocator must not hand these blocks to later main-stream kernels while the side stream reads them
        x.record_stream(self.side)
        g.record_stream(self.side)

    def _event(self):
        i = self._ev_next
        if i == len(self._evs):
            self._evs.append(torch.cuda.Event())
        self._ev_next = i + 1
        return self._evs[i]

    def _bn_bwd(self, site: BNSite, ga, ga2, c, relu, G, cnt):
        """backward through a = relu(bn(c)) (or bn only): returns g_c; writes dgamma/dbeta."""
        red = self._red(2 * site.C, c.device)
        if site.frozen:
            gc = self._new(c.shape, dtype=c.dtype, device=c.device)
            ops.bn_bwd_frozen(ga, ga2, c, site.scale, site.shift, site.mean, site.invstd, relu, red, gc)
            self._fin_later(red, site, G)
            return gc
        ops.bn_bwd_reduce(ga, ga2, c, site.scale, site.shift, site.mean, site.invstd, relu, red)
        gc = self._new(c.shape, dtype=c.dtype, device=c.device)
        if site.C <= _FIN_MAX_C:
            ops.bn_bwd_apply_fin(ga, ga2, c, site.scale, site.shift, site.mean, site.invstd, relu, red, cnt,
                                 G(site.mod.weight), G(site.mod.bias), gc)
            return gc
        k = self._new(2 * site.C, dtype=torch.float32, device=c.device)
        k1, k2 = k[:site.C], k[site.C:]
        ops.bn_bwd_finalize(red, cnt, site.C, G(site.mod.weight), G(site.mod.bias), False, k1, k2)
        ops.bn_bwd_apply(ga, ga2, c, site.scale, site.shift, site.mean, site.invstd, relu, k1, k2, gc)
        return gc

    def _conv_dgrad(self, conv_mod, g, gx, S, addend=None, k=3, addend_mask=None):
        """data gradient of Conv2d(k, stride S, pad k//2): g (conv output grad) -> gx (input grad view)"""
        dt = g.dtype
        wp = self.packed(conv_mod.weight, "dgrad")
        Cin = gx.shape[3]
        pad = k // 2
        if S == 1:
            taps = DG3 if k == 3 else (DG1 if k == 1 else DG7)
            ops.conv(g, wp, gx, taps, Cin, addend=addend, addend_mask=addend_mask)
        else:
            if k == 3 and Cin >= _PHASE_MIN_C and addend_mask is None:
                ops.conv_phases(g, wp, _phase(gx, 0, 0), _PH3[1], Cin, phases=_PH3[0], y_full=gx, addend_full=addend)
                return
            for ry in range(2):
                for rx in range(2):
                    taps = ops.transposed_phase_taps(k, 1, pad, 2, ry, rx)
                    if not taps:
                        continue   # (1x1 stride-2: only phase (0,0) receives gradient; addend already in place)
                    yv = _phase(gx, ry, rx)
                    av = _phase(addend, ry, rx) if addend is not None else None
                    ops.conv(g, wp, yv, taps, Cin, addend=av)

    def block_bwd(self, rec, go, go2, G, need_gx=True):
        """backward of BasicBlock; go (+go2): gradient wrt the block output. Returns g_x (or None)."""
        blk, x, c1, c2, cb, out = rec.blk, rec.x, rec.c1, rec.c2, rec.cb, rec.out
        dt, dev = c2.dtype, c2.device
        N, OH, OW, Cout = c2.shape
        cnt = N * OH * OW
        S = blk.stride
        bn1, bn2 = self.bn(blk.bn1), self.bn(blk.bn2)
        byp = cb is not None
        bnb = self.bn(blk.bnpass) if byp else None
        NS = L.STAT_SLOTS
        red = self._red((4 if byp else 2) * Cout, dev)
        red2 = red[:2 * Cout * NS]
        redb = red[2 * Cout * NS:] if byp else None
        mask = rec.mask         # (the final ReLU's bit mask: block_fwd keeps one whenever it keeps a record)
        # every site of the tail frozen: one pass (no sum stands between go and the data gradients); sites in different modes:
        # the two passes, with k1 = k2 = 0 for the frozen site
        nfrozen = int(bn2.frozen) + int(byp and bnb.frozen)
        onepass = nfrozen == (2 if byp else 1)
        fin = Cout <= _FIN_MAX_C and nfrozen == 0
        if not onepass:
            ops.block_tail_bwd_reduce(go, go2, out, c2, bn2.scale, bn2.shift, bn2.mean, bn2.invstd,
                                      cb, bnb.mean if byp else None, bnb.invstd if byp else None, red2, redb, relu_mask=mask)
        g_c2 = self._new(c2.shape, dtype=dt, device=dev)
        # identity block with one gradient operand: the skip gradient go*[out>0] is not written; conv1's data-gradient epilogue
        # re-forms it from go and the bit mask
        lazy_sc = not byp and go2 is None and need_gx and (fin or onepass)
        g_sc = None if lazy_sc else self._new(c2.shape, dtype=dt, device=dev)
        if onepass:
            ops.block_tail_bwd_frozen(go, go2, mask, c2, bn2.scale, bn2.shift, bn2.mean, bn2.invstd, red2,
                                      cb, bnb.scale if byp else None, bnb.mean if byp else None, bnb.invstd if byp else None, redb, g_c2, g_sc)
            self._fin_later(red2, bn2, G)
            if byp:
                self._fin_later(redb, bnb, G)
        elif fin:
            ops.block_tail_bwd_apply_fin(go, go2, mask, c2, bn2.scale, bn2.shift, bn2.mean, bn2.invstd, red2, G(blk.bn2.weight), G(blk.bn2.bias),
                                         cb, bnb.scale if byp else None, bnb.mean if byp else None, bnb.invstd if byp else None,
                                         redb, G(blk.bnpass.weight) if byp else None, G(blk.bnpass.bias) if byp else None, cnt, g_c2, g_sc)
        else:
            k = self._new(4 * Cout, dtype=torch.float32, device=dev)
            if bn2.frozen:
                ops.bn_bwd_finalize_frozen(red2, Cout, G(blk.bn2.weight), G(blk.bn2.bias), k[:Cout], k[Cout:2 * Cout])
            else:
                ops.bn_bwd_finalize(red2, cnt, Cout, G(blk.bn2.weight), G(blk.bn2.bias), False, k[:Cout], k[Cout:2 * Cout])
            if byp and bnb.frozen:
                ops.bn_bwd_finalize_frozen(redb, Cout, G(blk.bnpass.weight), G(blk.bnpass.bias), k[2 * Cout:3 * Cout], k[3 * Cout:])
            elif byp:
                ops.bn_bwd_finalize(redb, cnt, Cout, G(blk.bnpass.weight), G(blk.bnpass.bias), False, k[2 * Cout:3 * Cout], k[3 * Cout:])
            ops.block_tail_bwd_apply(go, go2, out, c2, bn2.scale, bn2.shift, bn2.mean, bn2.invstd, k[:Cout], k[Cout:2 * Cout],
                                     cb, bnb.scale if byp else None, bnb.mean if byp else None, bnb.invstd if byp else None,
                                     k[2 * Cout:3 * Cout] if byp else None, k[3 * Cout:] if byp else None, g_c2, g_sc, relu_mask=mask)
        # conv2: weight grad (input = relu(bn1(c1)) re-formed on load) and data grad.  Every weight gradient is issued BEFORE the
        # data-gradient conv that shares its gradient operand: on the side stream it then starts earliest
        kk = 9
        self._wg(c1, g_c2, T3, G(blk.conv2.weight), Cout * kk, kk, Cout, Cout, self.wws, xf=self.relu_affine(bn1))
        g_a1 = self._new(c1.shape, dtype=dt, device=dev)
        self._conv_dgrad(blk.conv2, g_c2, g_a1, 1)
        del g_c2
        g_c1 = self._bn_bwd(bn1, g_a1, None, c1, True, G, cnt)
        del g_a1
        Cin = x.shape[3]
        self._wg(x, g_c1, T3, G(blk.conv1.weight), Cin * kk, kk, Cout, Cin, self.wws, S=S, xf=rec.xf_in)
        if byp:
            self._wg(x, g_sc, T1, G(blk.bypass.weight), Cin, 1, Cout, Cin, self.wws, S=S, xf=rec.xf_in)
        if not need_gx:
            return None
        gx = self._new(x.shape, dtype=dt, device=dev)
        if byp:
            self._conv_dgrad(blk.conv1, g_c1, gx, S)
            self._conv_dgrad(blk.bypass, g_sc, gx, S, addend=gx, k=1)
        elif lazy_sc:
            self._conv_dgrad(blk.conv1, g_c1, gx, S, addend=go, addend_mask=mask)
        else:
            self._conv_dgrad(blk.conv1, g_c1, gx, S, addend=g_sc)
        return gx

    # ------------------------------------------------------------------ DoubleResNet
    def double_fwd(self, dbl, x, out, training, dt, xf_in=None):
        N, H, W, _ = x.shape
        S = dbl.res1.stride
        mid = self._new((N, out.shape[1], out.shape[2], out.shape[3]), dtype=dt, device=x.device)
        r1 = self.block_fwd(dbl.res1, x, mid, training, dt, xf_in)
        r2 = self.block_fwd(dbl.res2, mid, out, training, dt)
        return (r1, r2) if self._save else None

    def double_bwd(self, recs, go, go2, G, need_gx=True):
        r1, r2 = recs
        g_mid = self.block_bwd(r2, go, go2, G)
        return self.block_bwd(r1, g_mid, None, G, need_gx)

    # ------------------------------------------------------------------ ConvTransposeLayer
    def deconv_fwd(self, dl, x, cat, Cd, dt, xf_x=None):
        """ConvTranspose2d(k4,s2,p1) of x into channels [0,Cd) of the concat buffer (4 output phases)."""
        wp = self.packed(dl.deconv.weight, "tfwd")
        up = cat[..., :Cd]
        if Cd >= _PHASE_MIN_C:
            ops.conv_phases(x, wp, _phase(up, 0, 0), _PH4[1], Cd, phases=_PH4[0], y_full=up, xf=xf_x)
            return
        for ry in range(2):
            for rx in range(2):
                ops.conv(x, wp, _phase(up, ry, rx), ops.transposed_phase_taps(4, 1, 1, 2, ry, rx), Cd, xf=xf_x)

    def declayer_fwd(self, dl, x, cat, Cd, out, training, dt, xf_x=None, xf_cat=None):
        """ConvTransposeLayer.forward (models/common_layers.py:127-132); the skip half of `cat` is already filled.
        xf_x / xf_cat: affines of a virtual deconv input / virtual skip channels (ASPP_ResNet)."""
        self.deconv_fwd(dl, x, cat, Cd, dt, xf_x)
        recs = self.double_fwd(dl.res, cat, out, training, dt, xf_cat)
        if not self._save:
            return None
        rec = Saved()
        rec.dl, rec.x, rec.cat, rec.Cd, rec.recs, rec.xf_x = dl, x, cat, Cd, recs, xf_x
        return rec

    def declayer_bwd(self, rec, go, G, xf_x: Optional[Affine] = None):
        """returns (g_x, g_cat); g_cat[..., Cd:] is the gradient of the skip tensor (w.r.t. the transformed
        values when the layer was given affines)"""
        dl, x, cat, Cd = rec.dl, rec.x, rec.cat, rec.Cd
        xf_x = rec.xf_x if xf_x is None else xf_x
        g_cat = self.double_bwd(rec.recs, go, None, G)
        g_up = g_cat[..., :Cd]
        Cin = x.shape[3]
        dW = G(dl.deconv.weight)
        for ry in range(2):
            for rx in range(2):
                taps = ops.transposed_phase_taps(4, 1, 1, 2, ry, rx)
                self._wg(x, _phase(g_up, ry, rx), taps, dW, 16, Cd * 16, Cd, Cin, self.wws, xf=xf_x)
        # data gradient of the transposed conv = ordinary stride-2 conv over g_up
        gx = self._new(x.shape, dtype=x.dtype, device=x.device)
        wp = self.packed(dl.deconv.weight, "tdgrad")
        ops.conv(g_up, wp, gx, ops.conv_taps(4, 1, 1), Cin, S=2)
        return gx, g_cat

    # ------------------------------------------------------------------ stem
    STEM_TAPS = [(ky - 3, 0, ky) for ky in range(7)]

    def stem_fwd(self, conv1, x, c0, stats, dt):
        """conv1 7x7 on the caller's NCHW image (models/ub_uresnet.py:41,94) on the matrix cores: the image is
        expanded to 16 channels per plane (column shifts -3..3), then each plane is a 7-tap vertical conv."""
        N, Cin, H, W = x.shape
        Cout = conv1.out_channels
        x16 = self._new((N, H, W, 16 * Cin), dtype=dt, device=x.device)
        self._untaped(lambda: ops.stem_expand(x, x16))
        if self._rec is not None:
            self._rec.pre = lambda xx: ops.stem_expand(xx, x16)
        w = conv1.weight
        for ci in range(Cin):
            last = ci == Cin - 1
            ops.conv(x16[..., 16 * ci:16 * ci + 16], self.packed(w, "stem%d" % ci), c0, self.STEM_TAPS, Cout,
                     bias=conv1.bias if ci == 0 else None, addend=c0 if ci > 0 else None, stats=stats if last else None)
        return x16

    def stem_bwd(self, conv1, x16, g_c0, G):
        Cout = conv1.out_channels
        Cin = x16.shape[3] // 16
        dW = G(conv1.weight)
        taps = [(ky - 3, 0, 7 * ky) for ky in range(7)]
        for ci in range(Cin):
            # the last launch(es) of a backward pass: the compute stream has nothing left to run beside them
            self._wg(x16[..., 16 * ci:16 * ci + 16], g_c0, taps, dW, Cin * 49, 1, Cout, 7, self.wws, dst_offset=ci * 49, exclusive=True)
        red = self._red(Cout, g_c0.device)
        ops.channel_sum(g_c0, red)
        ops.cast_f64_to_f32(red, G(conv1.bias), Cout)


    # ------------------------------------------------------------------ head
    def head_fwd(self, m, d1o, training, dt, sv):
        """conv10 + bias -> bn10 -> relu -> conv11 + bias -> log-softmax (fused epilogue, NCHW fp32)"""
        N, H, W, _ = d1o.shape
        bn10 = self.bn(m.bn10)
        nk = m.conv10.out_channels
        c10 = self._new((N, H, W, nk), dtype=dt, device=d1o.device)
        ops.conv(d1o, self.packed(m.conv10.weight, "fwd"), c10, T7, nk, bias=m.conv10.bias, stats=bn10.stats)
        self._finish_bn(bn10, N * H * W, training)
        ncls = m.conv11.out_channels
        out = self._final_logsoftmax(m, c10, self.packed(m.conv11.weight, "fwd"), self.relu_affine(bn10), (N, ncls, H, W))
        sv.d1o, sv.c10, sv.out, sv.dt = d1o, c10, out.detach(), dt     # (an alias without grad_fn: autograd attaches the node to `out` itself, and node -> ctx -> sv -> out would be a cycle)
        return out

    def head_bwd(self, m, sv, g_logp, G):
        dt, dev = sv.dt, sv.x.device
        N, ncls, H, W = sv.out.shape
        ip = m.conv10.in_channels
        if not g_logp.is_contiguous():
            g_logp = g_logp.contiguous()
        g_l = self._new((N, H, W, 16), dtype=dt, device=dev)
        self._logsoftmax_bwd(g_logp, sv.out, g_l)
        bn10 = self.bn(m.bn10)
        nk = m.conv10.out_channels
        self._wg(sv.c10, g_l, T7, G(m.conv11.weight), nk * 49, 49, ncls, nk, self.wws, xf=self.relu_affine(bn10))
        NS = L.STAT_SLOTS
        red = self._red(16 + nk, dev)
        ops.channel_sum(g_l, red[:16 * NS])
        ops.cast_f64_to_f32(red[:16 * NS], G(m.conv11.bias), ncls, stride=16)
        g_a10 = self._new((N, H, W, nk), dtype=dt, device=dev)
        # data gradient of conv11: K = the 16 (zero-padded) logit channels
        ops.conv(g_l, self.packed(m.conv11.weight, "dgrad"), g_a10, DG7, nk)
        del g_l
        g_c10 = self._bn_bwd(bn10, g_a10, None, sv.c10, True, G, N * H * W)
        del g_a10
        self._wg(sv.d1o, g_c10, T7, G(m.conv10.weight), ip * 49, 49, nk, ip, self.wws)
        ops.channel_sum(g_c10, red[16 * NS:])
        ops.cast_f64_to_f32(red[16 * NS:], G(m.conv10.bias), nk)
        g = self._new(sv.d1o.shape, dtype=dt, device=dev)
        self._conv_dgrad(m.conv10, g_c10, g, 1, k=7)
        return g

    def _final_logsoftmax(self, m, c10, wp, xf, shape):
        """conv11 + bias + LogSoftmax (models/ub_uresnet.py:64,143) into a NEW fp32 NCHW tensor: the one forward op that is
        never taped, so callers get fresh memory from every pass"""
        def head():
            out = self._fresh(shape, dtype=torch.float32, device=c10.device)
            ops.conv(c10, wp, out, T7, shape[1], xf=xf, bias=m.conv11.bias, logsoftmax=True)
            return out
        if self._rec is not None:
            self._rec.post = head
        return self._untaped(head)

    def _logsoftmax_bwd(self, g_logp, out, g_l):
        """first op of backward; reads the loss gradient and the log-probabilities of THIS pass (caller-owned): never taped"""
        self._untaped(lambda: ops.logsoftmax_bwd(g_logp, out, g_l))
        if self._rec is not None:
            self._rec.pre = lambda g, o: ops.logsoftmax_bwd(g, o, g_l)

    def _check_input(self, x, cin):
        L.require_cuda(x, "input")
        if x.dtype != torch.float32:
            raise RuntimeError("ubresnet_amd: input must be float32 NCHW (got %s)" % x.dtype)
        if x.dim() != 4 or x.shape[1] != cin:
            raise RuntimeError("ubresnet_amd: expected input [B,%d,H,W], got %s" % (cin, tuple(x.shape)))
        if x.shape[2] % 32 or x.shape[3] % 32:
            raise RuntimeError("ubresnet_amd: H and W must be multiples of 32 (ConvTranspose2d output_size contract of the "
                               "reference, models/common_layers.py:128); got %dx%d" % (x.shape[2], x.shape[3]))
        return x if x.is_contiguous() else x.contiguous()

    def _grad_views(self, dev):
        flat = self._new(self.grad_numel, dtype=torch.float32, device=dev)
        views = {}
        for name, p in self.grad_order:
            o = self.grad_offsets[name]
            n = p.numel()
            views[id(p)] = flat[o:o + n].view(p.shape)
            if n % 4:       # padding up to the next 16-byte boundary (conv11.bias of a 3-class net): defined, for flat optimizers
                flat[o + n:o + (n + 3) // 4 * 4].zero_()
        return flat, views

    def _stage_notifier(self, flat, grad_ready):
        done = [0]
        ids = [id(p) for _, p in self.grad_order]

        def stage_done(last_param):
            self._fin_flush()
            self._wg_flush()         # the stage's weight gradients are final only after their (batched) slab sums
            i = ids.index(id(last_param))
            hi = self.grad_offsets[self.grad_order[i][0]] + (self.grad_order[i][1].numel() + 3) // 4 * 4
            if self._rec is not None and hi > done[0]:
                # a replayed backward hands flat[done:hi] to the data-parallel reducer through these tape events
                m0 = self._rec.tape.mark(0)
                m1 = self._rec.tape.mark(1) if (self._side_on and self._rec.nstreams > 1) else None
                self._rec.stages.append((done[0], hi, m0, m1))
            if grad_ready is None:
                if hi > done[0]:
                    done[0] = hi
                return
            if hi > done[0]:
                if self._side_on:
                    # flat[done:hi] is final once BOTH streams reach this point: the consumer is told to wait for the
                    # side stream's event as well (neither producer stream stalls for the exchange)
                    ev = self._event()
                    ev.record(self.side)
                    grad_ready(flat, done[0], hi, wait_events=(ev,))
                else:
                    grad_ready(flat, done[0], hi)
                done[0] = hi
        return stage_done

    # ------------------------------------------------------------------ ASPP levels (models/ASPP_ResNet.py:227-286)
    def _affine_arena(self, sv, device, sizes, relu_ranges):
        """per-pass [4][T] float arena of per-channel affines: identity (sub 0, scale 1, shift 0, lo -inf) except
        lo = 0 on `relu_ranges` (where BatchNorm+ReLU sites will be bound).  One template copy per pass."""
        T = sum(sizes)
        key = (device, tuple(sizes), tuple(relu_ranges))
        tmpl = self._const.get(key)
        if tmpl is None:
            tmpl = torch.zeros((4, T), dtype=torch.float32, device=device)
            tmpl[1].fill_(1.0)
            tmpl[3].fill_(ops.NEG_BIG)
            for lo, hi in relu_ranges:
                tmpl[3, lo:hi].zero_()
            self._const[key] = tmpl
        arena = self._new(tmpl.shape, dtype=tmpl.dtype, device=tmpl.device)
        arena.copy_(tmpl)
        sv.arena = arena
        offs, o = [], 0
        for n in sizes:
            offs.append(o)
            o += n
        return arena, offs

    def _bind_site(self, site, arena, off):
        """BatchNorm+ReLU site whose vectors live at arena[:, off:off+C]"""
        Cn = site.C
        site.mean, site.scale, site.shift = arena[0, off:off + Cn], arena[1, off:off + Cn], arena[2, off:off + Cn]

    def _arena_affine(self, arena, off, n):
        return Affine(arena[0, off:off + n], arena[1, off:off + n], arena[2, off:off + n], arena[3, off:off + n])

    def aspp_level_fwd(self, layer, post, e, cpost, arena, off_acat, training, dt):
        """ASPP.forward + ASPP_post.forward (models/ASPP_ResNet.py:227-263,280-286).  e: encoder output view
        [N,h,w,C]; cpost: destination view of the RAW 1x1 output (its BN+ReLU is folded into consumers)."""
        N, h, w, Cn = e.shape
        acat = self._new((N, h, w, 64 + Cn), dtype=dt, device=e.device)
        cnt = N * h * w
        for b, (conv, bn, k, dil) in enumerate(layer.branches()):
            site = self.bn(bn)
            ops.conv(e, self.packed(conv.weight, "fwd"), acat[..., 16 * b:16 * b + 16], ops.conv_taps(k, dil, dil * (k // 2)),
                     16, bias=conv.bias, stats=site.stats)
            self._finish_bn(site, cnt, training)
        ops.maxpool_fwd(e, None, acat[..., 64:], None, 1)
        psite = self.bn(post.ASPP_bn)
        xf = self._arena_affine(arena, off_acat, 64 + Cn)
        ops.conv(acat, self.packed(post.ASPP_conv.weight, "fwd"), cpost, T1, Cn, xf=xf, bias=post.ASPP_conv.bias, stats=psite.stats)
        self._finish_bn(psite, cnt, training)
        if not self._save:
            return None
        rec = Saved()
        rec.layer, rec.post, rec.e, rec.cpost, rec.acat, rec.xf = layer, post, e, cpost, acat, xf
        return rec

    def aspp_level_bwd(self, rec, g_post, g_base, G):
        """g_post: gradient w.r.t. relu(bn(cpost)) (a slice of the consumer's input gradient); g_base: gradient
        already owed to e through the direct skip (accumulated into the result).  Returns the ASPP's total g_e."""
        layer, post, e, cpost, acat = rec.layer, rec.post, rec.e, rec.cpost, rec.acat
        N, h, w, Cn = e.shape
        dt, dev, cnt = e.dtype, e.device, N * h * w
        psite = self.bn(post.ASPP_bn)
        g_cpost = self._bn_bwd(psite, g_post, None, cpost, True, G, cnt)
        self._wg(acat, g_cpost, T1, G(post.ASPP_conv.weight), 64 + Cn, 1, Cn, 64 + Cn, self.wws, xf=rec.xf)
        red = self._red(Cn, dev)
        ops.channel_sum(g_cpost, red)
        ops.cast_f64_to_f32(red, G(post.ASPP_conv.bias), Cn)
        g_acat = self._new(acat.shape, dtype=dt, device=dev)
        ops.conv(g_cpost, self.packed(post.ASPP_conv.weight, "dgrad"), g_acat, DG1, 64 + Cn)
        del g_cpost
        g_e = self._new(e.shape, dtype=dt, device=dev)
        ops.maxpool_bwd(e, None, g_acat[..., 64:], g_base, g_e, 1)
        for b, (conv, bn, k, dil) in enumerate(layer.branches()):
            site = self.bn(bn)
            g_cb = self._bn_bwd(site, g_acat[..., 16 * b:16 * b + 16], None, acat[..., 16 * b:16 * b + 16], True, G, cnt)
            kk = k * k
            taps = ops.conv_taps(k, dil, dil * (k // 2))
            self._wg(e, g_cb, taps, G(conv.weight), Cn * kk, kk, 16, Cn, self.wws)
            redb = self._red(16, dev)
            ops.channel_sum(g_cb, redb)
            ops.cast_f64_to_f32(redb, G(conv.bias), 16)
            ops.conv(g_cb, self.packed(conv.weight, "dgrad"), g_e, ops.conv_dgrad_taps_s1(k, dil, dil * (k // 2)), Cn, addend=g_e)
        return g_e

    # ------------------------------------------------------------------ stages of a pass (shared by both networks)
    # uresnet_* and aspp_* below are a buffer layout plus calls to these.  What differs between the networks arrives as
    # arguments: the concat buffers [deconv | ASPP_post | skip], the bottom tensor, the input affines of dec_layer5 /
    # dec_layer4, and in backward the gradient each encoder level is owed beside the chain's.
    def _forward_begin(self, x, training, dt, save):
        self._save = save
        x = self._check_input(x, self.model.conv1.in_channels)
        sv = Saved()
        self._alloc_pass_workspaces(sv, x.device, training)
        self.pack_all(dt, x.device, "fwd")
        if save:
            self._pack_bwd_early(dt, x.device)
        return x, sv

    def _concat_buffers(self, x, dt, widths):
        """cat1 .. cat5, the decoder levels' input buffers: level i at 1 / 2^(i-1) of the input resolution"""
        N, _, H, W = x.shape
        return [self._new((N, H >> i, W >> i, c), dtype=dt, device=x.device) for i, c in enumerate(widths)]

    def stem_pool_fwd(self, m, x, cat1, training, dt, sv):
        """conv1 -> (bn1 + relu folded into consumers) -> pool; x0 goes into the skip half of dec_layer1's concat buffer"""
        N, _, H, W = x.shape
        ip, dev = m.inplanes, x.device
        bn1 = self.bn(m.bn1)
        c0 = self._new((N, H, W, ip), dtype=dt, device=dev)
        x16 = self.stem_fwd(m.conv1, x, c0, bn1.stats, dt)
        self._finish_bn(bn1, N * H * W, training)
        p0 = self._new((N, H // 2, W // 2, ip), dtype=dt, device=dev)
        amax = self._new((N, H // 2, W // 2, ip), dtype=torch.uint8, device=dev) if self._save else None   # window arg-max for the backward
        ops.maxpool_fwd(c0, self.relu_affine(bn1), p0, cat1[..., ip:], 2, argmax=amax)
        sv.x, sv.x16, sv.c0, sv.amax = x, x16, c0, amax
        return p0

    def stem_pool_bwd(self, m, sv, g_p0, g_x0, G):
        """g_p0: gradient of the pooled tensor; g_x0: gradient the skip connection into dec_layer1 owes relu(bn1(c0))"""
        bn1 = self.bn(m.bn1)
        N, H, W, _ = sv.c0.shape
        g_a0 = self._new(sv.c0.shape, dtype=sv.dt, device=sv.c0.device)
        ops.maxpool_bwd(sv.c0, self.relu_affine(bn1), g_p0, g_x0, g_a0, 2, argmax=sv.amax)
        g_c0 = self._bn_bwd(bn1, g_a0, None, sv.c0, True, G, N * H * W)
        self.stem_bwd(m.conv1, sv.x16, g_c0, G)

    def encoder_fwd(self, m, x, outs, training, dt):
        """enc_layer1 .. enc_layer5; outs: each level's output view (the skip channels of the next decoder level's concat buffer)"""
        recs = []
        for i, out in enumerate(outs, 1):
            recs.append(self.double_fwd(getattr(m, "enc_layer%d" % i), x, out, training, dt))
            x = out
        return tuple(recs)

    def encoder_bwd(self, m, sv, g, owed, G, stage_done):
        """g: gradient of enc_layer5's output.  owed[i - 1]: what the output of level i is owed beside the chain's gradient --
        None, a tensor (a concat buffer's skip channels), or a callable that issues the launches producing it right before
        the level's own (an ASPP level's backward)"""
        for i in (5, 4, 3, 2, 1):
            g2 = owed[i - 1]() if callable(owed[i - 1]) else owed[i - 1]
            g = self.double_bwd(sv.enc[i - 1], g, g2, G); stage_done(getattr(m, "enc_layer%d" % i).res1.conv1.weight)
        return g

    def decoder_fwd(self, m, x, cats, training, dt, xf={}):
        """dec_layer5 .. dec_layer1 from the bottom tensor x; the skip channels of cats = (cat1 .. cat5) are already filled.
        xf: {level: (affine of a virtual deconv input, affine of virtual concat channels)}.  -> (dec_layer1's output, records)"""
        recs = [None] * 5
        for i in (5, 4, 3, 2, 1):
            dl, cat = getattr(m, "dec_layer%d" % i), cats[i - 1]
            out = self._new(tuple(cat.shape[:3]) + (dl.res.res2.conv2.out_channels,), dtype=dt, device=x.device)
            xf_x, xf_cat = xf.get(i, (None, None))
            recs[i - 1] = self.declayer_fwd(dl, x, cat, dl.deconv.out_channels, out, training, dt, xf_x=xf_x, xf_cat=xf_cat)
            x = out
        return x, tuple(recs)

    def decoder_bwd(self, m, sv, g, G, stage_done):
        """-> (gradient of the bottom tensor, gradients of cat1 .. cat5: their skip channels are what the encoder is owed)"""
        g_cats = []
        for i, rec in enumerate(sv.dec, 1):
            g, g_cat = self.declayer_bwd(rec, g, G); stage_done(getattr(m, "dec_layer%d" % i).deconv.weight)
            g_cats.append(g_cat)
        return g, g_cats

    def _backward_begin(self, sv, grad_ready):
        dev = sv.x.device
        self._rebind(sv)
        self._pack_bwd(sv.dt, dev)
        flat, views = self._grad_views(dev)
        stage_done = self._stage_notifier(flat, grad_ready)
        self._side_begin(dev)
        self._red_begin(dev)
        return flat, views, (lambda p: views[id(p)]), stage_done

    def _backward_end(self, sv, stage_done):
        stage_done(self.grad_order[-1][1])
        self._side_end(sv.x.device)
        self._red_buf = None

    # ------------------------------------------------------------------ UResNet (models/ub_uresnet.py:88-147)
    def _uresnet_buffers(self, x, dt):
        """-> (cat1 .. cat5 = [deconv | skip], the bottom tensor, the encoder levels' outputs: the skip halves and the bottom)"""
        N, _, H, W = x.shape
        ip = self.model.inplanes
        cats = self._concat_buffers(x, dt, [2 * ip, 4 * ip, 8 * ip, 16 * ip, 32 * ip])
        x5 = self._new((N, H // 32, W // 32, 32 * ip), dtype=dt, device=x.device)
        return cats, x5, [cats[1][..., 2 * ip:], cats[2][..., 4 * ip:], cats[3][..., 8 * ip:], cats[4][..., 16 * ip:], x5]

    def uresnet_forward(self, x: torch.Tensor, training: bool, dt: torch.dtype, save: bool):
        """training: BatchNorm modules in train mode use batch statistics (and update their running statistics), modules in eval
        mode are frozen; training = False freezes every site.  save: keep activations for backward"""
        m = self.model
        x, sv = self._forward_begin(x, training, dt, save)
        cats, x5, enc = self._uresnet_buffers(x, dt)
        p0 = self.stem_pool_fwd(m, x, cats[0], training, dt, sv)
        sv.enc, sv.aspp = self.encoder_fwd(m, p0, enc, training, dt), ()
        d1o, sv.dec = self.decoder_fwd(m, x5, cats, training, dt)
        out = self.head_fwd(m, d1o, training, dt, sv)
        return out, (sv if save else None)

    def uresnet_backward(self, sv: Saved, g_logp: torch.Tensor, grad_ready: Optional[Callable] = None):
        """-> flat fp32 gradient buffer (layout self.grad_offsets)."""
        m = self.model
        flat, views, G, stage_done = self._backward_begin(sv, grad_ready)
        g = self.head_bwd(m, sv, g_logp, G); stage_done(m.bn10.bias)
        g, gc = self.decoder_bwd(m, sv, g, G, stage_done)
        # skip gradients arrive through the concat buffers' second halves
        owed = [gc[i][..., sv.dec[i].Cd:] for i in (1, 2, 3, 4)] + [None]
        g = self.encoder_bwd(m, sv, g, owed, G, stage_done)
        self.stem_pool_bwd(m, sv, g, gc[0][..., sv.dec[0].Cd:], G)
        self._backward_end(sv, stage_done)
        return flat, views

    # ------------------------------------------------------------------ ASPP_ResNet (models/ASPP_ResNet.py:416-523)
    def _aspp_levels(self):
        m = self.model
        return [(m.ASPP_layer_enc3, m.ASPP_combine_enc3), (m.ASPP_layer_enc4, m.ASPP_combine_enc4), (m.ASPP_layer_enc5, m.ASPP_combine_enc5)]

    def _aspp_buffers(self, x, dt):
        """-> (cat1 .. cat5 with cat4 / cat5 = [deconv | ASPP_post | skip], skip5 = [ASPP_post(e5) | e5] (the bottom tensor),
        the encoder levels' outputs, the destinations of the three ASPP_post convs)"""
        N, _, H, W = x.shape
        ip = self.model.inplanes
        C3, C4, C5 = 8 * ip, 16 * ip, 32 * ip
        cats = self._concat_buffers(x, dt, [2 * ip, 4 * ip, 8 * ip, 3 * C3, 3 * C4])
        skip5 = self._new((N, H // 32, W // 32, 2 * C5), dtype=dt, device=x.device)
        enc = [cats[1][..., 2 * ip:], cats[2][..., 4 * ip:], cats[3][..., 2 * C3:], cats[4][..., 2 * C4:], skip5[..., C5:]]
        return cats, skip5, enc, [cats[3][..., C3:2 * C3], cats[4][..., C4:2 * C4], skip5[..., :C5]]

    def aspp_forward(self, x, training, dt, save):
        m = self.model
        x, sv = self._forward_begin(x, training, dt, save)
        ip = m.inplanes
        C3, C4, C5 = 8 * ip, 16 * ip, 32 * ip
        levels = self._aspp_levels()
        # affine arena: [acat3 | acat4 | acat5 | cat4 (up,post3,e3) | cat5 (up,post4,e4) | skip5 (post5,e5)]
        sizes = [64 + C3, 64 + C4, 64 + C5, C3 + 2 * C3, C4 + 2 * C4, 2 * C5]
        o, offs0 = 0, []
        for n in sizes:
            offs0.append(o)
            o += n
        relu_ranges = [(offs0[0], offs0[0] + 64), (offs0[1], offs0[1] + 64), (offs0[2], offs0[2] + 64),
                       (offs0[3] + C3, offs0[3] + 2 * C3), (offs0[4] + C4, offs0[4] + 2 * C4), (offs0[5], offs0[5] + C5)]
        arena, offs = self._affine_arena(sv, x.device, sizes, relu_ranges)
        for (layer, post), o_acat, o_post in zip(levels, offs[:3], (offs[3] + C3, offs[4] + C4, offs[5])):
            for b, (_, bn, _, _) in enumerate(layer.branches()):
                self._bind_site(self.bn(bn), arena, o_acat + 16 * b)
            self._bind_site(self.bn(post.ASPP_bn), arena, o_post)
        self._snapshot_sites(sv)

        cats, skip5, enc, posts = self._aspp_buffers(x, dt)
        p0 = self.stem_pool_fwd(m, x, cats[0], training, dt, sv)
        sv.enc = self.encoder_fwd(m, p0, enc, training, dt)
        sv.aspp = tuple(self.aspp_level_fwd(layer, post, e, cpost, arena, o_acat, training, dt)
                        for (layer, post), e, cpost, o_acat in zip(levels, enc[2:], posts, offs[:3]))
        xf = {5: (self._arena_affine(arena, offs[5], 2 * C5), self._arena_affine(arena, offs[4], 3 * C4)),
              4: (None, self._arena_affine(arena, offs[3], 3 * C3))}
        d1o, sv.dec = self.decoder_fwd(m, skip5, cats, training, dt, xf)
        out = self.head_fwd(m, d1o, training, dt, sv)
        return out, (sv if save else None)

    def aspp_backward(self, sv, g_logp, grad_ready=None):
        m = self.model
        flat, views, G, stage_done = self._backward_begin(sv, grad_ready)
        ip = m.inplanes
        C3, C4, C5 = 8 * ip, 16 * ip, 32 * ip
        g = self.head_bwd(m, sv, g_logp, G); stage_done(m.bn10.bias)
        gs5, gc = self.decoder_bwd(m, sv, g, G, stage_done)
        a3, a4, a5 = sv.aspp
        # an ASPP level's backward turns [gradient of its post conv's output | gradient of the direct skip] into the level's g_e
        g_e5 = self.aspp_level_bwd(a5, gs5[..., :C5], gs5[..., C5:], G)
        owed = [gc[1][..., 2 * ip:], gc[2][..., 4 * ip:],
                lambda: self.aspp_level_bwd(a3, gc[3][..., C3:2 * C3], gc[3][..., 2 * C3:], G),
                lambda: self.aspp_level_bwd(a4, gc[4][..., C4:2 * C4], gc[4][..., 2 * C4:], G), None]
        g = self.encoder_bwd(m, sv, g_e5, owed, G, stage_done)
        self.stem_pool_bwd(m, sv, g, gc[0][..., ip:], G)
        self._backward_end(sv, stage_done)
        return flat, views

    # ------------------------------------------------------------------ inference schedule (UResNet and ASPP_ResNet, eval mode)
    # SURVEY.md section 8d, k = 1: eval-mode BatchNorm is a fixed per-channel affine, so it is folded into the packed
    # weights (scale) and the conv bias; ReLU and the residual add run in the conv epilogue (ubr_conv_desc.act).  Every
    # tensor is written once, activated, and read by its consumers with no transform; block tails, BatchNorm finalize
    # launches and the raw conv2 / bypass outputs of the training schedule disappear (201 M instead of 250 M elements
    # per 512x512 image).  Reference call sites: deploy/run_ubresnet_precropped.py:88-89,147 (model.eval(); forward).
    def _infer_plan(self, dt, device):
        m = self.model
        key = ("inf", dt, device)
        ptrs = tuple(p.data_ptr() for _, p in self.grad_order) + tuple(b.data_ptr() for b in m.buffers())
        plan = self._plans.get(key)
        if plan is not None and plan["ptrs"] == ptrs:
            return plan
        cpu = L.chans_per_unit(dt)
        pairs = [(m.conv1, m.bn1), (m.conv10, m.bn10)]
        for mod in m.modules():
            if hasattr(mod, "bn2") and hasattr(mod, "conv2"):          # BasicBlock
                pairs += [(mod.conv1, mod.bn1), (mod.conv2, mod.bn2)]
                if mod.bypass is not None:
                    pairs.append((mod.bypass, mod.bnpass))
        # ASPP levels: the four branch pairs of a level stay adjacent, so their folded biases are the 64 contiguous floats
        # ubr_aspp_front reads, and their weights are packed into the one 28-tap image it reads
        levels = [mod for mod in m.modules() if hasattr(mod, "branches") and hasattr(mod, "B5_gp")]
        first_branch = {}
        for lay in levels:
            first_branch[id(lay.B1_bn)] = lay
            pairs += [(conv, bn) for conv, bn, _, _ in lay.branches()]
        pairs += [(mod.ASPP_conv, mod.ASPP_bn) for mod in m.modules() if hasattr(mod, "ASPP_conv")]
        total = sum(bn.num_features for _, bn in pairs)
        vec = self._new(2 * total, dtype=torch.float32, device=device)
        scale_of, bias_of, fold_tbl, off = {}, {}, b"", 0
        front_bias, front_img, branch_dst = {}, {}, {}
        for conv, bn in pairs:
            Cn = bn.num_features
            sc, bi = vec[off:off + Cn], vec[total + off:total + off + Cn]
            if id(bn) in first_branch:
                front_bias[id(first_branch[id(bn)])] = vec[total + off:total + off + 64]
            off += Cn
            scale_of[id(conv.weight)], bias_of[id(bn)] = sc, bi
            for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
                if t is None or t.dtype != torch.float32 or t.device != device:
                    raise RuntimeError("ubresnet_amd: inference needs affine BatchNorm2d with float32 running statistics on %s" % device)
            fold_tbl += struct.pack("<QQQQQQQif", bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                    conv.bias.data_ptr() if conv.bias is not None else 0, sc.data_ptr(), bi.data_ptr(), Cn, float(bn.eps))
        for lay in levels:
            Cn = lay.B1_conv.in_channels
            if Cn % cpu or any(conv.out_channels != 16 for conv, _, _, _ in lay.branches()):
                raise RuntimeError("ubresnet_amd: ASPP level with %d input channels cannot be packed for %s" % (Cn, dt))
            front = self._new((ops.ASPP_FRONT_TAPS, Cn // cpu, 16, cpu), dtype=dt, device=device)
            front_img[id(lay)] = front
            t0 = 0
            for conv, _, kk, _ in lay.branches():
                branch_dst[id(conv.weight)] = front[t0:t0 + kk * kk]
                t0 += kk * kk
        images, tables, counts = self._image_tables(dt, device, ("fwd",), scale_of=scale_of, slot_of=branch_dst)
        plan = {"ptrs": ptrs, "images": images, "bias": bias_of, "vec": vec, "fold": self._device_table(fold_tbl, device), "nfold": len(pairs),
                "pack": self._device_table(tables["fwd"], device), "npack": counts["fwd"], "front_img": front_img, "front_bias": front_bias}
        self._plans[key] = plan
        return plan

    def _block_infer(self, blk, x, out, fb, dt):
        """BasicBlock.forward (models/common_layers.py:39-58) with folded BatchNorms: 2 launches (3 with a bypass conv)"""
        N, OH, OW, Cout = out.shape
        S = blk.stride
        c1 = self._new((N, OH, OW, Cout), dtype=dt, device=x.device)
        ops.conv(x, self.packed(blk.conv1.weight, "fwd"), c1, T3, Cout, S=S, bias=fb[id(blk.bn1)], act=1)
        sc = x
        if blk.bypass is not None:
            sc = self._new((N, OH, OW, Cout), dtype=dt, device=x.device)
            ops.conv(x, self.packed(blk.bypass.weight, "fwd"), sc, T1, Cout, S=S, bias=fb[id(blk.bnpass)])
        ops.conv(c1, self.packed(blk.conv2.weight, "fwd"), out, T3, Cout, bias=fb[id(blk.bn2)], addend=sc, act=3)

    def _double_infer(self, dbl, x, out, fb, dt):
        mid = self._new(out.shape, dtype=dt, device=x.device)
        self._block_infer(dbl.res1, x, mid, fb, dt)
        self._block_infer(dbl.res2, mid, out, fb, dt)

    def _infer_begin(self, x, dt):
        """fold every BatchNorm and repack every forward image for this pass (two launches) -> (checked input, inference plan)"""
        x = self._check_input(x, self.model.conv1.in_channels)
        plan = self._infer_plan(dt, x.device)
        st = L.stream_ptr()
        L.check(L.lib().ubr_bn_fold_batched(plan["fold"].data_ptr(), plan["nfold"], st), "bn_fold_batched")
        L.check(L.lib().ubr_pack_weights_batched(L.dtype_id(dt), plan["pack"].data_ptr(), plan["npack"], st), "pack_weights_batched")
        self._images = plan["images"]
        return x, plan

    def _stem_infer(self, m, x, cat1, fb, dt):
        """conv1 (+bn1 folded, ReLU in the epilogue) writes x0 straight into dec1's concat buffer; the pool reads it"""
        N, Cin, H, W = x.shape
        ip = m.inplanes
        x0 = cat1[..., ip:]
        x16 = self._new((N, H, W, 16 * Cin), dtype=dt, device=x.device)
        self._untaped(lambda: ops.stem_expand(x, x16))
        if self._rec is not None:
            self._rec.pre = lambda xx: ops.stem_expand(xx, x16)
        for ci in range(Cin):
            ops.conv(x16[..., 16 * ci:16 * ci + 16], self.packed(m.conv1.weight, "stem%d" % ci), x0, self.STEM_TAPS, ip,
                     bias=fb[id(m.bn1)] if ci == 0 else None, addend=x0 if ci > 0 else None, act=2 if ci == Cin - 1 else 0)
        p0 = self._new((N, H // 2, W // 2, ip), dtype=dt, device=x.device)
        ops.maxpool_fwd(x0, None, p0, None, 2)
        return p0

    def _encoder_infer(self, m, x, outs, fb, dt):
        for i, out in enumerate(outs, 1):
            self._double_infer(getattr(m, "enc_layer%d" % i), x, out, fb, dt)
            x = out

    def _decoder_infer(self, m, x, cats, fb, dt):
        for i in (5, 4, 3, 2, 1):
            dl, cat = getattr(m, "dec_layer%d" % i), cats[i - 1]
            out = self._new(tuple(cat.shape[:3]) + (dl.res.res2.conv2.out_channels,), dtype=dt, device=x.device)
            self.deconv_fwd(dl, x, cat, dl.deconv.out_channels, dt)
            self._double_infer(dl.res, cat, out, fb, dt)
            x = out
        return x

    def _head_infer(self, m, d1o, fb, dt):
        N, H, W, _ = d1o.shape
        nk = m.conv10.out_channels
        c10 = self._new((N, H, W, nk), dtype=dt, device=d1o.device)
        ops.conv(d1o, self.packed(m.conv10.weight, "fwd"), c10, T7, nk, bias=fb[id(m.bn10)], act=1)
        ncls = m.conv11.out_channels
        return self._final_logsoftmax(m, c10, self.packed(m.conv11.weight, "fwd"), None, (N, ncls, H, W))

    def _aspp_level_infer(self, layer, post, e, cpost, plan, dt):
        """ASPP.forward + ASPP_post.forward (models/ASPP_ResNet.py:227-263,280-286), BatchNorms folded: the five branches in
        one launch, then the 1x1 back to C channels straight into its slice of the decoder's concat buffer"""
        N, h, w, Cn = e.shape
        acat = self._new((N, h, w, 64 + Cn), dtype=dt, device=e.device)
        ops.aspp_front(e, plan["front_img"][id(layer)], plan["front_bias"][id(layer)], acat)
        ops.conv(acat, self.packed(post.ASPP_conv.weight, "fwd"), cpost, T1, Cn, bias=plan["bias"][id(post.ASPP_bn)], act=1)

    def uresnet_infer(self, x, dt):
        """eval-mode UResNet.forward (models/ub_uresnet.py:88-147), nothing saved; buffer layout of uresnet_forward"""
        m = self.model
        x, plan = self._infer_begin(x, dt)
        fb = plan["bias"]
        cats, x5, enc = self._uresnet_buffers(x, dt)
        p0 = self._stem_infer(m, x, cats[0], fb, dt)
        self._encoder_infer(m, p0, enc, fb, dt)
        return self._head_infer(m, self._decoder_infer(m, x5, cats, fb, dt), fb, dt)

    def aspp_infer(self, x, dt):
        """eval-mode ASPP_ResNet.forward (models/ASPP_ResNet.py:416-523), nothing saved; buffer layout of aspp_forward"""
        m = self.model
        x, plan = self._infer_begin(x, dt)
        fb = plan["bias"]
        cats, skip5, enc, posts = self._aspp_buffers(x, dt)
        p0 = self._stem_infer(m, x, cats[0], fb, dt)
        self._encoder_infer(m, p0, enc, fb, dt)
        for (layer, post), e, cpost in zip(self._aspp_levels(), enc[2:], posts):
            self._aspp_level_infer(layer, post, e, cpost, plan, dt)
        return self._head_infer(m, self._decoder_infer(m, skip5, cats, fb, dt), fb, dt)

    # ------------------------------------------------------------------ dispatch
    def forward(self, x, training, dt, save):
        from . import plan
        return plan.forward(self, x, training, dt, save)

    def backward(self, sv, g_out, grad_ready=None, allow_plan=True):
        from . import plan
        return plan.backward(self, sv, g_out, grad_ready, allow_plan)

    def forward_eager(self, x, training, dt, save):
        if self.kind == "uresnet":
            if not training and not save and _INFER_FOLD:
                return self.uresnet_infer(x, dt), None
            return self.uresnet_forward(x, training, dt, save)
        if self.kind == "aspp":
            if not training and not save and _INFER_FOLD:
                return self.aspp_infer(x, dt), None
            return self.aspp_forward(x, training, dt, save)
        raise RuntimeError("ubresnet_amd: unknown network kind %r" % self.kind)

    def backward_eager(self, sv, g_out, grad_ready=None):
        if self.kind == "uresnet":
            return self.uresnet_backward(sv, g_out, grad_ready)
        if self.kind == "aspp":
            return self.aspp_backward(sv, g_out, grad_ready)
        raise RuntimeError("ubresnet_amd: unknown network kind %r" % self.kind)
