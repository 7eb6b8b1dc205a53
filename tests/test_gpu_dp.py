"""Data-parallel path on the GPU box: two ranks (gloo rendezvous on 127.0.0.1, both on cuda:0) run the real
train step on their shards of the global batch; after GradAllReducer.finish() every rank's .grad tensors are
the mean of the per-shard gradients (BatchNorm statistics local to the shard, as nn.DataParallel in
training/train_ubresnet2018_wlarcv2.py:99-103), and the .grad tensors alias the flat buffer that was reduced."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, backend="gloo", mode="step"):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = rank if backend == "nccl" else 0
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    if mode == "accum":
        return _worker_accum(rank, world, q)
    if mode == "steps":
        return _worker_steps(rank, world, q)
    if mode == "aspp":
        return _worker_aspp(rank, world, q)
    if mode == "aspp-steps":
        return _worker_aspp_steps(rank, world, q)
    if mode == "frozen":
        return _worker_frozen(rank, world, q)
    from oracle import uresnet_oracle as O
    from ubresnet_amd import synthetic
    from ubresnet_amd.dist import GradAllReducer, shard_range
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
    x, lab, wgt = synthetic.make_batch(4, 64, 64, 1000)
    crit = PixelWiseNLLLoss()

    def local_grads(lo, hi):
        m = UResNet(3, 1, 16)
        m.load_state_dict(sd)
        m = m.cuda().train()
        loss = crit(m(torch.from_numpy(x[lo:hi]).cuda()), torch.from_numpy(lab[lo:hi]).cuda(), torch.from_numpy(wgt[lo:hi]).cuda())
        loss.backward()
        return m, {n: p.grad.clone() for n, p in m.named_parameters()}

    # reference: both shards computed locally, no exchange
    _, g0 = local_grads(0, 2)
    _, g1 = local_grads(2, 4)
    lo, hi = shard_range(4, rank, world)
    m = UResNet(3, 1, 16)
    if rank == 0:
        m.load_state_dict(sd)       # the other ranks keep their random init: GradAllReducer broadcasts rank 0's state
    m = m.cuda().train()
    from ubresnet_amd.optim import FlatAdam
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)      # parameters become views of one buffer before the first forward
    red = GradAllReducer(m, bucket_bytes=8 << 20)
    loss = crit(m(torch.from_numpy(x[lo:hi]).cuda()), torch.from_numpy(lab[lo:hi]).cuda(), torch.from_numpy(wgt[lo:hi]).cuda())
    loss.backward()
    red.finish()
    torch.cuda.synchronize()
    flat = m.__dict__["_ubr_flat_grad"]
    ok, worst = True, 0.0
    for n, p in m.named_parameters():
        want = 0.5 * (g0[n] + g1[n])
        scale = max(want.abs().max().item(), 1e-8)
        err = (p.grad - want).abs().max().item() / scale
        worst = max(worst, err)
        inside = flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + flat.numel() * 4
        ok = ok and inside and (err <= 1e-5 or want.abs().max().item() < 1e-6)
    # SURVEY.md section 8e "Validation": the exchanged gradients equal the single-rank REFERENCE PATH (CPU oracle) run
    # shard by shard with per-shard BatchNorm statistics, averaged -- to the whole-network gradient tolerance
    # (tests/test_gpu_uresnet.py::_grad_verdict: ReLU-mask flips make fp32 gradients discontinuous)
    worst_l2, min_cos = 0.0, 1.0
    if rank == 0:
        xt, lt, wt = torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(wgt)
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        og = [O.train_step_grads(O.uresnet_forward, sd64, xt[a:b].double(), lt[a:b], wt[a:b].double())[1] for a, b in ((0, 2), (2, 4))]
        for n, p in m.named_parameters():
            if n in ("conv1.bias", "conv10.bias"):
                continue
            want = 0.5 * (og[0][n] + og[1][n])
            got = p.grad.detach().cpu().double()
            l2 = float((got - want).norm() / max(float(want.norm()), 1e-12))
            cos = float(torch.nn.functional.cosine_similarity(got.reshape(1, -1), want.reshape(1, -1)))
            worst_l2, min_cos = max(worst_l2, l2), min(min_cos, cos)
        ok = ok and worst_l2 <= 2e-2 and min_cos >= 0.9999
        print("dp vs oracle (shard by shard): worst l2 %.3e, min cos %.6f" % (worst_l2, min_cos), flush=True)
    # the replicas take the same optimizer step from the averaged flat buffer and stay bitwise in sync
    before = opt.flat.clone()
    opt.step()
    torch.cuda.synchronize()
    moved = float((opt.flat - before).abs().max())
    digest = opt.flat.double().sum().item()
    q.put((rank, bool(ok and moved > 0 and torch.isfinite(opt.flat).all().item()), worst, digest))
    dist.destroy_process_group()


def _worker_accum(rank, world, q):
    """two backward passes per optimizer step (gradient accumulation) under the reducer: the first pass is exchanged
    during backward, the second accumulates locally and finish() reduces the accumulated .grad tensors"""
    from oracle import uresnet_oracle as O
    from ubresnet_amd import synthetic
    from ubresnet_amd.dist import GradAllReducer
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
    x, lab, wgt = synthetic.make_batch(4, 64, 64, 1000)
    crit = PixelWiseNLLLoss()

    def run(m, i):
        crit(m(torch.from_numpy(x[i:i + 1]).cuda()), torch.from_numpy(lab[i:i + 1]).cuda(), torch.from_numpy(wgt[i:i + 1]).cuda()).backward()

    single = []
    for i in range(4):                      # every image alone, no exchange
        m = UResNet(3, 1, 16); m.load_state_dict(sd); m = m.cuda().train()
        run(m, i)
        single.append({n: p.grad.clone() for n, p in m.named_parameters()})
    m = UResNet(3, 1, 16); m.load_state_dict(sd); m = m.cuda().train()
    red = GradAllReducer(m, bucket_bytes=8 << 20)
    run(m, 2 * rank)
    run(m, 2 * rank + 1)                    # no zero_grad in between
    red.finish()
    torch.cuda.synchronize()
    worst = 0.0
    for n, p in m.named_parameters():
        want = 0.5 * (single[0][n] + single[1][n] + single[2][n] + single[3][n])
        worst = max(worst, (p.grad - want).abs().max().item() / max(want.abs().max().item(), 1e-8))
    digest = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).double().sum().item()
    q.put((rank, bool(worst <= 1e-5), worst, digest))
    dist.destroy_process_group()


def _worker_steps(rank, world, q):
    """several optimizer steps under the reducer: from the second step on the backward pass is a replayed launch tape and the
    gradient ranges are handed to the reducer through tape marks (ordered=False, dist.py) -- bitwise the same parameters as the
    Python-scheduled run (ubresnet_amd.plan.ENABLED = False), and the same on every rank"""
    from oracle import uresnet_oracle as O
    from ubresnet_amd import plan, synthetic
    from ubresnet_amd.dist import GradAllReducer, shard_range
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
    crit = PixelWiseNLLLoss()
    lo, hi = shard_range(4, rank, world)
    res = {}
    for enabled in (True, False):
        plan.ENABLED = enabled
        m = UResNet(3, 1, 16)
        m.load_state_dict(sd)
        m = m.cuda().train()
        m.compute_dtype = torch.bfloat16
        opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
        red = GradAllReducer(m, bucket_bytes=1 << 20)          # small buckets: several exchanges per backward
        for i in range(4):
            x, lab, wgt = synthetic.make_batch(4, 64, 64, 1000 + 10 * i)
            loss = crit(m(torch.from_numpy(x[lo:hi]).cuda()), torch.from_numpy(lab[lo:hi]).cuda(), torch.from_numpy(wgt[lo:hi]).cuda())
            opt.zero_grad()
            loss.backward()
            red.finish()
            opt.step()
        torch.cuda.synchronize()
        eng = m.__dict__["_ubr_engine"]
        replayed = any(p.bwd is not None and p.uses >= 3 for p in eng._planned.values())
        res[enabled] = (opt.flat.clone(), replayed)
    same = torch.equal(res[True][0], res[False][0])
    digest = res[True][0].double().sum().item()
    q.put((rank, bool(same and res[True][1] and not res[False][1] and torch.isfinite(res[True][0]).all().item()), 0.0, digest))
    dist.destroy_process_group()


def _worker_aspp(rank, world, q):
    """ASPP_ResNet under the reducer: its completion order interleaves ASPP_combine / ASPP_layer / enc_layer for levels 5, 4, 3,
    and levels 4 and 3 are back-propagated from inside the encoder's loop.  1 MiB buckets: several leave during backward.
    Global batch 2 of 3x64x96, one image per rank (BatchNorm statistics local to the shard)"""
    from oracle import uresnet_oracle as O
    from ubresnet_amd import synthetic
    from ubresnet_amd.dist import GradAllReducer, shard_range
    from ubresnet_amd.models.ASPP_ResNet import ASPP_ResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    from test_gpu_uresnet import _grad_row, _grad_verdict
    sd = O.seeded_state_dict(O.aspp_resnet_schema(3, 3, 16), 42)
    x, lab, wgt = synthetic.make_batch(2, 64, 96, 1000, planes=3)
    crit = PixelWiseNLLLoss()

    def step(m, lo, hi):
        crit(m(torch.from_numpy(x[lo:hi]).cuda()), torch.from_numpy(lab[lo:hi]).cuda(), torch.from_numpy(wgt[lo:hi]).cuda()).backward()

    def local_grads(lo, hi):
        m = ASPP_ResNet(3, 3, 16, showsizes=False)
        m.load_state_dict(sd)
        m = m.cuda().train()
        step(m, lo, hi)
        return {n: p.grad.clone() for n, p in m.named_parameters()}

    g0, g1 = local_grads(0, 1), local_grads(1, 2)
    lo, hi = shard_range(2, rank, world)
    m = ASPP_ResNet(3, 3, 16, showsizes=False)
    if rank == 0:
        m.load_state_dict(sd)       # the other ranks keep their random init: GradAllReducer broadcasts rank 0's state
    m = m.cuda().train()
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
    red = GradAllReducer(m, bucket_bytes=1 << 20)
    launches = []
    launch = red._launch
    red._launch = lambda a, b: (launches.append((a, b)), launch(a, b))[1]
    step(m, lo, hi)
    in_backward = len(launches)
    red.finish()
    torch.cuda.synchronize()
    flat = m.__dict__["_ubr_flat_grad"]
    ok, worst = in_backward >= 3, 0.0
    for n, p in m.named_parameters():
        want = 0.5 * (g0[n] + g1[n])
        scale = max(want.abs().max().item(), 1e-8)
        err = (p.grad - want).abs().max().item() / scale
        worst = max(worst, err)
        inside = flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + flat.numel() * 4
        ok = ok and inside and (err <= 1e-5 or want.abs().max().item() < 1e-6)
    # rank 0: the exchanged gradients against the fp64 oracle run shard by shard, through the whole-network gate of
    # tests/test_gpu_aspp.py::test_aspp_train_step (cosine >= 0.999, relative L2 <= 5e-2, or within 10x the fp32 oracle's own
    # distance from fp64; the conv biases a BatchNorm follows are analytically zero)
    info = {"buckets_in_backward": in_backward, "worst_l2": 0.0, "min_cos": 1.0}
    if rank == 0:
        xt, lt, wt = torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(wgt)
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        o32 = [O.train_step_grads(O.aspp_resnet_forward, sd, xt[a:b], lt[a:b], wt[a:b])[1] for a, b in ((0, 1), (1, 2))]
        o64 = [O.train_step_grads(O.aspp_resnet_forward, sd64, xt[a:b].double(), lt[a:b], wt[a:b].double())[1] for a, b in ((0, 1), (1, 2))]
        params = dict(m.named_parameters())
        zero_bias = {"conv1.bias", "conv10.bias"} | {n for n in o64[0] if n.endswith("_conv.bias")}
        fails = []
        for n in o64[0]:
            gv = params[n].grad.detach().cpu().double()
            if n in zero_bias:
                if gv.abs().max().item() > 1e-4:
                    fails.append("%s is not zero" % n)
                continue
            row = _grad_row(n, gv, 0.5 * (o32[0][n] + o32[1][n]).double(), 0.5 * (o64[0][n] + o64[1][n]))
            fails += _grad_verdict(row, cos_min=0.999, l2_max=5e-2)
            info["worst_l2"], info["min_cos"] = max(info["worst_l2"], row[3]), min(info["min_cos"], row[5])
        ok = ok and not fails
        print("dp aspp vs oracle (shard by shard): worst l2 %.3e, min cos %.6f, %d buckets left during backward; %s"
              % (info["worst_l2"], info["min_cos"], in_backward, "; ".join(fails[:6]) or "all pass"), flush=True)
    before = opt.flat.clone()
    opt.step()
    torch.cuda.synchronize()
    moved = float((opt.flat - before).abs().max())
    digest = opt.flat.double().sum().item()
    q.put((rank, bool(ok and moved > 0 and torch.isfinite(opt.flat).all().item()), worst, digest, info))
    dist.destroy_process_group()


def _worker_aspp_steps(rank, world, q):
    """_worker_steps for ASPP_ResNet in bf16: 4 optimizer steps under the reducer, the replayed backward hands its ranges over
    through tape marks -- bitwise the parameters of the Python-scheduled run, and the same on every rank"""
    from oracle import uresnet_oracle as O
    from ubresnet_amd import plan, synthetic
    from ubresnet_amd.dist import GradAllReducer, shard_range
    from ubresnet_amd.models.ASPP_ResNet import ASPP_ResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    sd = O.seeded_state_dict(O.aspp_resnet_schema(3, 3, 16), 42)
    crit = PixelWiseNLLLoss()
    lo, hi = shard_range(2, rank, world)
    res = {}
    for enabled in (True, False):
        plan.ENABLED = enabled
        m = ASPP_ResNet(3, 3, 16, showsizes=False)
        m.load_state_dict(sd)
        m = m.cuda().train()
        m.compute_dtype = torch.bfloat16
        opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
        red = GradAllReducer(m, bucket_bytes=1 << 20)
        for i in range(4):
            x, lab, wgt = synthetic.make_batch(2, 64, 96, 1000 + 10 * i, planes=3)
            loss = crit(m(torch.from_numpy(x[lo:hi]).cuda()), torch.from_numpy(lab[lo:hi]).cuda(), torch.from_numpy(wgt[lo:hi]).cuda())
            opt.zero_grad()
            loss.backward()
            red.finish()
            opt.step()
        torch.cuda.synchronize()
        eng = m.__dict__["_ubr_engine"]
        replayed = any(p.bwd is not None and p.uses >= 3 for p in eng._planned.values())
        res[enabled] = (opt.flat.clone(), replayed)
    same = torch.equal(res[True][0], res[False][0])
    digest = res[True][0].double().sum().item()
    q.put((rank, bool(same and res[True][1] and not res[False][1] and torch.isfinite(res[True][0]).all().item()), 0.0, digest, {}))
    dist.destroy_process_group()


def _worker_frozen(rank, world, q):
    """UResNet fine-tuned with a frozen encoder under the reducer: stem and encoder BatchNorms in eval mode on normalising
    running statistics (the frozen-BatchNorm fixture's), decoder and head training.  The frozen sites' dgamma / dbeta are
    written at the end of their stage (Engine._fin_flush), inside the range that stage reports"""
    import numpy as np
    from oracle import uresnet_oracle as O
    from ubresnet_amd import synthetic
    from ubresnet_amd.dist import GradAllReducer, shard_range
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    from grad_ready_probe import freeze_encoder
    g = np.load(os.path.join(REPO, "tests", "golden", "uresnet_ip16_frozen_2x1x64x64.npz"))
    sd = O.state_dict_with_bn_stats(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), int(g["meta"][5])), g["bn_keys"], g["bn_stats"])
    x, lab, wgt = synthetic.make_batch(4, 64, 64, 1000)
    crit = PixelWiseNLLLoss()

    def step(m, lo, hi):
        crit(m(torch.from_numpy(x[lo:hi]).cuda()), torch.from_numpy(lab[lo:hi]).cuda(), torch.from_numpy(wgt[lo:hi]).cuda()).backward()

    def local_grads(lo, hi):
        m = UResNet(3, 1, 16)
        m.load_state_dict(sd)
        m = m.cuda()
        freeze_encoder(m)
        step(m, lo, hi)
        return {n: p.grad.clone() for n, p in m.named_parameters()}

    g0, g1 = local_grads(0, 2), local_grads(2, 4)
    lo, hi = shard_range(4, rank, world)
    m = UResNet(3, 1, 16)
    if rank == 0:
        m.load_state_dict(sd)
    m = m.cuda()
    frozen = freeze_encoder(m)
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
    red = GradAllReducer(m, bucket_bytes=1 << 20)       # (broadcasts rank 0's parameters and running statistics)
    step(m, lo, hi)
    red.finish()
    torch.cuda.synchronize()
    ok, worst = len(frozen) == 26, 0.0
    for n, p in m.named_parameters():
        want = 0.5 * (g0[n] + g1[n])
        err = (p.grad - want).abs().max().item() / max(want.abs().max().item(), 1e-8)
        worst = max(worst, err)
        ok = ok and (err <= 1e-5 or want.abs().max().item() < 1e-6)
    # a frozen module's running statistics are bit for bit what rank 0 loaded; a training module's moved
    state = m.state_dict()
    for name in frozen:
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            ok = ok and torch.equal(state["%s.%s" % (name, k)].cpu(), sd["%s.%s" % (name, k)])
    ok = ok and not torch.equal(state["bn10.running_mean"].cpu(), sd["bn10.running_mean"])
    before = opt.flat.clone()
    opt.step()
    torch.cuda.synchronize()
    moved = float((opt.flat - before).abs().max())
    digest = opt.flat.double().sum().item()
    q.put((rank, bool(ok and moved > 0 and torch.isfinite(opt.flat).all().item()), worst, digest, {}))
    dist.destroy_process_group()


def _ddp_worker(rank, world, port, q):
    """the reference's own kind of wrap (training/train_ubresnet2018_wlarcv2.py:99,103: nn.DataParallel; here its
    one-process-per-GPU sibling DistributedDataParallel, which works on a one-GPU box): gradients reach DDP's reducer through
    the autograd compatibility path and the step equals the unwrapped one"""
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import warnings
    from oracle import uresnet_oracle as O
    from ubresnet_amd import synthetic
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
    x, lab, wgt = [torch.from_numpy(a).cuda() for a in synthetic.make_batch(2, 64, 64, 1000)]
    crit = PixelWiseNLLLoss()
    plain = UResNet(3, 1, 16); plain.load_state_dict(sd); plain = plain.cuda().train()
    crit(plain(x), lab, wgt).backward()
    wrapped = UResNet(3, 1, 16); wrapped.load_state_dict(sd); wrapped = wrapped.cuda().train()
    ddp = torch.nn.parallel.DistributedDataParallel(wrapped, device_ids=[0])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        crit(ddp(x), lab, wgt).backward()
    torch.cuda.synchronize()
    warned = any("GradAllReducer" in str(i.message) for i in w)
    ok = warned and all(p.grad is not None and torch.equal(p.grad, q_.grad) for p, q_ in zip(wrapped.parameters(), plain.parameters()))
    opt = torch.optim.SGD(ddp.parameters(), lr=0.1)
    before = wrapped.conv11.weight.detach().clone()
    opt.step()
    ok = ok and not torch.equal(before, wrapped.conv11.weight.detach())
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_distributed_data_parallel_wrapper_trains():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_ddp_worker, args=(0, 1, _free_port(), q))
    p.start()
    res = q.get(timeout=600)
    p.join(timeout=60)
    assert res == (0, True)


def test_two_rank_replayed_steps_equal_python_scheduled_steps():
    res = _run_two_ranks(mode="steps")
    assert [r[:2] for r in res] == [(0, True), (1, True)]
    assert res[0][3] == res[1][3], "replicas diverged: %r vs %r" % (res[0][3], res[1][3])


def _run_two_ranks(backend="gloo", mode="step"):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q, backend, mode)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=600) for _ in ps)
    for p in ps:
        p.join(timeout=60)
    return res


def test_two_rank_accumulated_micro_batches():
    res = _run_two_ranks(mode="accum")
    print("dp accumulate worst rel err per rank", [r[2] for r in res])
    assert [r[:2] for r in res] == [(0, True), (1, True)]
    assert res[0][3] == res[1][3], "ranks hold different gradients after finish()"


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL over xGMI); the one-GPU box runs the gloo variant")
def test_two_rank_gradient_average_rccl():
    """the same step with backend nccl (= RCCL), one rank per GPU: runs wherever the box has two devices"""
    res = _run_two_ranks(backend="nccl")
    assert [r[:2] for r in res] == [(0, True), (1, True)]
    assert res[0][3] == res[1][3]


def test_two_rank_gradient_average():
    res = _run_two_ranks()
    print("dp worst rel err per rank", [r[2] for r in res])
    assert [r[:2] for r in res] == [(0, True), (1, True)]
    assert res[0][3] == res[1][3], "replicas diverged after the optimizer step: %r vs %r" % (res[0][3], res[1][3])


def test_two_rank_aspp_gradient_average():
    res = _run_two_ranks(mode="aspp")
    print("dp aspp worst rel err per rank vs local shards", [r[2] for r in res], "rank 0 vs oracle", res[0][4])
    assert [r[:2] for r in res] == [(0, True), (1, True)]
    assert res[0][3] == res[1][3], "replicas diverged after the optimizer step: %r vs %r" % (res[0][3], res[1][3])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL over xGMI); the one-GPU box runs the gloo variant")
def test_two_rank_aspp_gradient_average_rccl():
    """the ASPP_ResNet step with backend nccl (= RCCL), one rank per GPU: runs wherever the box has two devices"""
    res = _run_two_ranks(backend="nccl", mode="aspp")
    assert [r[:2] for r in res] == [(0, True), (1, True)]
    assert res[0][3] == res[1][3]


def test_two_rank_aspp_replayed_steps_equal_python_scheduled_steps():
    res = _run_two_ranks(mode="aspp-steps")
    assert [r[:2] for r in res] == [(0, True), (1, True)]
    assert res[0][3] == res[1][3], "replicas diverged: %r vs %r" % (res[0][3], res[1][3])


def test_two_rank_frozen_encoder_gradient_average():
    res = _run_two_ranks(mode="frozen")
    print("dp frozen-encoder worst rel err per rank vs local shards", [r[2] for r in res])
    assert [r[:2] for r in res] == [(0, True), (1, True)]
    assert res[0][3] == res[1][3], "replicas diverged after the optimizer step: %r vs %r" % (res[0][3], res[1][3])


def test_grad_accumulates_like_autograd():
    sys.path.insert(0, REPO)
    from oracle import uresnet_oracle as O
    from ubresnet_amd import synthetic
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss
    sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
    x, lab, wgt = synthetic.make_batch(1, 64, 64, 1000)
    m = UResNet(3, 1, 16)
    m.load_state_dict(sd)
    m = m.cuda().train()
    crit = PixelWiseNLLLoss()
    args = (torch.from_numpy(lab).cuda(), torch.from_numpy(wgt).cuda())
    crit(m(torch.from_numpy(x).cuda()), *args).backward()
    g1 = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.bn1.momentum = 0.0          # keep the running stats (they do not enter train-mode outputs anyway)
    crit(m(torch.from_numpy(x).cuda()), *args).backward()       # no zero_grad: gradients accumulate
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad, 2 * g1[n], rtol=1e-5, atol=1e-7), n
    m.zero_grad()
    assert all(p.grad is None for p in m.parameters())
