"""tests/stage_shadow.py without a device: the expected-graph matcher on a hand-written tape, the tap + replay + graphs on the CPU
stand-in for the kernels (every launch = its fp64 reference rounded once), and the tape mutations a wiring bug would leave.
The stand-in exercises the plumbing (tap, graphs, chain); its error ratios say nothing about the bounds, which the device run measures."""
import pytest
import torch

import kref
import stage_shadow as S

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------
# a hand-written tape: conv1(x) -> c1; conv2(relu(bn1(c1))) -> c2; bypass(x) -> cb; tail(c2, cb) -> out, mask.  Addresses invented.
# ------------------------------------------------------------------------------------------------------------------
def _rec(ptr, shape, dtype, fill=0.0):
    t = torch.full(shape, fill, dtype=dtype)
    r = S.TRec(t, False)
    r.ptr, r.after = ptr, t.clone()
    return r


N, H, W, C = 1, 4, 4, 16
ACT = (N, H, W, C)
ADDR = dict(x=0x1000, c1=0x2000, c2=0x3000, cb=0x4000, out=0x5000, mask=0x6000, w1=0x7000, w2=0x8000, wb=0x9000,
            mean1=0xa000, scale1=0xa100, shift1=0xa200, zero=0xa300, mean2=0xb000, scale2=0xb100, shift2=0xb200,
            meanb=0xc000, scaleb=0xc100, shiftb=0xc200)


def _vec(name):
    return _rec(ADDR[name], (C,), torch.float32)


def _hand_tape(dt=BF, mask_bytes=None):
    act = lambda n: _rec(ADDR[n], ACT, dt)
    wp = lambda n, taps: _rec(ADDR[n], (taps, C // kref.CPU[dt], 16, kref.CPU[dt]), dt)
    none_xf = {"xf.sub": None, "xf.scale": None, "xf.shift": None, "xf.lo": None}
    nb = N * H * W * (C // kref.CPU[dt]) if mask_bytes is None else mask_bytes
    return [
        S.Launch("conv", dict(x=act("x"), wp=wp("w1", 9), y=act("c1"), Cout=C, S=1, **none_xf)),
        S.Launch("conv", dict(x=act("c1"), wp=wp("w2", 9), y=act("c2"), Cout=C, S=1,
                              **{"xf.sub": _vec("mean1"), "xf.scale": _vec("scale1"), "xf.shift": _vec("shift1"), "xf.lo": _vec("zero")})),
        S.Launch("conv", dict(x=act("x"), wp=wp("wb", 1), y=act("cb"), Cout=C, S=1, **none_xf)),
        S.Launch("block_tail_fwd", dict(c2=act("c2"), mean2=_vec("mean2"), scale2=_vec("scale2"), shift2=_vec("shift2"), sc=act("cb"),
                                        mean_b=_vec("meanb"), scale_b=_vec("scaleb"), shift_b=_vec("shiftb"), out=act("out"),
                                        relu_mask=_rec(ADDR["mask"], (nb,), torch.uint8))),
    ]


def _hand_graph(dt=BF):
    g = S.Graph()
    ext = lambda n, shape, d: S.Sym(n, shape, d, ptr=ADDR[n])
    v = lambda n: ext(n, (C,), torch.float32)
    x, out = ext("x", ACT, dt), ext("out", ACT, dt)
    c1, c2, cb = g.new("c1", ACT, dt), g.new("c2", ACT, dt), g.new("cb", ACT, dt)
    wshape = lambda taps: (taps, C // kref.CPU[dt], 16, kref.CPU[dt])
    mask = g.new("mask", (N * H * W * (C // kref.CPU[dt]),), torch.uint8)
    no = {"xf.sub": None, "xf.scale": None, "xf.shift": None, "xf.lo": None}
    g.node("conv", writes=("y",), x=x, wp=ext("w1", wshape(9), dt), y=c1, Cout=C, S=1, **no)
    g.node("conv", writes=("y",), x=c1, wp=ext("w2", wshape(9), dt), y=c2, Cout=C, S=1,
           **{"xf.sub": v("mean1"), "xf.scale": v("scale1"), "xf.shift": v("shift1"), "xf.lo": v("zero")})
    g.node("conv", writes=("y",), x=x, wp=ext("wb", wshape(1), dt), y=cb, Cout=C, S=1, **no)
    g.node("block_tail_fwd", writes=("out", "relu_mask"), c2=c2, mean2=v("mean2"), scale2=v("scale2"), shift2=v("shift2"), sc=cb,
           mean_b=v("meanb"), scale_b=v("scaleb"), shift_b=v("shiftb"), out=out, relu_mask=mask)
    return g


def test_graph_accepts_a_correct_and_a_permuted_hand_written_tape():
    _hand_graph().match(_hand_tape())
    t = _hand_tape()
    _hand_graph().match([t[0], t[2], t[1], t[3]])         # the bypass conv depends on nothing but x
    _hand_graph().match([t[2], t[0], t[1], t[3]])


def test_graph_rejects_a_consumer_before_its_producer_and_an_extra_launch():
    t = _hand_tape()
    with pytest.raises(AssertionError, match="before"):
        _hand_graph().match([t[1], t[0], t[2], t[3]])
    with pytest.raises(AssertionError, match="does not ask for"):
        _hand_graph().match(t + [_hand_tape()[2]])


def test_graph_rejects_one_swapped_xf_and_one_wrong_mask_length():
    t = _hand_tape()
    t[1].args["xf.sub"], t[1].args["xf.scale"] = _vec("mean2"), _vec("scale2")      # bn2's vectors where bn1's belong
    with pytest.raises(AssertionError, match="xf.sub"):
        _hand_graph().match(t)
    with pytest.raises(AssertionError, match="relu_mask"):
        _hand_graph().match(_hand_tape(mask_bytes=N * H * W * (C // 8) // 2))
    # the fp32 unit width in a 16-bit type gives twice the bytes: also not this dtype's mask
    with pytest.raises(AssertionError, match="relu_mask"):
        _hand_graph().match(_hand_tape(mask_bytes=N * H * W * (C // 4)))
    t = _hand_tape()
    t[3].args["c2"].dtype = torch.float32
    with pytest.raises(AssertionError, match="dtype"):
        _hand_graph().match(t)


def test_graph_rejects_a_reader_that_does_not_see_its_writers_bytes():
    t = _hand_tape()
    t[1].args["x"].before = torch.ones(ACT, dtype=BF)       # c1's storage handed to something else in between
    with pytest.raises(AssertionError, match="not the bytes"):
        _hand_graph().match(t)


# ------------------------------------------------------------------------------------------------------------------
# the whole machinery on the CPU stand-in
# ------------------------------------------------------------------------------------------------------------------
CASES = {
    "identity": lambda m, dt: S.block_case(m, dt, "cpu", 16, 16, 1, (24, 40), emu=True),
    "identity_go2": lambda m, dt: S.block_case(m, dt, "cpu", 32, 32, 1, (20, 36), go2=True, emu=True),
    "projection": lambda m, dt: S.block_case(m, dt, "cpu", 16, 32, 1, (20, 36), emu=True),
    "down": lambda m, dt: S.block_case(m, dt, "cpu", 32, 64, 2, (24, 40), emu=True),
    "virtual": lambda m, dt: S.block_case(m, dt, "cpu", 32, 32, 2, (24, 40), virtual=True, emu=True),
    "separate_finalize": lambda m, dt: S.block_case(m, dt, "cpu", 32, 32, 1, (20, 36), fin_max=16, emu=True),
    "eval": lambda m, dt: S.block_case(m, dt, "cpu", 16, 32, 1, (20, 36), training=False, backward=False, emu=True),
    "double": lambda m, dt: S.double_case(m, dt, "cpu", 32, 64, 2, (24, 40), need_gx=False, emu=True),
    "all_frozen_identity": lambda m, dt: S.block_case(m, dt, "cpu", 32, 32, 1, (20, 36), emu=True, freeze=("bn1", "bn2")),
    "all_frozen_projection": lambda m, dt: S.block_case(m, dt, "cpu", 16, 32, 1, (20, 36), emu=True, freeze=("bn1", "bn2", "bnpass")),
    "mixed_bn2_frozen": lambda m, dt: S.block_case(m, dt, "cpu", 16, 32, 1, (20, 36), emu=True, freeze=("bn2",)),
    "mixed_bnpass_frozen": lambda m, dt: S.block_case(m, dt, "cpu", 32, 64, 2, (24, 40), emu=True, freeze=("bnpass",)),
    "aspp_level": lambda m, dt: S.aspp_case(m, dt, "cpu", 128, (20, 36), emu=True),
    "deconv_layer": lambda m, dt: S.declayer_case(m, dt, "cpu", 64, 32, 32, 32, (12, 20), emu=True),
    "stem_one_plane": lambda m, dt: S.stem_case(m, dt, "cpu", 2, 1, 24, 40, 16, emu=True),
    "stem_three_planes": lambda m, dt: S.stem_case(m, dt, "cpu", 2, 3, 20, 36, 32, emu=True),
    "stem_eval": lambda m, dt: S.stem_case(m, dt, "cpu", 2, 1, 24, 40, 16, training=False, emu=True),
    "head_3_classes": lambda m, dt: S.head_case(m, dt, "cpu", 2, 24, 40, 16, 16, 3, emu=True),
    "head_4_classes": lambda m, dt: S.head_case(m, dt, "cpu", 2, 20, 36, 16, 16, 4, emu=True),
    "head_bn10_frozen": lambda m, dt: S.head_case(m, dt, "cpu", 2, 24, 40, 16, 16, 3, freeze=("bn10",), emu=True),
}


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", sorted(CASES))
def test_stage_on_the_cpu_stand_in(monkeypatch, case, dt):
    r = CASES[case](monkeypatch, dt)
    stat = S.check_all(r)
    assert all(v[1] <= 1.0 for v in stat.values())
    for o in r["outputs"]:
        assert bool(torch.isfinite(o.float()).all())


@pytest.fixture(scope="module")
def projection_run():
    mp = pytest.MonkeyPatch()
    try:
        r = CASES["projection"](mp, BF)
        S.check_all(r)
        yield r
    finally:
        mp.undo()


@pytest.mark.parametrize("kind", S.MUTATIONS)
def test_mutated_tape_is_rejected(projection_run, kind):
    tape, what = S.mutate(projection_run["tape"], kind)
    with pytest.raises(AssertionError):
        projection_run["graph"].match(tape)
    if kind in ("swap_bn2_bnpass", "xf_identity", "swap_red"):
        with pytest.raises(AssertionError):
            S.replay(tape)


def test_permuted_recorded_tape_is_accepted(projection_run):
    tape = list(projection_run["tape"])
    i = next(i for i, L in enumerate(tape) if L.op == "wgrad")
    tape[i], tape[i + 1] = tape[i + 1], tape[i]          # a weight gradient and the data gradient issued after it are independent
    projection_run["graph"].match(tape)


def test_replay_sees_one_wrong_element_and_one_byte_beside_a_view(projection_run):
    tape, _ = S.mutate(projection_run["tape"], "dtype_fp32")       # (a copy of the records)
    L = next(L for L in projection_run["tape"] if L.op == "block_tail_bwd_apply_fin")
    r = L.args["g_c2"]
    bad = S._copy_rec(r, after=r.after.clone())
    bad.after[1, 7, 9, 3] += 0.25
    with pytest.raises(AssertionError, match="outside the bound"):
        S.check_launch(0, S.Launch(L.op, dict(L.args, g_c2=bad)))
    L = next(L for L in projection_run["tape"] if L.op == "bn_finalize")
    r, last = L.args["scale"], L.args["invstd"]
    bad = S._copy_rec(r, base_after=r.base_after.clone())
    # the first element behind the site's four vectors: nothing has written it yet, so whatever it holds, one bit of it changes
    bad.base_after.view(kref._ITY[bad.base_after.element_size()])[last.off + last.shape[0]] ^= 1
    with pytest.raises(AssertionError, match="outside its output"):
        S.check_launch(0, S.Launch(L.op, dict(L.args, scale=bad)))


def test_chain_sees_an_exact_element_changed_after_its_launch(projection_run):
    r = projection_run
    assert S.check_chain(r["tape"], r["flat"], r["outputs"]) > 0
    val, ex = S.chain(r["tape"], r["flat"])[r["flat"].untyped_storage().data_ptr()]
    i = int(ex.nonzero()[0])
    gx = r["flat"]
    old = gx.view(-1)[i].clone()
    gx.view(-1)[i] = 0.375 if float(old) != 0.375 else 0.5          # (a BatchNorm gradient clobbered after the launch that wrote it)
    try:
        with pytest.raises(AssertionError, match="chain of rounded replays"):
            S.check_chain(r["tape"], r["flat"], r["outputs"])
    finally:
        gx.view(-1)[i] = old


# ------------------------------------------------------------------------------------------------------------------
# the whole networks on the stand-in (one storage type each, as on the device): wiring, and the harness at the networks' size
# ------------------------------------------------------------------------------------------------------------------
def _net(which, dt):
    mp = pytest.MonkeyPatch()
    try:
        r = S.net_case(mp, dt, "cpu", which, emu=True)
    finally:
        mp.undo()          # (the tap comes off before any other test launches anything: the tape is this pass and nothing else)
    yield r, S.check_all(r)


@pytest.fixture(scope="module")
def uresnet_run():
    yield from _net("uresnet", BF)


def _assert_net(r, stat):
    assert all(v[1] <= 1.0 for v in stat.values())
    assert sum(v[0] for v in stat.values()) == len(r["tape"]) and r["exact"] > 0
    assert bool(torch.isfinite(r["outputs"][0]).all())
    # the flat gradient buffer and the reduction arenas went the device-side way: no host copy of a whole storage per launch
    big = [v for L in r["tape"] for v in L.args.values() if isinstance(v, S.TRec) and v.big]
    assert big and all(v.base_before is None and v.base_after is None and v.outside == (0, -1) for v in big)
    assert len({id(v.base_init) for v in big}) <= 4


def test_whole_uresnet_on_the_cpu_stand_in(uresnet_run):
    _assert_net(*uresnet_run)


def test_whole_aspp_resnet_on_the_cpu_stand_in():
    for r, stat in _net("aspp", torch.float16):
        _assert_net(r, stat)
        # dec_layer5 reads its virtual deconv input and dec_layer4 / 5 their virtual concat channels through arena slices
        xf = [L for L in r["tape"] if L.op == "conv_phases" and L.args.get("xf.scale") is not None]
        assert len(xf) == 1 and xf[0].args["xf.scale"].shape == (1024,)


@pytest.mark.parametrize("kind", S.NET_MUTATIONS)
def test_mutated_network_tape_is_rejected(uresnet_run, kind):
    r, _ = uresnet_run
    tape, what = S.mutate(r["tape"], kind)
    with pytest.raises(AssertionError):
        r["graph"].match(tape)
    if kind in S.VALUE_MUTATIONS:
        with pytest.raises(AssertionError):
            S.replay([L for L in tape if L.op == "conv" and L.args["logsoftmax"]])
    r["graph"].match(r["tape"])          # (the graph is none the worse for the failed match)


@pytest.mark.parametrize("kind", S.STEM_MUTATIONS)
def test_mutated_stem_tape_is_rejected(monkeypatch, kind):
    r = CASES["stem_three_planes"](monkeypatch, BF)
    r["graph"].match(r["tape"])
    tape, what = S.mutate(r["tape"], kind)
    with pytest.raises(AssertionError):
        r["graph"].match(tape)


def test_a_byte_beside_a_view_of_a_big_storage_is_seen(monkeypatch):
    """a launch that writes into a storage above BIG_STORAGE keeps only the device-side verdict; one stray element turns it"""
    monkeypatch.setattr(S, "BIG_STORAGE", 64)
    from ubresnet_amd import ops
    buf = torch.zeros(4096, dtype=torch.float64)
    src = torch.arange(64, dtype=torch.float64)

    def stray(g, red):
        red[:16] += 1.0
        buf[3000] = 5.0            # outside `red`
    monkeypatch.setattr(ops, "channel_sum", stray)
    tap = S.Tap(monkeypatch, sync=lambda: None)
    ops.channel_sum(torch.zeros((1, 1, 1, 16), dtype=BF), buf[1024:1024 + 16 * kref.STAT_SLOTS])
    rec = tap.tape[0].args["red"]
    assert rec.big and rec.base_after is None and rec.outside == (1, 3000) and rec.base_init.numel() == 4096
    with pytest.raises(AssertionError, match="outside its output"):
        S._check_untouched(0, tap.tape[0])
