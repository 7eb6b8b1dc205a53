"""ubq_score_event (libubresnet_score.so) and EventScorer on the device, every table compared whole and for equality with the
numpy reference of tests/score_ref.py.  CASES is the module's table -- score_ref.KERNEL_CASES, one entry per compiled kernel --
and tests/test_cpu_score.py holds it against the library's symbol table and against the case ids below."""
import numpy as np
import pytest
import torch

import score_ref as R

pytestmark = pytest.mark.gpu

CASES = R.KERNEL_CASES
FILL = 255

if torch.cuda.is_available():
    from ubresnet_amd import _score as S
    from ubresnet_amd import deploy, metrics, scoring, synthetic


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _run(case, label, conf, truth, Cn, radius, lo, edges, fill=FILL, seed=1, dev=None):
    """one ubq_score_event into a table that already holds counts above 2^32, twice: both tables equal the reference, word for
    word; `case` is the id in CASES, which also fixes the truth type.  `dev`: device tensors to use instead of uploads."""
    assert any(case in ids for ids in CASES.values()), "case %r is not in the table" % case
    kind = R.KIND_OF_CASE[case]
    assert truth.dtype == R.KIND_DTYPE[kind]
    P, rows, cols = label.shape
    bins = len(edges) + 1
    n = R.words(P, Cn, bins)
    assert S.table_words(P, Cn, bins) == n
    table0 = R.prefill(seed, n)
    ref = R.reference(label, conf, truth, Cn, fill, radius, lo, edges, table0)
    dl, dc, dt = dev if dev is not None else (_dev(label), _dev(conf), _dev(truth))
    got = []
    for _ in range(2):
        tab = _dev(table0)
        S.score_event(dl.data_ptr(), dc.data_ptr(), dt.data_ptr(), kind, Cn, fill, radius, lo, S.edges_array(edges), bins,
                      tab.data_ptr(), P, rows, cols, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got.append(tab.cpu().numpy().view(np.uint64))
    what = "%s C=%d bins=%d radius=%d from=%d %dx%dx%d" % (case, Cn, bins, radius, lo, P, rows, cols)
    assert np.array_equal(got[0], ref), what
    assert np.array_equal(got[1], got[0]), what + ": the second run differs"
    return R.unpack(ref - table0, P, Cn, bins)


@pytest.mark.parametrize(("case", "Cn"), [("grid-C1-u8", 1), ("grid-C3-u8", 3), ("grid-C16-u8", 16),
                                           ("grid-C1-i64", 1), ("grid-C3-i64", 3), ("grid-C16-i64", 16)])
def test_parameter_grid_on_the_base_shapes(case, Cn):
    """bins x radius x interface_from on a view of two tiles and a ragged one each way, with element loads (150 columns) and
    4-pixel loads (152); the inputs hold every listed confidence pattern, the edges and their neighbours, and bad truths / labels"""
    kind = R.KIND_OF_CASE[case]
    for shape in R.BASE_SHAPES:
        for bins in R.GRID_BINS:
            edges = R.equal_edges(bins)
            label, conf, truth = R.make_event(100 + Cn, *shape, Cn, kind, edges=edges)
            dev = (_dev(label), _dev(conf), _dev(truth))
            for radius in R.GRID_RADII:
                for lo in sorted(set([0, 1, Cn])):
                    cf, rel, tally = _run(case, label, conf, truth, Cn, radius, lo, edges, seed=bins + radius, dev=dev)
                    assert int(tally[:, :2].sum()) == int((label != FILL).sum())
                    if radius == 0 or lo == Cn:
                        assert cf[:, 1].sum() == 0 and rel[:, 1].sum() == 0
                    elif Cn >= 3:
                        assert (cf[:, 1].sum((1, 2)) > 0).all()


@pytest.mark.parametrize("case", ["one-pixel-u8", "one-pixel-i64"])
def test_a_view_of_one_pixel(case):
    dt = R.KIND_DTYPE[R.KIND_OF_CASE[case]]
    for lab, tr, h, want in ((1, 1, 0x3C00, [1, 0, 0, 0]), (0, 1, 0x3400, [1, 0, 0, 0]), (FILL, 2, 0, [0, 0, 1, 0]), (FILL, 0, 0, [0, 0, 0, 0]),
                             (2, 3, 0x3C00, [0, 1, 0, 0]), (3, 0, 0x3C00, [0, 1, 0, 0]), (1, 2, 0x7C00, [1, 0, 0, 1])):
        cf, rel, tally = _run(case, np.array([[[lab]]], np.uint8), np.array([[[h]]], np.uint16), np.array([[[tr]]], dt), 3, 8, 1,
                              R.equal_edges(10))
        assert tally.tolist() == [want] and int(cf[:, 1].sum()) == 0 and int(cf.sum()) == want[0]


@pytest.mark.parametrize("case", ["narrow-u8", "narrow-i64"])
def test_views_narrower_than_the_radius(case):
    kind = R.KIND_OF_CASE[case]
    edges = R.equal_edges(10)
    for shape in ((2, 40, 3), (2, 5, 140), (3, 4, 4)):
        label, conf, truth = R.make_event(12, *shape, 3, kind, edges=edges)
        for radius in (2, 8):
            cf, _, _ = _run(case, label, conf, truth, 3, radius, 1, edges)
            assert cf[:, 1].sum() > 0


def _blank(P, rows, cols, kind):
    return (np.full((P, rows, cols), 0, np.uint8), np.full((P, rows, cols), 0x3800, np.uint16),
            np.zeros((P, rows, cols), R.KIND_DTYPE[kind]))


@pytest.mark.parametrize("case", ["contacts-u8", "contacts-i64"])
def test_contacts_across_tile_borders_and_at_the_view_edges(case):
    """C = 4, interface_from = 2: classes 0 and 1 never make a contact, 2 and 3 do; every pixel is lit unless said"""
    kind = R.KIND_OF_CASE[case]
    TH, TW = R.TILE_H, R.TILE_W
    rows, cols = 2 * TH + 5, 2 * TW + 22
    edges = R.equal_edges(4)

    def pairs(radius):
        """(y, x) of a class-2 pixel and of the class-3 pixel that touches it at this radius, and nothing else within reach"""
        return [((5, TW - 1), (5, TW - 1 + radius)),                      # across a vertical tile border
                ((TH - 1, 40), (TH - 1 + radius, 40)),                    # across a horizontal one
                ((TH - 1, 2 * TW - 1), (TH - 1 + radius, 2 * TW - 1 + radius)),   # across a tile corner, diagonally
                ((0, 0), (radius, radius)),                               # the view's corners and edges: the window is clipped
                ((0, cols - 1), (radius, cols - 1 - radius)),
                ((rows - 1, 0), (rows - 1 - radius, radius)),
                ((rows - 1, cols - 1), (rows - 1, cols - 1 - radius)),
                ((TH + 10, 0), (TH + 10 + radius, 0)),
                ((0, TW + 30), (0, TW + 30 + radius))]

    for radius in (1, 2, 8):
        label, conf, truth = _blank(1, rows, cols, kind)
        for a, b in pairs(radius):
            truth[0][a], truth[0][b] = 2, 3
            label[0][a], label[0][b] = 2, 2
        # just out of reach: no contact
        truth[0, 50, 60], truth[0, 50, 60 + radius + 1] = 2, 3
        # a contact made only by an unlit neighbour
        truth[0, 20, 60], truth[0, 20 + radius, 60] = 3, 2
        label[0, 20 + radius, 60] = FILL
        # two different classes below interface_from: no contact; and a class below next to one above: none either
        truth[0, 40, 200], truth[0, 40, 201] = 1, 0
        truth[0, 45, 200], truth[0, 45, 201] = 1, 2
        cf, rel, tally = _run(case, label, conf, truth, 4, radius, 2, edges)
        n = len(pairs(radius))
        assert int(cf[0, 1].sum()) == 2 * n + 1 and cf[0, 1, 2, 2] == n and cf[0, 1, 3, 2] == n and cf[0, 1, 3, 0] == 1
        assert int(tally[0, 2]) == 1 and int(tally[0, 0]) == rows * cols - 1
        # one class less in reach: the same picture at a smaller radius loses every contact
        if radius > 1:
            cf, _, _ = _run(case, label, conf, truth, 4, radius - 1, 2, edges)
            assert int(cf[0, 1].sum()) == 0


@pytest.mark.parametrize("case", ["all-unlit-u8", "all-unlit-i64"])
def test_an_unlit_event_moves_only_the_dark_tally(case):
    kind = R.KIND_OF_CASE[case]
    label, conf, truth = R.make_event(9, 2, 37, 150, 3, kind)
    label[:] = FILL
    cf, rel, tally = _run(case, label, conf, truth, 3, 2, 1, R.equal_edges(10))
    assert cf.sum() == 0 and rel.sum() == 0 and (tally[:, [0, 1, 3]] == 0).all()
    assert tally[:, 2].tolist() == [int(((truth[p] >= 1) & (truth[p] < 3)).sum()) for p in range(2)] and (tally[:, 2] > 0).all()


@pytest.mark.parametrize("case", ["all-lit-u8", "all-lit-i64"])
def test_an_all_lit_single_class_single_bin_event(case):
    """the contended path: every lane of every wave adds to the same three counters"""
    kind = R.KIND_OF_CASE[case]
    for shape in ((2, 37, 150), (1, 70, 256)):
        label, conf, truth = _blank(*shape, kind)
        conf[:] = 0x3BFF
        cf, rel, tally = _run(case, label, conf, truth, 1, 2, 1, [])
        n = shape[1] * shape[2]
        assert (cf[:, 0, 0, 0] == n).all() and (rel[:, 0, 0] == [n, n, n * int(R.fix(0x3BFF))]).all() and (tally[:, 0] == n).all()


@pytest.mark.parametrize("case", ["misaligned-u8", "misaligned-i64"])
def test_buffers_that_start_off_the_vector_alignment(case):
    """152 columns would take the 4-pixel loads; label and confidence that start one element into their allocation cannot"""
    kind = R.KIND_OF_CASE[case]
    edges = R.equal_edges(10)
    label, conf, truth = R.make_event(11, 2, 37, 152, 3, kind, edges=edges)

    def off(a, k):
        flat = torch.zeros(a.size + 8, dtype=_dev(a[:1, :1, :1]).dtype, device="cuda")
        flat[k:k + a.size] = _dev(a).reshape(-1)
        return flat[k:k + a.size].view(a.shape)

    for kl, kc in ((1, 0), (0, 1), (2, 2), (3, 3)):
        _run(case, label, conf, truth, 3, 2, 1, edges, dev=(off(label, kl), off(conf, kc), _dev(truth)))


@pytest.mark.parametrize("case", ["many-tiles-u8", "many-tiles-i64"])
def test_a_plane_of_more_tiles_than_workgroups(case):
    """306 tiles for at most 256 workgroups: some walk two tiles and count both into one LDS table"""
    P, rows, cols = R.MANY_TILES_SHAPE
    assert -(-rows // R.TILE_H) * -(-cols // R.TILE_W) > R.GRID_X
    edges = R.equal_edges(10)
    label, conf, truth = R.make_event(21, P, rows, cols, 3, R.KIND_OF_CASE[case], edges=edges)
    for radius, lo in ((2, 1), (8, 0)):
        cf, rel, tally = _run(case, label, conf, truth, 3, radius, lo, edges)
        assert (cf.sum((0, 2, 3)) > 0).all() and (tally > 0).all()


@pytest.mark.parametrize("case", ["values-u8", "values-i64"])
def test_confidence_patterns_and_truth_values_one_by_one(case):
    """a lit, rightly labelled pixel per listed pattern, per edge and per neighbour of an edge; then one pixel per truth value
    that is no class -- 2^40 + 1 narrows to class 1 and must still be ignored"""
    kind = R.KIND_OF_CASE[case]
    edges = R.equal_edges(10)
    bits = list(R.CONF_BITS) + [v for e in edges for v in (e - 1, e, e + 1)]
    label, conf, truth = _blank(1, 3, len(bits), kind)
    label[0, 1:] = FILL
    truth[0, 0], label[0, 0] = 1, 1
    conf[0, 0] = bits
    cf, rel, tally = _run(case, label, conf, truth, 3, 0, 1, edges)
    assert int(tally[0, 3]) == 3 and int(tally[0, 0]) == len(bits)           # 0x7C00, 0x7E00 and 0xBC00 are not binned
    assert int(rel[0, 0, :, 0].sum()) == len(bits) - 3
    for i, e in enumerate(edges):                                            # e - 1 falls below the edge, e and e + 1 do not
        one = np.zeros((1, 1, 1), np.uint16)
        for h, b in ((e - 1, i), (e, i + 1), (e + 1, i + 1)):
            one[:] = h
            _, r, _ = _run(case, label[:, :1, :1], one, truth[:, :1, :1], 3, 0, 1, edges)
            assert r[0, 0, b].tolist() == [1, 1, int(R.fix(h))], (hex(h), b)
    bad = R.bad_truths(kind, 3)
    label, conf, truth = _blank(1, 2, len(bad), kind)
    truth[0, 0], truth[0, 1] = bad, bad
    label[0, 0], label[0, 1] = 1, FILL
    cf, rel, tally = _run(case, label, conf, truth, 3, 2, 0, edges)
    assert tally.tolist() == [[0, len(bad), 0, 0]] and cf.sum() == 0 and rel.sum() == 0


def test_event_scorer_rows_and_the_bytes_around_them():
    """three events into rows 0..2 of a table of four: each row is its event's reference, row 3 stays zero; a full table raises,
    reset() clears it; uint8 and int64 truths of the same event give the same row"""
    P, rows, cols, Cn = 2, 37, 150, 4
    sc = scoring.EventScorer(num_classes=Cn, planes=P, bins=10, radius=2, interface_from=1, capacity=4)
    zero = np.zeros(sc.words, np.uint64)
    want = []
    for n in range(3):
        label, conf, truth = R.make_event(40 + n, P, rows, cols, Cn, R.I64, edges=sc.edges)
        sc.add(deploy.Products(_dev(label), _dev(conf).view(torch.float16), None), _dev(truth))
        want.append(R.reference(label, conf, truth, Cn, FILL, 2, 1, sc.edges, zero))
    raw = sc._table.cpu().numpy().view(np.uint64)
    assert np.array_equal(raw[:3], np.stack(want)) and not raw[3].any()
    score = sc.read()
    assert score.events == 3 and np.array_equal(score.tables, np.stack(want))
    total = np.stack(want).astype(object).sum(0)
    assert [int(v) for v in score.total] == [int(v) for v in total]
    u8 = np.where((truth >= 0) & (truth < 256), truth, 255).astype(np.uint8)       # the same classes: no value below Cn is made or lost
    sc.add((_dev(label), _dev(conf).view(torch.float16)), _dev(u8))
    assert np.array_equal(sc.read().tables[3], want[2])
    with pytest.raises(RuntimeError, match="table is full"):
        sc.add((_dev(label), _dev(conf).view(torch.float16)), _dev(u8))
    with pytest.raises(ValueError, match=r"label must be \[2, rows, cols\]"):
        sc.add((_dev(label)[:1], _dev(conf).view(torch.float16)[:1]), _dev(u8)[:1])
    sc.reset()
    assert sc.events == 0 and sc.read().events == 0 and not sc._table.cpu().numpy().any()
    sc.add((_dev(label), _dev(conf).view(torch.float16)), _dev(u8))
    assert np.array_equal(sc.read().tables[0], want[2])


@pytest.mark.parametrize("tta", [None, ("cols",)], ids=["plain", "tta-cols"])
def test_end_to_end_whole_view_products(tta):
    """a seeded ip16 UResNet through WholeViewSegmenter(output="products") at 64 x 96 tiles on a 96 x 160 view, synthetic truth"""
    from oracle import uresnet_oracle as O
    from ubresnet_amd.models.ub_uresnet import UResNet
    P, rows, cols, Cn = 3, 96, 160, 3
    m = UResNet(num_classes=Cn, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(Cn, 1, 16, 16), 42))
    m = m.cuda().eval()
    x, lab, _ = synthetic.make_batch(P, rows, cols, 1000)
    view, truth = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    seg = deploy.WholeViewSegmenter(m, rows, cols, planes=P, tile=(64, 96), batch=4, dtype=torch.float32, output="products", tta=tta)
    prod = seg(view)
    sc = scoring.EventScorer(num_classes=Cn, planes=P, bins=10, radius=2, interface_from=1)
    sc.add(prod, truth)
    score = sc.read()
    label, conf = prod.label.cpu().numpy(), prod.confidence.cpu().view(torch.int16).numpy().view(np.uint16)
    ref = R.reference(label, conf, lab, Cn, FILL, 2, 1, sc.edges, np.zeros(sc.words, np.uint64))
    assert np.array_equal(score.tables[0], ref)
    t = score.tallies()
    lit = int((label != FILL).sum())
    assert t["scored"] + t["ignored"] == lit and 0 < lit < P * rows * cols
    assert int(prod.counts.sum()) == lit
    cm = torch.from_numpy(R.unpack(ref, P, Cn, 10)[0].astype(np.int64).sum((0, 1)))
    assert torch.equal(score.confusion(), cm) and int(cm.sum()) == t["scored"]
    assert score.accuracy() == metrics.accuracy_from_confusion(cm, track_shower=True) and score.iou() == metrics.iou(cm)
    print(score)
