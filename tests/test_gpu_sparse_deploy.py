"""Sparse event I/O through the deployment surface (GPU): WholeViewSegmenter(output="pixels") and a SparseEvent as input, with seeded
models from the oracle, a 3 x 1 x 96 x 160 view, tiles of 64 x 96 and batch 4, fp32 and f16 compute.  The pixel list expanded is
the products of a segmenter with the same settings, byte for byte -- plain, with a flip view, with margin and blend, and for a
stacked ASPP_ResNet; read() is the lit mask's nonzero in order; a SparseEvent gives what its dense view gives for every output;
a second event leaves nothing of the first in the reused buffers; a short capacity overflows and the count still tells; and the
dense-in / products-out path is the one ubp_stitch_products launch per chunk it was.  Every comparison is on bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import uresnet_oracle as O

if torch.cuda.is_available():
    from ubresnet_amd import deploy, sparse

P, ROWS, COLS, TH, TW, BATCH = 3, 96, 160, 64, 96, 4
THR = 10.0
_CACHE = {}


def _uresnet():
    if "uresnet" not in _CACHE:
        sd = O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42)
        _CACHE["uresnet"] = deploy.load_model(None, "cuda:0", num_classes=3, state_dict=sd)
    return _CACHE["uresnet"]


def _aspp():
    if "aspp" not in _CACHE:
        sd = O.seeded_state_dict(O.aspp_resnet_schema(3, 3, 16), 42)
        _CACHE["aspp"] = deploy.load_model(None, "cuda:0", num_classes=3, input_channels=3, state_dict=sd, arch="aspp")
    return _CACHE["aspp"]


def _view(seed=21):
    """a tenth of the pixels carry charge, as on a wire plane, most of it above the threshold of the lit test"""
    if ("view", seed) not in _CACHE:
        rs = np.random.RandomState(seed)
        v = (rs.rand(P, 1, ROWS, COLS) * (rs.rand(P, 1, ROWS, COLS) > 0.9) * 100.0).astype(np.float32)
        _CACHE[("view", seed)] = torch.from_numpy(v).cuda()
    return _CACHE[("view", seed)]


def _segmenter(model, dtype=torch.float32, **kw):
    return deploy.WholeViewSegmenter(model, ROWS, COLS, planes=P, tile=(TH, TW), batch=BATCH, dtype=dtype, **kw)


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()]).cpu().numpy()


def _same_products(a, b, what):
    for x, y, field in zip(a, b, ("label", "confidence", "counts")):
        assert x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape), (what, field, x.shape, y.shape)
        assert np.array_equal(_bits(x), _bits(y)), "%s: %s differs" % (what, field)


def _lit(view, stacked):
    lit = view[:, 0] > THR
    return lit.any(dim=0, keepdim=True) if stacked else lit


SETTINGS = {
    "plain": dict(),
    "tta": dict(tta=("cols",)),
    "blend": dict(margin=8, blend="linear"),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_pixels_expanded_are_the_products(setting, dtype):
    view = _view()
    want = _segmenter(_uresnet(), dtype, output="products", **SETTINGS[setting])(view)
    seg = _segmenter(_uresnet(), dtype, output="pixels", **SETTINGS[setting])
    pl = seg(view)
    assert isinstance(pl, sparse.PixelList) and (pl.planes, pl.rows, pl.cols, pl.fill_label) == (P, ROWS, COLS, 255)
    assert pl.capacity == P * ROWS * COLS and pl.index.is_cuda and pl.count.is_cuda
    _same_products(pl.to_products(), want, setting)
    # read(): the lit mask's nonzero, in order, with the products' label and confidence there
    lit = _lit(view, False).reshape(-1)
    where = torch.nonzero(lit).reshape(-1)
    index, label, conf = pl.read()
    assert int(pl.count) == where.numel() > 100 and index.dtype == torch.int32 and not index.is_cuda
    assert np.array_equal(index.numpy(), where.cpu().numpy().astype(np.int32))
    assert np.array_equal(label.numpy(), want.label.reshape(-1)[where].cpu().numpy())
    assert np.array_equal(_bits(conf), _bits(want.confidence.reshape(-1)[where]))
    assert int((want.label.reshape(-1)[~lit] != 255).sum()) == 0


def test_pixels_of_a_stacked_model():
    view = _view()
    want = _segmenter(_aspp(), output="products")(view)
    pl = _segmenter(_aspp(), output="pixels")(view)
    assert (pl.planes, pl.capacity) == (1, ROWS * COLS) and tuple(pl.counts.shape) == (3,)
    _same_products(pl.to_products(), want, "stacked")
    where = torch.nonzero(_lit(view, True).reshape(-1)).reshape(-1)
    assert np.array_equal(pl.read()[0].numpy(), where.cpu().numpy().astype(np.int32)) and where.numel() > 100


@pytest.mark.parametrize("output", ["scores", "products", "pixels"])
def test_a_sparse_event_is_its_dense_view(output):
    view = _view().clone()
    flat = view.reshape(-1)
    flat[5], flat[77] = float("nan"), -0.0                       # a list keeps both: neither has the bits of +0.0
    event = sparse.SparseEvent.from_dense(view).validate()
    assert 0.05 < event.n / view.numel() < 0.2 and not event.index.is_cuda
    dense = _segmenter(_uresnet(), output=output)(view)
    seg = _segmenter(_uresnet(), output=output)
    got = seg(event)
    assert np.array_equal(_bits(seg._view_buf), _bits(view)), "the scattered view is not the dense one"
    assert int(seg.status) == 0
    if output == "scores":
        assert np.array_equal(_bits(got), _bits(dense))
    elif output == "products":
        _same_products(got, dense, "sparse in, products out")
    else:
        for x, y in zip(got.read(), dense.read()):
            assert np.array_equal(_bits(x), _bits(y))
        _same_products(got.to_products(), dense.to_products(), "sparse in, pixels out")
    # the same list from pinned memory and from the device
    pinned = sparse.SparseEvent(event.index.pin_memory(), event.value.pin_memory(), P, ROWS, COLS)
    on_dev = sparse.SparseEvent(event.index.cuda(), event.value.cuda(), P, ROWS, COLS)
    for ev in (pinned, on_dev):
        seg(ev)
        assert np.array_equal(_bits(seg._view_buf), _bits(view))


def test_a_second_event_leaves_nothing_of_the_first():
    seg = _segmenter(_uresnet(), output="pixels")
    first, second = _view(21), _view(22)
    pl = seg(sparse.SparseEvent.from_dense(first))
    ptrs = (seg._view_buf.data_ptr(), pl.index.data_ptr(), pl.label.data_ptr(), pl.confidence.data_ptr(), pl.count.data_ptr(),
            seg._compactor.scratch.data_ptr(), seg._pix_dense[0].data_ptr())
    n1 = int(pl.count)
    # a short second event: fewer entries in and fewer lit pixels out than the first left in the buffers
    short = second.clone()
    short[:, :, ROWS // 2:] = 0
    pl2 = seg(sparse.SparseEvent.from_dense(short))
    assert ptrs == (seg._view_buf.data_ptr(), pl2.index.data_ptr(), pl2.label.data_ptr(), pl2.confidence.data_ptr(), pl2.count.data_ptr(),
                    seg._compactor.scratch.data_ptr(), seg._pix_dense[0].data_ptr()), "view, output and scratch buffers are reused"
    assert 0 < int(pl2.count) < n1 and np.array_equal(_bits(seg._view_buf), _bits(short))
    want = _segmenter(_uresnet(), output="products")(short)
    _same_products(pl2.to_products(), want, "second event")
    assert np.array_equal(pl2.read()[0].numpy(), torch.nonzero(_lit(short, False).reshape(-1)).reshape(-1).cpu().numpy().astype(np.int32))
    assert int(seg.status) == 0


def test_a_short_capacity_overflows_and_the_count_still_tells():
    view = _view()
    total = int((_lit(view, False)).sum())
    seg = _segmenter(_uresnet(), output="pixels", capacity=total - 1)
    pl = seg(view)
    assert pl.capacity == total - 1 and int(pl.count) == total
    with pytest.raises(OverflowError, match="%d lit pixels, capacity %d" % (total, total - 1)):
        pl.read()
    full = _segmenter(_uresnet(), output="pixels", capacity=total)(view)
    index = full.read()[0]
    assert index.numel() == total and np.array_equal(_bits(pl.index), _bits(full.index[:total - 1])), "the entries that fit are the first ones"
    # an invalid list is counted, not written
    bad = sparse.SparseEvent(torch.tensor([7, 7, 3, P * ROWS * COLS], dtype=torch.int32), torch.ones(4), P, ROWS, COLS)
    with pytest.raises(ValueError):
        bad.validate()
    seg(bad)
    assert int(seg.status) == 3


def test_dense_in_products_out_is_the_path_it_was(monkeypatch):
    """the products of a dense view are what _stitch_products, called directly on the per-chunk scores, writes; no call of the new
    library is made on that path"""
    from ubresnet_amd import _sparse as Z
    view = _view()
    seg = _segmenter(_uresnet(), output="products")
    calls = []
    real = deploy._stitch_products
    monkeypatch.setattr(deploy, "_stitch_products", lambda *a, **k: (calls.append((a[4], a[1:4], a[6:9], a[10:])), real(*a, **k))[1])
    for f in ("scatter_view", "compact", "expand"):
        monkeypatch.setattr(Z, f, lambda *a, **k: pytest.fail("the sparse library was called on the dense path"))
    got = seg(view)
    monkeypatch.undo()
    chunks = [seg.tiles[i:i + BATCH] for i in range(0, len(seg.tiles), BATCH)]
    assert [c[0] for c in calls] == chunks and all(c[1:] == ((3, TH, TW), (1, THR, 255), (P, ROWS, COLS)) for c in calls)
    assert seg._compactor is None and seg._view_buf is None and seg.status is None and seg._pix_dense is None
    # the same launches by hand: the scores of every chunk from a scores segmenter's stitch inputs
    want = deploy.Products(torch.empty((P, ROWS, COLS), dtype=torch.uint8, device="cuda"),
                           torch.empty((P, ROWS, COLS), dtype=torch.float16, device="cuda"),
                           torch.zeros((P, 3), dtype=torch.int64, device="cuda"))
    lib = deploy.L.lib()
    for chunk in chunks:
        deploy.L.check(lib.ubr_crop_tiles(view.data_ptr(), P, ROWS, COLS, deploy._desc7(chunk), len(chunk), TH, TW, seg._static_in.data_ptr(),
                                          deploy.L.stream_ptr()), "crop_tiles")
        seg._graph.replay()
        deploy._stitch_products(seg._static_out, 3, TH, TW, chunk, view, 1, THR, 255, want, P, ROWS, COLS)
    _same_products(got, want, "dense in, products out")
