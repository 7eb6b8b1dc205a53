"""ubresnet_amd.crops on the device: EventCropStager batches against the reference of tests/crop_ref.py composed on the host,
sparse events in against dense ones, seeds, PixelWeights and DetectorEffects in BatchStager's order against calling them by hand,
and three epoch.train steps fed by the stager against the same batches fed as plain tensors.  View 96 x 160, crops 64 x 64 (cell
32: two by four positions), four crops per event.  Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

import crop_ref as R
import oracle.uresnet_oracle as O
from ubresnet_amd import synthetic

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import crops
    from ubresnet_amd.detector import DetectorEffects
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.pixel_weights import PixelWeights
    from ubresnet_amd.sparse import SparseEvent
    from ubresnet_amd.training import epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

P, ROWS, COLS, H, W, K = 3, 96, 160, 64, 64, 4
NEVENTS = 5
KW = dict(crop=(H, W), per_event=K, min_lit=300, tries=4, flip_rows=True, flip_cols=True, seed=77)


@pytest.fixture(scope="module")
def events():
    """(image, label) numpy pairs, made once and never changed"""
    return [synthetic.make_labelled_event(P, ROWS, COLS, 300 + 10 * i) for i in range(NEVENTS)]


def _dense(events, pin=False):
    out = []
    for image, label in events:
        i, l = torch.from_numpy(image), torch.from_numpy(label)
        out.append(crops.LabelledEvent(i.pin_memory() if pin else i, l.pin_memory() if pin else l))
    return out


def _sparse(events):
    return [crops.LabelledEvent(SparseEvent.from_dense(torch.from_numpy(image)), SparseEvent.from_dense(torch.from_numpy(label.astype(np.float32))))
            for image, label in events]


def _reference(events, number, seed=77, weight=None):
    """the batch of event `number` (events cycle) from the numpy reference -> (adc bits, label, weight bits, table)"""
    image, label = events[number % len(events)]
    g = R.largest_cell(ROWS, COLS, H, W)
    geo = R.geometry(ROWS, COLS, H, W, g)
    s = R.sat(R.counting(image, None, 0, 0, False, 10.0), g)
    table = R.choose(s, geo, g, None, K, KW["tries"], KW["min_lit"], seed, number, True, True)
    oi, ol, ow, bad = R.gather(image, label, 0, weight, False, table, H, W)
    assert bad == 0
    return oi, ol, ow, table


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _take(stager, n):
    out = []
    for _ in range(n):
        adc, label, weight = stager.next()
        out.append((adc.clone(), label.clone(), weight.clone(), stager.tables.clone()))
    torch.cuda.synchronize()
    return out


def test_stager_batches_equal_the_reference_composed_on_the_host(events):
    assert R.largest_cell(ROWS, COLS, H, W) == 32
    with crops.EventCropStager(_dense(events, pin=True), crops.EventCropper(**KW), events_per_batch=2) as st:
        got = _take(st, 4)                                       # eight events: the five cycle
        assert st.batchsize == 2 * K and st.count >= 8
    accepted = []
    for b, (adc, label, weight, tables) in enumerate(got):
        assert adc.shape == (2 * K, 1, H, W) and label.shape == weight.shape == (2 * K, H, W) and label.dtype == torch.int64
        for e in range(2):
            oi, ol, ow, table = _reference(events, 2 * b + e)
            s = slice(e * K, (e + 1) * K)
            assert np.array_equal(tables[s].cpu().numpy(), table), (b, e)
            assert np.array_equal(_bits(adc[s]), oi) and np.array_equal(label[s].cpu().numpy(), ol) and np.array_equal(_bits(weight[s]), ow)
            accepted += table[:, 5].tolist()
    assert (got[0][2] == 1.0).all() and 0 < sum(accepted), "no weight view: ones; and min_lit was met somewhere"
    assert int(st.cropper.status.item()) == 0


def test_sparse_events_give_the_bytes_of_dense_events(events):
    with crops.EventCropStager(_dense(events), crops.EventCropper(**KW)) as a, crops.EventCropStager(_sparse(events), crops.EventCropper(**KW)) as b:
        da, db = _take(a, 3), _take(b, 3)
    for x, y in zip(da, db):
        for s, t in zip(x, y):
            assert torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, t.view(torch.int32) if t.dtype == torch.float32 else t)
    assert int(b.cropper.status.item()) == 0


def test_one_seed_agrees_and_another_differs(events):
    dev = [crops.LabelledEvent(e.image.cuda(), e.label.cuda()) for e in _dense(events)]        # events on the device
    with crops.EventCropStager(_dense(events), crops.EventCropper(**KW)) as a, crops.EventCropStager(dev, crops.EventCropper(**KW)) as b, \
            crops.EventCropStager(_dense(events), crops.EventCropper(**dict(KW, seed=78))) as c:
        da, db, dc = _take(a, 3), _take(b, 3), _take(c, 3)
    for x, y in zip(da, db):
        assert all(torch.equal(s, t) for s, t in zip(x, y))
    assert any(not torch.equal(x[3], z[3]) for x, z in zip(da, dc))
    for n, z in enumerate(dc):
        assert np.array_equal(z[3].cpu().numpy(), _reference(events, n, seed=78)[3])


def test_weights_and_detector_reach_the_batch_in_batch_stagers_order(events):
    pw = PixelWeights(num_classes=3, max_weight=50.0, radius=1, gain=2.0, when="missing")
    det = DetectorEffects(dead_runs=(1, 2), run_len=(2, 6), gain=(0.8, 1.2), noise_sigma=1.0, dead_label=0, seed=9)
    with crops.EventCropStager(_dense(events), crops.EventCropper(**KW), weights=pw, detector=det) as st:
        got = _take(st, 2)
        counts = st.counts.clone()
    for seq, (adc, label, weight, tables) in enumerate(got):
        oi, ol, ow, table = _reference(events, seq)
        x = torch.from_numpy(oi.view(np.float32)).cuda()
        lab, wgt = torch.from_numpy(ol).cuda(), torch.from_numpy(ow.view(np.float32)).cuda()
        t = torch.from_numpy(det.table(seq, K, 1, W).view(np.int32)).cuda()
        det.launch(x.data_ptr(), lab.data_ptr(), wgt.data_ptr(), (K, 1, H, W), t.data_ptr(), seq, stream=torch.cuda.current_stream().cuda_stream)
        want_w = pw(lab)                                         # after the detector: the weights balance the labels as they finally are
        torch.cuda.synchronize()
        assert torch.equal(adc.view(torch.int32), x.view(torch.int32)) and torch.equal(label, lab)
        assert torch.equal(weight.view(torch.int32), want_w.view(torch.int32)) and not torch.equal(adc.view(torch.int32), torch.from_numpy(oi.view(np.int32)).cuda())
    assert counts.shape == (K, 16) and torch.equal(counts, pw.counts)
    # an event that brings its weight keeps it under when="missing"
    wv = torch.from_numpy(np.random.RandomState(3).uniform(0.5, 2.0, (P, ROWS, COLS)).astype(np.float32))
    own = [crops.LabelledEvent(e.image, e.label, wv) for e in _dense(events)]
    with crops.EventCropStager(own, crops.EventCropper(**KW), weights=pw) as st:
        (adc, label, weight, tables), = _take(st, 1)
        assert st.counts is None
    assert np.array_equal(_bits(weight), _reference(events, 0, weight=wv.numpy())[2])


class _Recorded(object):
    def __init__(self):
        self.inner, self.losses = PixelWiseNLLLoss(), []

    def forward(self, pred, label, weight):
        loss = self.inner.forward(pred, label, weight)
        self.losses.append(loss.detach().clone())
        return loss

    def flush(self):
        self.inner.flush()


class _Plain(object):
    def __init__(self, batches):
        self.batches = list(batches)

    def next(self):
        return self.batches.pop(0)


def test_three_train_steps_fed_by_the_stager_equal_plain_tensors(events):
    def run(stager):
        m = UResNet(num_classes=3, input_channels=1, inplanes=16)
        m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
        m = m.cuda()
        crit = _Recorded()
        epoch.train(stager, m, crit, FlatAdam(m, lr=1e-3), 3, nclasses=3, print_freq=10, log=lambda s: None)
        torch.cuda.synchronize()
        return torch.stack(crit.losses).cpu(), [p.detach().clone() for p in m.parameters()]

    with crops.EventCropStager(_dense(events), crops.EventCropper(**KW)) as st:
        plain = [b[:3] for b in _take(st, 3)]
    with crops.EventCropStager(_dense(events), crops.EventCropper(**KW)) as st:
        fed, params = run(st)
    flat, params2 = run(_Plain(plain))
    assert torch.isfinite(fed).all() and torch.equal(fed.view(torch.int32), flat.view(torch.int32)), (fed, flat)
    assert all(torch.equal(a, b) for a, b in zip(params, params2))
