"""BatchStager(detector=DetectorEffects(...)) on the device, at 4 x 1 x 64 x 64 with synthetic loaders: batch `seq` is the
reference of tests/det_ref.py applied to the un-detected batch `seq` under detector.table(seq, ...) -- bit for bit with dead
wires and gain only, within the derived bound with noise -- on the plain path and on the Augment path, whatever the thread
count; PixelWeights counts the labels after masking; a skip-resume continues bitwise; without a detector the stager is what it
was; epoch.train runs over detected batches.  The host half is tests/test_cpu_det.py."""
import math

import numpy as np
import pytest
import torch

import augment_ref as AR
import det_ref as R
import oracle.uresnet_oracle as O
from ubresnet_amd import synthetic
from ubresnet_amd.augment import Augment
from ubresnet_amd.detector import DetectorEffects

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.pixel_weights import PixelWeights
    from ubresnet_amd.staging import BatchStager
    from ubresnet_amd.training import epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

B, P, H, W = 4, 1, 64, 64
AUG = dict(pad=4, seed=11)
QUIET = dict(dead_runs=(1, 3), run_len=(1, 20), gain=(0.9, 1.1), dead_label=0, dead_weight=0.0, seed=21)
NOISY = dict(QUIET, noise_sigma=1.5)
_PLAIN = {}
_NOISY_FIRST = {}           # (augment, seq) -> the noisy image as the first thread count staged it


def _plain(seq, augment):
    """the un-detected batch `seq` (image, label int64, weight), computed once per path and left unchanged"""
    key = (seq, augment)
    if key not in _PLAIN:
        x, lab, wgt = synthetic.make_batch(B, H, W, 1000 + B * seq)
        if augment:
            a = Augment(**AUG)
            x, lab, wgt = AR.reference(x, lab.astype(np.float32), wgt, a.params(seq, B), a.pad, pad_label=a.pad_label, pad_weight=a.pad_weight)
        _PLAIN[key] = (x, lab.astype(np.int64), wgt)
    return _PLAIN[key]


def _want(seq, augment, det):
    x, lab, wgt = _plain(seq, augment)
    d = DetectorEffects(**det)
    return R.reference(x, lab, wgt, d.table(seq, B, P, W), d.noise_sigma, d.noise_on == "all", d.seed, seq, d.dead_label, d.dead_weight)


def _stager(det=None, augment=False, loader=None, **kw):
    ld = loader
    if ld is None:
        ld = synthetic.SyntheticLArCVDataset(height=H, width=W, tag="train", nentries=64)
        ld.start(B)
    if det is not None:
        kw["detector"] = DetectorEffects(**det)
    return BatchStager(ld, B, H, W, tag="train", timeout=20.0, augment=Augment(**AUG) if augment else None, **kw)


def _same(got, ref, what):
    """a staged batch against reference(): label and weight bit for bit, the image by det_ref.compare; -> worst error / bound"""
    adc, label, weight = got
    assert adc.is_cuda and adc.is_contiguous() and tuple(adc.shape) == (B, P, H, W) and adc.dtype == torch.float32, what
    assert label.dtype == torch.int64 and weight.dtype == torch.float32, what
    assert np.array_equal(label.cpu().numpy(), ref["label"]), "%s: label differs" % what
    assert np.array_equal(weight.cpu().numpy().view(np.int32), ref["weight"].view(np.int32)), "%s: weight differs" % what
    return R.compare(adc.cpu().numpy(), ref)


def test_without_a_detector_the_stager_is_what_it_was():
    for augment in (False, True):
        with _stager(augment=augment) as a, _stager(augment=augment, detector=None) as b:
            assert a.detector is None and b.detector is None and all(s.table is None for s in b._slots)
            for seq in range(3):
                x, y = a.next(), b.next()
                torch.cuda.synchronize()
                assert all(torch.equal(p, q) for p, q in zip(x, y))
                want = _plain(seq, augment)
                assert all(np.array_equal(p.cpu().numpy(), q) for p, q in zip(x, want))


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
@pytest.mark.parametrize("threads", [1, 2, 4])
def test_dead_wires_and_gain_are_the_reference_bit_for_bit(threads, augment):
    held = []
    with _stager(QUIET, augment, threads=threads) as st:
        for seq in range(5):                                 # every slot comes round again
            got = st.next()
            torch.cuda.synchronize()
            ref = _want(seq, augment, QUIET)
            assert not ref["noisy"].any() and ref["dead_all"].any()
            assert _same(got, ref, "threads=%d batch %d" % (threads, seq)) == 0.0
            held.append(got)
    for seq, got in enumerate(held):                         # earlier batches after every later next()
        _same(got, _want(seq, augment, QUIET), "held batch %d" % seq)
    ref, plain = _want(0, augment, QUIET), _plain(0, augment)
    assert not np.array_equal(ref["exact"], plain[0]) and (ref["weight"] == 0.0).sum() > (plain[2] == 0.0).sum()


@pytest.mark.parametrize(("augment", "threads"), [(False, 2), (True, 2), (True, 4), (False, 1)],
                         ids=["plain", "augment", "augment-4-threads", "plain-1-thread"])
def test_noise_is_within_the_bound_of_the_reference(augment, threads):
    worst = 0.0
    with _stager(NOISY, augment, threads=threads) as st:
        for seq in range(3):
            ref = _want(seq, augment, NOISY)
            assert ref["noisy"].any() and not ref["noisy"].all()
            got = st.next()
            worst = max(worst, _same(got, ref, "batch %d" % seq))
            first = _NOISY_FIRST.setdefault((augment, seq), got[0].cpu())
            assert torch.equal(first.view(torch.int32), got[0].cpu().view(torch.int32)), "the noise depends on the thread count"
    assert 0.0 < worst <= 1.0
    print("staged noise (%s, %d threads): worst error / bound %.3f" % ("augment" if augment else "plain", threads, worst))
    with _stager(dict(NOISY, noise_on="all")) as st:
        ref = _want(0, False, dict(NOISY, noise_on="all"))
        assert np.array_equal(ref["noisy"], ~np.broadcast_to(R.unpack_table(DetectorEffects(**NOISY).table(0, B, P, W), W)[1][:, :, None, :],
                                                            ref["noisy"].shape))
        _same(st.next(), ref, "noise on all")


class _NoWeight(object):
    def __init__(self, inner):
        self.inner = inner

    def __getitem__(self, idx):
        return {k: v for k, v in self.inner[idx].items() if not k.startswith("weight_")}


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
def test_pixel_weights_count_the_labels_after_masking(augment):
    det = dict(QUIET, dead_label=2, dead_weight=None, dead_runs=(2, 4))     # dead wires become class 2: the counts must show them
    ld = synthetic.SyntheticLArCVDataset(height=H, width=W, tag="train", nentries=64)
    ld.start(B)
    with _stager(det, augment, loader=_NoWeight(ld), weights=PixelWeights(num_classes=3)) as st:
        for seq in range(2):
            adc, label, weight = st.next()
            torch.cuda.synchronize()
            ref = _want(seq, augment, det)
            assert np.array_equal(label.cpu().numpy(), ref["label"])
            counts = st.counts.cpu().numpy()
            want = np.stack([np.bincount(ref["label"][i].reshape(-1), minlength=16)[:16] for i in range(B)])
            assert np.array_equal(counts, want)
            before = np.stack([np.bincount(_plain(seq, augment)[1][i].reshape(-1), minlength=16)[:16] for i in range(B)])
            assert not np.array_equal(want, before)
            assert (weight.cpu().numpy()[ref["label"] == 2] > 0).all()              # and the weights are made from those counts


def test_skip_resume_continues_bitwise():
    with _stager(NOISY, True) as st:
        for seq in range(3):
            st.next()
        after = [st.next() for _ in range(2)]
        torch.cuda.synchronize()
    with _stager(NOISY, True) as st:
        st.skip(3)
        resumed = [st.next() for _ in range(2)]
        torch.cuda.synchronize()
    with _stager(NOISY, True) as st:                         # skip after the stager has begun: the staged batch is skipped first
        st.next()
        st.skip(2)
        late = st.next()
        torch.cuda.synchronize()
    for i in range(2):
        assert all(torch.equal(a, b) for a, b in zip(after[i], resumed[i]))
        _same(resumed[i], _want(3 + i, True, NOISY), "resumed batch %d" % (3 + i))
    assert all(torch.equal(a, b) for a, b in zip(after[0], late))


def test_epoch_train_runs_over_detected_batches():
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
    m = m.cuda()
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
    lines = []
    with _stager(NOISY, True) as st:
        out = epoch.train(st, m, PixelWiseNLLLoss(), opt, 3, iiter=1, print_freq=1, log=lines.append)
    torch.cuda.synchronize()
    assert math.isfinite(out[0]) and out[0] > 0.0 and 0.0 <= out[1] <= 100.0
    assert all(torch.isfinite(p).all() for p in m.parameters())


def test_a_detector_needs_the_device_stage():
    ld = synthetic.SyntheticLArCVDataset(height=H, width=W, tag="train", nentries=8)
    ld.start(B)
    with pytest.raises(ValueError, match="device=None"):
        BatchStager(ld, B, H, W, device=None, pin=False, detector=DetectorEffects(**QUIET))
