"""BatchStager(augment=Augment(...)) on the device, at 4 x 1 x 64 x 64 with synthetic loaders: batch `seq` is exactly the numpy
reference of tests/augment_ref.py applied to loader batch `seq` under augment.params(seq, B), whatever the thread count; held
tensors stay the caller's; a skip-resume continues bitwise; epoch.train runs over augmented batches and its meters, the
track/shower one included, are those of a per-step loop.  The host half is tests/test_cpu_augment.py."""
import numpy as np
import pytest
import torch

import augment_ref as R
import oracle.uresnet_oracle as O
from ubresnet_amd import synthetic
from ubresnet_amd.augment import Augment

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd import metrics
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.staging import BatchStager
    from ubresnet_amd.training import epoch
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

B, H, W = 4, 64, 64
AUG = dict(pad=4, seed=11)
_WANT = {}


def _want(seq, weight=True, **kw):
    """the augmented batch `seq`, computed once per configuration and left unchanged"""
    key = (seq, weight, tuple(sorted(kw.items())))
    if key not in _WANT:
        x, lab, wgt = synthetic.make_batch(B, H, W, 1000 + B * seq)
        a = Augment(**AUG)
        _WANT[key] = R.reference(x, lab.astype(np.float32), wgt if weight else None, a.params(seq, B), a.pad,
                                 pad_label=a.pad_label, pad_weight=a.pad_weight, **kw)
    return _WANT[key]


def _stager(augment=True, loader=None, **kw):
    ld = loader
    if ld is None:
        ld = synthetic.SyntheticLArCVDataset(height=H, width=W, tag="train", nentries=64)
        ld.start(B)
    return BatchStager(ld, B, H, W, tag="train", timeout=20.0, augment=Augment(**AUG) if augment else None, **kw)


def _same(got, want, what):
    for name, t, a in zip(("adc", "label", "weight"), got, want):
        assert t.is_cuda and t.is_contiguous() and tuple(t.shape) == a.shape, (what, name)
        assert t.dtype == (torch.int64 if name == "label" else torch.float32), (what, name)
        assert torch.equal(t.cpu(), torch.from_numpy(a)), "%s: %s differs" % (what, name)


@pytest.mark.parametrize("threads", [1, 2])
def test_six_batches_are_the_reference_of_their_sequence_number(threads):
    held = []
    with _stager(threads=threads) as st:
        for seq in range(6):
            got = st.next()
            torch.cuda.synchronize()
            _same(got, _want(seq), "threads=%d batch %d" % (threads, seq))
            held.append(got)
        torch.cuda.synchronize()
    for seq, got in enumerate(held):                     # earlier batches after every later next()
        _same(got, _want(seq), "held batch %d" % seq)
    ptrs = [t.data_ptr() for bt in held for t in bt]
    assert len(set(ptrs)) == len(ptrs), "device memory was handed out twice while the caller held it"
    plain = synthetic.make_batch(B, H, W, 1000)
    assert not np.array_equal(_want(0)[0], plain[0]) and (_want(0)[1] >= 0).all()
    assert any((_want(s)[2] == 0.0).any() for s in range(6)), "no padding was ever cut in"


class _NoWeight(object):
    def __init__(self, inner):
        self.inner = inner

    def __getitem__(self, idx):
        return {k: v for k, v in self.inner[idx].items() if not k.startswith("weight_")}


def test_offset_threshold_and_a_wire_without_weights_reach_the_kernel():
    ld = synthetic.SyntheticLArCVDataset(height=H, width=W, tag="train", nentries=64)
    ld.start(B)
    with _stager(loader=_NoWeight(ld), label_offset=-1, adc_threshold=30.0) as st:
        for seq in range(4):                             # every slot comes round again
            got = st.next()
            torch.cuda.synchronize()
            want = _want(seq, weight=False, label_offset=-1, threshold=30.0)
            _same(got, want, "batch %d" % seq)
            assert set(np.unique(want[2])) <= {0.0, 1.0}


def test_skip_resume_continues_bitwise():
    with _stager() as st:
        for seq in range(3):
            st.next()
        after = [st.next() for _ in range(3)]
        torch.cuda.synchronize()
    with _stager() as st:
        st.skip(3)
        resumed = [st.next() for _ in range(3)]
        torch.cuda.synchronize()
    with _stager() as st:                                # skip after the stager has begun: the staged batch is skipped first
        st.next()
        st.skip(2)
        late = st.next()
        torch.cuda.synchronize()
    for i in range(3):
        _same(resumed[i], _want(3 + i), "resumed batch %d" % (3 + i))
        assert all(torch.equal(a, b) for a, b in zip(after[i], resumed[i]))
    _same(late, _want(3), "batch 3 after a late skip")


def test_without_an_augment_the_stager_is_what_it_was():
    with _stager(augment=False) as st:
        assert st.augment is None
        got = st.next()
        torch.cuda.synchronize()
        _same(got, synthetic.make_batch(B, H, W, 1000), "plain batch 0")
        assert got[0].data_ptr() + 4 * 2 * B * H * W == got[2].data_ptr(), "adc and weight are views of the packed copy"


def _model():
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
    return m.cuda()


def test_epoch_train_over_augmented_batches_and_the_fifth_meter():
    steps = 4
    # the plain loop on the reference's batches, stopping the host at every step
    m = _model().train()
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
    crit = PixelWiseNLLLoss()
    losses, accs, fifth = [], [], []
    for seq in range(steps):
        x, lab, wgt = (torch.from_numpy(a).cuda() for a in _want(seq))
        pred = m.forward(x)
        loss = crit.forward(pred, lab, wgt)
        opt.zero_grad()
        loss.backward()
        opt.step()
        cm = metrics.confusion_matrix(pred.detach(), lab).cpu()
        accs.append(metrics.accuracy_from_confusion(cm))
        n12 = int(cm[1].sum() + cm[2].sum())
        fifth.append(100.0 * float(cm[1, 1] + cm[2, 2]) / n12 if n12 else 0.0)               # the host formula
        losses.append(loss.item())
    crit.flush()
    end = {n: p.detach().clone() for n, p in m.named_parameters()}

    m2 = _model()
    opt2 = FlatAdam(m2, lr=1e-3, weight_decay=1e-4)
    lines = []
    with _stager() as st:
        out = epoch.train(st, m2, PixelWiseNLLLoss(), opt2, steps, iiter=1, print_freq=2, log=lines.append, track_shower=True)
    torch.cuda.synchronize()
    assert len(out) == 3
    assert out[0] == sum(losses) / steps and out[1] == sum(a[1] for a in accs) / steps
    assert out[2] == sum(fifth) / steps and any(f > 0.0 for f in fifth)
    assert all(torch.equal(p.detach(), end[n]) for n, p in m2.named_parameters())
    assert all("Acc[trk/shr]" in l for l in lines) and len(lines) == 3

    # the default: return values and log lines as they were
    m3 = _model()
    opt3 = FlatAdam(m3, lr=1e-3, weight_decay=1e-4)
    lines = []
    with _stager() as st:
        out = epoch.train(st, m3, PixelWiseNLLLoss(), opt3, steps, iiter=1, print_freq=2, log=lines.append)
    assert out == (sum(losses) / steps, sum(a[1] for a in accs) / steps) and not any("trk/shr" in l for l in lines)
    with _stager() as st:
        st.skip(steps)
        got = epoch.validate(st, m3, PixelWiseNLLLoss(), 2, print_freq=1, log=lambda s: None, track_shower=True)
    assert isinstance(got, tuple) and len(got) == 2 and 0.0 <= got[1] <= 100.0
