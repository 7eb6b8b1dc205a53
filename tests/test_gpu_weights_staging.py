"""BatchStager(weights=PixelWeights(...)) on the device, at 2 x 1 x 64 x 64 with synthetic loaders: the generated weight image
is exactly the numpy reference of tests/weights_ref.py applied to the labels the stager returns, with and without an Augment;
`when` decides between wire weights and generated ones; without `weights` the stager is what it was; and a train step on
generated weights has the loss of the same step on the reference's weights uploaded from the host."""
import numpy as np
import pytest
import torch

import augment_ref as AR
import oracle.uresnet_oracle as O
import weights_ref as R
from ubresnet_amd import synthetic
from ubresnet_amd.augment import Augment
from ubresnet_amd.pixel_weights import PixelWeights

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.staging import BatchStager
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss

B, H, W = 2, 64, 64
AUG = dict(pad=4, seed=11)
PW = dict(num_classes=3, radius=1, gain=2.0)


class _NoWeight(object):
    """a loader whose wire carries no weight_<tag> entry"""

    def __init__(self, inner):
        self.inner = inner

    def __getitem__(self, idx):
        return {k: v for k, v in self.inner[idx].items() if not k.startswith("weight_")}


def _stager(drop=True, **kw):
    ld = synthetic.SyntheticLArCVDataset(height=H, width=W, tag="train", nentries=64)
    ld.start(B)
    return BatchStager(_NoWeight(ld) if drop else ld, B, H, W, tag="train", timeout=20.0, **kw)


def _two(**kw):
    with _stager(**kw) as st:
        out = []
        for _ in range(2):
            got = st.next()
            torch.cuda.synchronize()
            out.append(tuple(t.cpu().numpy() for t in got) + (None if st.counts is None else st.counts.cpu().numpy(),))
    return out


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _ref(label):
    return R.reference(label, PW["num_classes"], radius=PW["radius"], gain=PW["gain"], lo=1)


def test_generated_weights_are_the_reference_on_the_returned_labels():
    plain = _two()
    made = _two(weights=PixelWeights(**PW))
    for seq, (p, m) in enumerate(zip(plain, made)):
        x, lab, _ = synthetic.make_batch(B, H, W, 1000 + B * seq)
        assert np.array_equal(_bits(m[0]), _bits(p[0])) and np.array_equal(_bits(m[0]), _bits(x)), "adc of batch %d" % seq
        assert np.array_equal(m[1], p[1]) and np.array_equal(m[1], lab), "label of batch %d" % seq
        want, counts = _ref(m[1])
        assert np.array_equal(_bits(m[2]), _bits(want)), "weight of batch %d" % seq
        assert np.array_equal(m[3], counts) and p[3] is None
        assert (p[2] == 1.0).all(), "without weights a wire without the key still gives all ones"
        assert (want != 1.0).any() and (want > R.reference(m[1], 3)[0]).any(), "no interface pixel in the synthetic batch"


def test_generated_weights_follow_the_augmented_labels():
    a = Augment(**AUG)
    made = _two(weights=PixelWeights(**PW), augment=Augment(**AUG))
    for seq, m in enumerate(made):
        x, lab, _ = synthetic.make_batch(B, H, W, 1000 + B * seq)
        adc, label, _ = AR.reference(x, lab.astype(np.float32), None, a.params(seq, B), a.pad, pad_label=a.pad_label,
                                     pad_weight=a.pad_weight)
        assert np.array_equal(_bits(m[0]), _bits(adc)) and np.array_equal(m[1], label), "batch %d" % seq
        want, counts = _ref(label)
        assert np.array_equal(_bits(m[2]), _bits(want)) and np.array_equal(m[3], counts), "weight of batch %d" % seq


def test_when_decides_between_wire_and_generated_weights():
    wire = _two(drop=False, weights=PixelWeights(when="missing", **PW))
    always = _two(drop=False, weights=PixelWeights(when="always", **PW))
    for seq, (w, a) in enumerate(zip(wire, always)):
        x, lab, wgt = synthetic.make_batch(B, H, W, 1000 + B * seq)
        assert np.array_equal(_bits(w[2]), _bits(wgt)) and w[3] is None, "batch %d: the wire weights" % seq
        want, counts = _ref(lab)
        assert np.array_equal(_bits(a[2]), _bits(want)) and np.array_equal(a[3], counts), "batch %d: generated" % seq
        assert not np.array_equal(want, wgt)
        for got in (w, a):
            assert np.array_equal(_bits(got[0]), _bits(x)) and np.array_equal(got[1], lab)


def test_pixel_weights_call_and_counts():
    _, lab, _ = synthetic.make_batch(B, H, W, 1000)
    pw = PixelWeights(**PW)
    label = torch.from_numpy(lab).cuda()
    got = pw(label)
    out = torch.full((B, H, W), -1.0, device="cuda")
    assert pw(label, out=out) is out
    torch.cuda.synchronize()
    want, counts = _ref(lab)
    assert got.dtype == torch.float32 and got.shape == label.shape and tuple(pw.counts.shape) == (B, 16)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    assert np.array_equal(pw.counts.cpu().numpy(), counts)
    with pytest.raises(ValueError):
        pw(label.int())


def _model():
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
    return m.cuda().train()


def _step(m, x, lab, wgt):
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
    crit = PixelWiseNLLLoss()
    loss = crit.forward(m.forward(x), lab, wgt)
    opt.zero_grad()
    loss.backward()
    opt.step()
    crit.flush()
    torch.cuda.synchronize()
    return loss.detach().cpu().numpy()


def test_a_train_step_on_generated_weights_is_the_step_on_the_reference_weights():
    with _stager(weights=PixelWeights(**PW)) as st:
        x, lab, wgt = st.next()
        m1 = _model()
        loss1 = _step(m1, x, lab, wgt)
    xs, labs, _ = synthetic.make_batch(B, H, W, 1000)
    want, _ = _ref(labs)
    m2 = _model()
    loss2 = _step(m2, torch.from_numpy(xs).cuda(), torch.from_numpy(labs).cuda(), torch.from_numpy(want).cuda())
    assert loss1.view(np.int32) == loss2.view(np.int32) and np.isfinite(loss1)
    assert all(torch.equal(p, q) for p, q in zip(m1.parameters(), m2.parameters()))
    ones = _step(_model(), torch.from_numpy(xs).cuda(), torch.from_numpy(labs).cuda(), torch.ones((B, H, W), device="cuda"))
    assert ones.view(np.int32) != loss1.view(np.int32), "the generated weights did not reach the loss"
