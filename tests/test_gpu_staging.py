"""ubresnet_amd.staging.BatchStager on the device: the same tensors as synthetic.DeviceStager, bit for bit; all-ones weights
when the wire has none; tensors that stay the caller's; a training run that cannot tell the stager from resident batches; and
bad labels that surface through PixelWiseNLLLoss as they do today.  The host half is tests/test_cpu_staging.py."""
import numpy as np
import pytest
import torch

import oracle.uresnet_oracle as O
from ubresnet_amd import synthetic

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ubresnet_amd.models.ub_uresnet import UResNet
    from ubresnet_amd.optim import FlatAdam
    from ubresnet_amd.staging import BatchStager
    from ubresnet_amd.training.pixelwise_nllloss import PixelWiseNLLLoss


def _loader(b, p, h, w, nentries=16, **kw):
    ld = synthetic.SyntheticLArCVDataset(height=h, width=w, tag="train", nentries=nentries, planes=p, **kw)
    ld.start(b)
    return ld


@pytest.mark.parametrize("threads", [1, 2])
@pytest.mark.parametrize("shape", [(2, 1, 64, 64), (2, 3, 64, 96), (3, 1, 5, 7)], ids=["2x1x64x64", "2x3x64x96", "3x1x5x7"])
def test_same_tensors_as_device_stager(shape, threads):
    b, p, h, w = shape
    old = synthetic.DeviceStager(_loader(b, p, h, w), b, h, w, planes=p, tag="train")
    with BatchStager(_loader(b, p, h, w), b, h, w, planes=p, tag="train", threads=threads, timeout=20.0) as new:
        for i in range(5):
            want, got = old.next(), new.next()
            torch.cuda.synchronize()
            for name, t, u in zip(("adc", "label", "weight"), want, got):
                assert u.is_cuda and u.dtype == t.dtype and u.shape == t.shape and u.is_contiguous(), (name, i)
                assert torch.equal(t, u), "batch %d: %s differs" % (i, name)
            assert got[1].dtype == torch.int64 and tuple(got[0].shape) == shape and int(got[1].max()) == 2


class _NoWeight(object):
    def __init__(self, inner):
        self.inner = inner

    def __getitem__(self, idx):
        d = self.inner[idx]
        d["weight_train"][:] = 7.0                     # must not show up anywhere
        return {k: v for k, v in d.items() if not k.startswith("weight_")}


def test_missing_weight_gives_ones():
    b, p, h, w = 3, 1, 5, 7
    with BatchStager(_NoWeight(_loader(b, p, h, w)), b, h, w, timeout=20.0) as st:
        for i in range(4):                             # every slot comes round again
            adc, lab, wgt = st.next()
            want = synthetic.make_batch(b, h, w, 1000 + b * i)
            assert torch.equal(wgt.cpu(), torch.ones(b, h, w)) and torch.equal(lab.cpu(), torch.from_numpy(want[1]))
            assert torch.equal(adc.cpu(), torch.from_numpy(want[0]))


def test_label_offset_and_threshold_reach_the_kernel():
    b, p, h, w = 2, 1, 64, 64
    with BatchStager(_loader(b, p, h, w), b, h, w, label_offset=-1, adc_threshold=30.0, timeout=20.0) as st:
        adc, lab, wgt = st.next()
        x, l, _ = synthetic.make_batch(b, h, w, 1000)
        dark = x[:, 0] < 30.0
        assert torch.equal(adc.cpu(), torch.from_numpy(np.where(x < 30.0, np.float32(0.0), x)))
        assert torch.equal(lab.cpu(), torch.from_numpy(np.where(dark, 0, l - 1)))
        assert dark.any() and (~dark).any()


def test_held_batches_keep_their_values():
    b, p, h, w = 2, 1, 64, 64
    held = []
    with BatchStager(_loader(b, p, h, w, nentries=64), b, h, w, threads=2, timeout=20.0) as st:
        for i in range(9):
            held.append(st.next())
        torch.cuda.synchronize()
    for i in range(3):                                 # each was held across six or more later next() calls
        x, lab, wgt = synthetic.make_batch(b, h, w, 1000 + b * i)
        a, l, g = held[i]
        assert torch.equal(a.cpu(), torch.from_numpy(x)) and torch.equal(l.cpu(), torch.from_numpy(lab))
        assert torch.equal(g.cpu(), torch.from_numpy(wgt))
    ptrs = [t.data_ptr() for bt in held for t in bt]
    assert len(set(ptrs)) == len(ptrs), "device memory was handed out twice while the caller held it"


def _model():
    m = UResNet(num_classes=3, input_channels=1, inplanes=16)
    m.load_state_dict(O.seeded_state_dict(O.uresnet_schema(3, 1, 16, 16), 42))
    return m.cuda().train()


def _state(m):
    out = {"param:" + n: p.detach().clone() for n, p in m.named_parameters()}
    out.update({"grad:" + n: p.grad.detach().clone() for n, p in m.named_parameters()})
    out.update({"buffer:" + n: v.detach().clone() for n, v in m.named_buffers()})
    return out


def test_training_cannot_tell_the_stager_from_resident_batches():
    b, h, w, steps = 2, 64, 64, 4
    crit = PixelWiseNLLLoss()
    ends = []
    for fed in ("stager", "resident"):
        m = _model()
        opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
        st = BatchStager(_loader(b, 1, h, w), b, h, w, timeout=20.0) if fed == "stager" else None
        for i in range(steps):
            if st is not None:
                x, lab, wgt = st.next()
            else:
                x, lab, wgt = (torch.from_numpy(a).cuda() for a in synthetic.make_batch(b, h, w, 1000 + b * i))
            loss = crit.forward(m.forward(x), lab, wgt)
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        crit.flush()
        if st is not None:
            st.close()
        ends.append(_state(m))
    assert ends[0].keys() == ends[1].keys() and any(k.startswith("buffer:") for k in ends[0])
    diff = [k for k in ends[0] if not torch.equal(ends[0][k], ends[1][k])]
    assert not diff, "%d of %d tensors differ: %s" % (len(diff), len(ends[0]), diff[:6])


class _BadLabel(object):
    def __init__(self, inner, value):
        self.inner, self.value = inner, value

    def __getitem__(self, idx):
        d = self.inner[idx]
        d["label_train"][11] = self.value
        return d


@pytest.mark.parametrize("value", [7.0, float("nan")], ids=["label-7", "label-nan"])
def test_a_bad_wire_label_surfaces_through_the_loss(value):
    b, h, w = 2, 64, 64
    crit = PixelWiseNLLLoss()
    crit.flush()
    m = _model()
    with BatchStager(_BadLabel(_loader(b, 1, h, w), value), b, h, w, timeout=20.0) as st:
        x, lab, wgt = st.next()
        assert int(lab.reshape(-1)[11]) == (7 if value == 7.0 else -2 ** 63)
        loss = crit.forward(m.forward(x), lab, wgt)
        loss.backward()
        with pytest.raises(RuntimeError, match=r"1 target label\(s\) outside \[0, 3\)"):
            crit.flush()
