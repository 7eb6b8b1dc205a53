"""The host half of ubresnet_amd.staging.BatchStager without a GPU (device=None, pin=False): producer threads, slots, batch
order, errors and shutdown.  The device half is tests/test_gpu_staging.py."""
import threading
import time

import numpy as np
import pytest

from ubresnet_amd.staging import BatchStager

SHAPES = [(3, 1, 5, 7), (2, 3, 8, 16)]          # (B, P, H, W); in the first, the packed sections are only 4-byte aligned


class StampLoader(object):
    """larcvdataset surface; every array of call k (0-based) is stamped with k.  Not thread-safe on purpose: it checks that no
    two calls overlap."""

    def __init__(self, shape, tag="train", sleep_ms=0.0, weight=True, fail_at=None, gate=None, seed=0):
        self.b, self.p, self.h, self.w = shape
        self.tag, self.sleep_ms, self.weight, self.fail_at, self.gate = tag, sleep_ms, weight, fail_at, gate
        self.calls = 0
        self.inside = 0
        self.overlap = False
        self.rs = np.random.RandomState(seed)

    @staticmethod
    def content(k, shape):
        b, p, h, w = shape
        n = b * h * w
        src = (np.arange(p * n, dtype=np.float32) % 997) + np.float32(1000 * k)
        return src, np.full(n, k % 3, np.float32), np.full(n, k + 0.5, np.float32)

    def __getitem__(self, idx):
        self.inside += 1
        self.overlap |= self.inside > 1
        try:
            k = self.calls
            self.calls += 1
            if self.fail_at is not None and k + 1 == self.fail_at:
                raise KeyError("the loader broke at call %d" % self.fail_at)
            if self.gate is not None:
                self.gate.wait(10.0)
            if self.sleep_ms:
                time.sleep(self.rs.uniform(0.0, self.sleep_ms) * 1e-3)
            src, lab, wgt = self.content(k, (self.b, self.p, self.h, self.w))
            d = {"source_%s" % self.tag: src, "label_%s" % self.tag: lab}
            if self.weight:
                d["weight_%s" % self.tag] = wgt
            return d
        finally:
            self.inside -= 1


def _stager(loader, shape, **kw):
    b, p, h, w = shape
    kw.setdefault("timeout", 5.0)
    return BatchStager(loader, b, h, w, planes=p, device=None, pin=False, **kw)


def _check(batch, k, shape):
    b, p, h, w = shape
    src, lab, wgt = StampLoader.content(k, shape)
    assert batch.seq == k
    assert batch.image.shape == (b, p, h, w) and batch.label_wire.shape == (b, h, w) and batch.weight.shape == (b, h, w)
    assert batch.image.dtype == batch.label_wire.dtype == batch.weight.dtype == np.float32
    assert np.array_equal(batch.image.reshape(-1), src) and np.array_equal(batch.label_wire.reshape(-1), lab)
    assert np.array_equal(batch.weight.reshape(-1), wgt)


def _no_live_thread(st):
    return not any(t.is_alive() for t in st._threads)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("threads", [1, 2, 4])
def test_forty_batches_arrive_in_sequence_order(threads, shape):
    loader = StampLoader(shape, sleep_ms=5.0, seed=threads)
    with _stager(loader, shape, threads=threads) as st:
        assert len(st._slots) == threads + 1
        for k in range(40):
            _check(st.next(), k, shape)
        times = st.stage_times()
    assert not loader.overlap, "two producers were inside the loader at once"
    assert _no_live_thread(st)
    assert times["loader"][1] >= 40 and times["fill"][1] >= 40 and times["wait_slot"][1] >= 40


@pytest.mark.parametrize("shape", SHAPES)
def test_a_slot_is_not_refilled_before_it_is_released(shape):
    loader = StampLoader(shape)
    with _stager(loader, shape, threads=2, slots=2) as st:
        for k in range(12):
            batch = st.next()
            time.sleep(0.02)                       # the producers have nothing to wait for but this slot
            _check(batch, k, shape)                # still this batch's content
            assert loader.calls <= k + 2, "the loader ran ahead of the free slots"


def test_missing_weight_entry_is_reported_not_invented():
    shape = SHAPES[0]
    with _stager(StampLoader(shape, weight=False), shape) as st:
        batch = st.next()
        assert batch.weight is None and batch.seq == 0


def test_a_loader_error_reaches_the_next_of_its_batch():
    shape = SHAPES[1]
    loader = StampLoader(shape, fail_at=5)
    st = _stager(loader, shape, threads=2)
    for k in range(4):
        _check(st.next(), k, shape)
    with pytest.raises(KeyError, match="broke at call 5"):
        st.next()
    assert _no_live_thread(st) and loader.calls == 5
    with pytest.raises(RuntimeError, match="closed"):
        st.next()


def test_a_wrong_array_is_an_error_not_a_conversion():
    shape = SHAPES[0]

    class Doubles(StampLoader):
        def __getitem__(self, idx):
            d = StampLoader.__getitem__(self, idx)
            d["label_train"] = d["label_train"].astype(np.float64)
            return d
    st = _stager(Doubles(shape), shape)
    with pytest.raises(ValueError, match="label_train"):
        st.next()
    assert _no_live_thread(st)


def test_a_blocked_loader_times_out():
    shape = SHAPES[0]
    gate = threading.Event()
    st = _stager(StampLoader(shape, gate=gate), shape, threads=2, timeout=0.5)
    t0 = time.monotonic()
    with pytest.raises(RuntimeError, match="^Batch Loader timed out$"):
        st.next()
    assert 0.4 < time.monotonic() - t0 < 1.9
    gate.set()                                     # let the stuck producer go
    st.close()
    assert _no_live_thread(st)


def test_close_joins_quickly_and_twice():
    shape = SHAPES[1]
    st = _stager(StampLoader(shape), shape, threads=4)
    _check(st.next(), 0, shape)
    t0 = time.monotonic()
    st.close()
    assert time.monotonic() - t0 < 1.0 and _no_live_thread(st)
    st.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.next()
    with pytest.raises(RuntimeError, match="closed"):
        st.skip(1)


@pytest.mark.parametrize("started", [False, True])
def test_skip_three_then_next_gives_batch_three(started):
    shape = SHAPES[0]
    loader = StampLoader(shape)
    with _stager(loader, shape, threads=2) as st:
        first = 0
        if started:                                # producers already run ahead: the skipped batches are taken and dropped
            _check(st.next(), 0, shape)
            first = 1
        st.skip(3)
        batch = st.next()
        assert batch.seq == first + 3
        _check(batch, first + 3, shape)
