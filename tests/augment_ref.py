"""Reference of uba_augment_batch (include/ubresnet_aug.h) in numpy, written from the header's rule, and the table of cases that
tests/test_gpu_augment_exact.py runs -- one entry per kernel compiled into libubresnet_aug.so, which tests/test_cpu_augment.py
holds against the library's symbol table.  T and L, the per-pixel rules, are data_ref.reference (ubd_prep_batch's reference);
the inputs come from data_ref too.  No GPU and no torch here.

Acceptance: every output is equal to the reference bit for bit; there is no tolerance anywhere."""
import numpy as np

import data_ref as D

INT64_MIN = D.INT64_MIN
wire_labels, adc_image, EDGE_LABELS = D.wire_labels, D.adc_image, D.EDGE_LABELS

# launch geometry and limits, as include/ubresnet_aug.h states them (tests/test_cpu_augment.py holds these against the header)
LANE_PIXELS, BLOCK, MAX_GRID, MAX_BATCH, MAX_PAD = 4, 256, 1024, 256, 16383

# kernel (normal form of tools/kernel_symbols.py) -> ids of the cases in test_gpu_augment_exact.py that launch it: the
# threshold switch of uba_augment_batch picks the instantiation
KERNEL_CASES = {
    "augment_batch_kernel<false>": ["sweep", "three-images", "edge-values", "grid-stride", "same-pixel", "identity"],
    "augment_batch_kernel<true>": ["sweep-thr10", "sweep-thr0", "three-images-thr", "edge-values-thr", "identity-thr"],
}


def groups(b, h, w):
    """lane work items of a batch: B * H * ceil(W / LANE_PIXELS)"""
    return b * h * ((w + LANE_PIXELS - 1) // LANE_PIXELS)


def stride_shape():
    """(B, H, W) at which the capped grid takes two full trips and a part of a third (every workgroup two, the first 5/16 of
    them three), on the vector path: a row is exactly one workgroup's trip, and there are 2 * MAX_GRID + MAX_GRID * 5 / 16 rows"""
    w = BLOCK * LANE_PIXELS
    rows = 2 * MAX_GRID + (5 * MAX_GRID) // 16
    b = 4
    assert rows % b == 0
    return b, rows // b, w


def source_index(params, b, h, w, pad):
    """the header's map: -> (sr [B,H], sc [B,W], inside [B,H,W]) for output pixel (b, r, c)"""
    par = np.asarray(params, np.int64).reshape(b, 4)
    r, c = np.arange(h, dtype=np.int64)[None, :], np.arange(w, dtype=np.int64)[None, :]
    pr = r + par[:, 2:3]
    pr = np.where(par[:, 0:1] != 0, (h + 2 * pad - 1) - pr, pr)
    pc = c + par[:, 3:4]
    pc = np.where(par[:, 1:2] != 0, (w + 2 * pad - 1) - pc, pc)
    sr, sc = pr - pad, pc - pad
    inside = ((sr >= 0) & (sr < h))[:, :, None] & ((sc >= 0) & (sc < w))[:, None, :]
    return sr, sc, inside


def reference(image, label_wire, weight, params, pad, label_offset=0, threshold=None, pad_label=0, pad_weight=0.0):
    """uba_augment_batch on the host.  image [B,P,H,W] f32, label_wire [B,H,W] f32, weight [B,H,W] f32 or None, params [B,4].
    -> (image_out [B,P,H,W] f32, label_out [B,H,W] int64, weight_out [B,H,W] f32)"""
    image = np.asarray(image, np.float32)
    b, p, h, w = image.shape
    lab, img, _ = D.reference(np.asarray(label_wire, np.float32).reshape(-1), label_offset, image.reshape(-1), p, h * w, threshold)
    img, lab = img.reshape(b, p, h, w), lab.reshape(b, h, w)
    wgt = np.ones((b, h, w), np.float32) if weight is None else np.asarray(weight, np.float32).reshape(b, h, w)
    sr, sc, inside = source_index(params, b, h, w, pad)
    bi = np.arange(b)[:, None, None]
    ri, ci = np.clip(sr, 0, h - 1)[:, :, None], np.clip(sc, 0, w - 1)[:, None, :]
    image_out = np.where(inside[:, None], img[bi[:, None], np.arange(p)[None, :, None, None], ri[:, None], ci[:, None]], np.float32(0.0))
    label_out = np.where(inside, lab[bi, ri, ci], np.int64(pad_label))
    weight_out = np.where(inside, wgt[bi, ri, ci], np.float32(pad_weight))
    return image_out.astype(np.float32, copy=False), label_out.astype(np.int64, copy=False), weight_out.astype(np.float32, copy=False)
