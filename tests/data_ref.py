"""Reference of ubd_prep_batch (include/ubresnet_data.h) in numpy, written from the header's rules, the inputs its tests share,
and the table of cases that tests/test_gpu_data_exact.py runs -- one entry per kernel compiled into libubresnet_data.so, which
tests/test_cpu_data.py holds against the library's symbol table.  No GPU and no torch here.

Acceptance: every output is equal to the reference bit for bit; there is no tolerance anywhere."""
import numpy as np

INT64_MIN = -2 ** 63

# launch geometry, as include/ubresnet_data.h states it (tests/test_cpu_data.py holds these against the header)
LANE_PIXELS, BLOCK, MAX_GRID = 4, 256, 2048
WAVE_SPAN = 64 * LANE_PIXELS
BLOCK_SPAN = BLOCK * LANE_PIXELS

# kernel (normal form of tools/kernel_symbols.py) -> ids of the cases in test_gpu_data_exact.py that launch it: the threshold
# switch of ubd_prep_batch picks the instantiation
KERNEL_CASES = {
    "prep_batch_kernel<false>": ["counts-aligned", "counts-offset", "grid-stride", "edge-labels", "untouched"],
    "prep_batch_kernel<true>": ["thr10-p1", "thr10-p3", "thr0-p3", "thr10-p3-offset", "thr-grid-stride", "one-of-three"],
}

# pixel counts around every span of the launch geometry: 1; a lane's vector; a wave; a workgroup; a last workgroup with a
# partial trip (three full workgroups, then two full waves and a part of the third)
COUNTS = ([1] + [s + d for s in (LANE_PIXELS, WAVE_SPAN, BLOCK_SPAN) for d in (-1, 0, 1)]
          + [3 * BLOCK_SPAN + 2 * WAVE_SPAN + 37])
# the grid is capped at MAX_GRID workgroups and strides: two full trips of the whole grid, then a part of a third
STRIDE_COUNT = 2 * MAX_GRID * BLOCK_SPAN + 5 * BLOCK_SPAN + WAVE_SPAN + 3

_F = np.float32
# (wire value, label at offset 0 or None for INT64_MIN)
EDGE_LABELS = [
    (_F(-0.0), 0),
    (_F(0.99999994), 0),
    (_F(-0.5), 0),
    (_F(2.5), 2),
    (_F(-2.5), -2),
    (_F(2147483520.0), 2147483520),                 # the largest float below 2^31
    (_F(-2147483520.0), -2147483520),
    (_F(2147483648.0), None),                       # 2^31
    (_F(-2147483648.0), None),                      # -2^31: |v| < 2^31 fails
    (_F(3e38), None),
    (_F(1e-40), 0),                                 # a subnormal
    (_F(-1e-40), 0),
    (_F(np.nan), None),
    (_F(np.inf), None),
    (_F(-np.inf), None),
]


def reference(label_wire, label_offset, image=None, planes=1, hw=1, threshold=None, weight=None, fill_weight=False):
    """ubd_prep_batch on the host.  label_wire [n] f32; image [B*planes*hw] f32 and weight [n] f32 are the buffers' contents
    BEFORE the call (or None).  -> (label int64 [n], image after, weight after)"""
    v = np.asarray(label_wire, np.float32).reshape(-1)
    n = v.size
    wide = v.astype(np.float64)                       # exact
    with np.errstate(invalid="ignore"):
        ok = np.abs(wide) < 2.0 ** 31                 # False for NaN
    label = np.full(n, INT64_MIN, np.int64)
    label[ok] = np.trunc(wide[ok]).astype(np.int64) + int(label_offset)
    if threshold is not None:
        img = np.array(image, np.float32).reshape(n // hw, planes, hw)
        with np.errstate(invalid="ignore"):
            below = img < np.float32(threshold)       # strict; False for NaN; decided on the original values
        img[below] = np.float32(0.0)
        label[below.all(axis=1).reshape(-1)] = 0
        image = img.reshape(-1)
    elif image is not None:
        image = np.array(image, np.float32).reshape(-1)
    if weight is not None:
        weight = np.ones(n, np.float32) if fill_weight else np.array(weight, np.float32).reshape(-1)
    return label, image, weight


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def wire_labels(rs, n):
    """class ids 0..2 as floats, with fractional and negative values and every edge value sprinkled in (all of them once n allows)"""
    v = rs.randint(0, 3, n).astype(np.float32)
    frac = rs.rand(n) < 0.1
    v[frac] = (rs.uniform(-4.0, 4.0, n).astype(np.float32))[frac]
    edges = np.array([e for e, _ in EDGE_LABELS], np.float32)
    k = min(n, 3 * len(edges))
    v[rs.choice(n, k, replace=False)] = np.resize(edges, k)
    return v


def adc_image(rs, nb, planes, hw, thr):
    """[nb*planes*hw] f32: about half below `thr`; values just below, at and just above it, -0.0 and NaN sprinkled in; and a
    quarter of the pixels lit in exactly one plane (the others below)"""
    t = np.float32(thr)
    a = rs.uniform(-5.0, 5.0, (nb, planes, hw)).astype(np.float32) + t + np.where(rs.rand(nb, planes, hw) < 0.5, _F(-6.0), _F(6.0))
    one = rs.rand(nb, hw) < 0.25
    which = rs.randint(0, planes, (nb, hw))
    for p in range(planes):
        lit = one & (which == p)
        a[:, p, :][one & ~lit] = t - _F(3.0)
        a[:, p, :][lit] = t + _F(3.0)
    flat = a.reshape(-1)
    special = np.array([np.nextafter(t, _F(-np.inf)), t, np.nextafter(t, _F(np.inf)), _F(-0.0), _F(0.0), _F(np.nan)], np.float32)
    k = min(flat.size, 4 * len(special))
    flat[rs.choice(flat.size, k, replace=False)] = np.resize(special, k)
    return flat
