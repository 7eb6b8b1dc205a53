"""The numpy reference of libubresnet_moment.so (include/ubresnet_moment.h): the weight of a pixel in np.float32 with np.rint, the
table by np.add.at in int64, and the derived quantities -- centroid, covariance, extent, axis, linearity -- from central moments
formed exactly in Python integers.  Everything up to the table is integer: the GPU tests compare bit for bit."""
import math

import numpy as np

TABLE_FIXED = 9
MAX_WEIGHT = 65535
MAX_ROWS = MAX_COLS = 4096
MAX_PLANE_PIXELS = 1 << 22
MAX_SCALE = 256
TRIP_PIXELS = 2048
SLOTS = 64
MAX_GRID = 1024
COLUMNS = ("weighted", "clipped", "odd", "Q", "Qr", "Qc", "Qrr", "Qrc", "Qcc")

# the values the ADC maker sprinkles: zeros of both signs, subnormals of both signs, the ties at scale 16 (0.5 -> 0, 1.5 -> 2,
# 2.5 -> 2), the largest unclipped value and the smallest clipped one at scale 16, huge, infinite, negative and NaN
EDGE_ADC = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 0.03125, 0.09375, 0.15625, 0.031249998, 4095.9375, 4096.0, 4095.96875, 1e30,
                     np.inf, -1.0, -np.inf, np.nan, -1e-30, 65535.0, 65536.0, 255.99805, 1.0, 100.0], np.float32)


def weight(view, adc_scale):
    """(w int64, clipped bool, odd bool) of float32 ADC values"""
    assert adc_scale in (1, 2, 4, 8, 16, 32, 64, 128, 256)
    v = np.asarray(view, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = v * np.float32(adc_scale)
        assert t.dtype == np.float32
        odd = np.isnan(t) | (t < 0)
        clipped = ~odd & (t > np.float32(MAX_WEIGHT))
        r = np.rint(np.where(odd | clipped, np.float32(0), t))
    w = np.where(clipped, MAX_WEIGHT, r.astype(np.int64))
    return w, clipped, odd


def table(ids, label, view, C, adc_scale, capacity, count):
    """int64 [min(count, capacity), 9 + C]: the rows ubm_moments stores"""
    P, rows, cols = ids.shape
    n = min(int(count), int(capacity))
    flat = ids.reshape(-1).astype(np.int64)
    q = np.flatnonzero((flat >= 0) & (flat < n))
    k = flat[q]
    lab = label.reshape(-1)[q].astype(np.int64)
    w, clipped, odd = weight(view.reshape(-1)[q], adc_scale)
    foreign = lab >= C                                            # no class of the table: odd, and nothing else
    w, clipped, odd = np.where(foreign, 0, w), clipped & ~foreign, odd | foreign
    r, c = q % (rows * cols) // cols, q % cols
    out = np.zeros((n, TABLE_FIXED + C), np.int64)
    for col, v in enumerate(((w > 0).astype(np.int64), clipped.astype(np.int64), odd.astype(np.int64), w, w * r, w * c, w * r * r, w * r * c,
                             w * c * c)):
        np.add.at(out[:, col], k, v)
    np.add.at(out, (k[~foreign], TABLE_FIXED + lab[~foreign]), w[~foreign])
    return out


def adc(shape, seed=5, lit=None):
    """a seeded field of ADC values in 0..300 with the edge values sprinkled over an eighth of it; where `lit` is given, every edge
    value is placed on a lit pixel at least once if there are enough of them"""
    rng = np.random.default_rng(seed + int(np.prod(shape)))
    v = (rng.random(shape) * 300).astype(np.float32)
    v[rng.random(shape) < 0.3] = np.float32(12.03125)             # a tie at scale 16 on many pixels
    pick = rng.random(shape) < 0.125
    v[pick] = EDGE_ADC[rng.integers(0, len(EDGE_ADC), int(pick.sum()))]
    if lit is not None:
        q = np.flatnonzero(lit.reshape(-1))
        if len(q) >= len(EDGE_ADC):
            v.reshape(-1)[rng.permutation(q)[:len(EDGE_ADC)]] = EDGE_ADC
    return v


WALK_PIXELS = 2 * TRIP_PIXELS * 2 + 5     # several trips, an odd count, a ragged last load whose last lane holds one real pixel


def walk_case():
    """(ids int32 [n], label uint8 [n], view float32 [n], n_ids) for n = WALK_PIXELS flat pixels: one case that crosses every branch
    of the pixel walk the moment and overlap libraries share (csrc/ubr_walk.h).  A wave holds 64 lanes of four consecutive pixels,
    256 pixels; the waves cycle through four id patterns, each with ids of its own:
      0  all 64 lanes share one id (one group of 64, one combined round)
      1  64 distinct ids, one per lane (every lane solo)
      2  two ids interleaved lane by lane (two groups of 32)
      3  lanes 0..15 one id; lane 16 two ids, two pixels each (the "mixed" round: four per-pixel rounds for the wave); lanes 17..31
         no pixel that takes part; lanes 32..47 an id each (solo); lanes 48..63 two ids interleaved, the pixels 1 and 2 of each
         lane dark (a group whose lanes hold fewer than four pixels)
    The last load is ragged: lane 0 holds four pixels and lane 1 one, of the same id.  The ADC values cycle through EDGE_ADC (23
    values, coprime with the 4 pixels of a lane and the 256 of a wave); the labels cycle through 0..3 with a foreign 4 every 11th."""
    n = WALK_PIXELS
    lane, wave = (np.arange(n) // 4) % 64, np.arange(n) // 256
    slot = np.arange(n) % 4
    base = wave * 100                                             # the ids of a wave are its own: < 100 per wave
    ids = np.full(n, -1, np.int64)
    for kind in range(4):
        w = wave % 4 == kind
        if kind == 0:
            ids[w] = base[w]
        elif kind == 1:
            ids[w] = base[w] + lane[w]
        elif kind == 2:
            ids[w] = base[w] + lane[w] % 2
        else:
            ids[w & (lane < 16)] = base[w & (lane < 16)]
            mixed = w & (lane == 16)
            ids[mixed] = base[mixed] + 1 + slot[mixed] // 2
            solo = w & (lane >= 32) & (lane < 48)
            ids[solo] = base[solo] + lane[solo]
            pair = w & (lane >= 48) & ((slot == 0) | (slot == 3))
            ids[pair] = base[pair] + 90 + lane[pair] % 2
    ids[n - 5:] = base[-1] + 99                                   # the ragged tail: lane 0 whole, lane 1 one pixel
    label = (np.arange(n) % 4).astype(np.uint8)
    label[::11] = 4
    view = EDGE_ADC[np.arange(n) % len(EDGE_ADC)]
    assert n % 4 == 1 and n > 4 * TRIP_PIXELS and (wave[-1] % 4, lane[-1], slot[-1]) == (0, 1, 0)
    return ids.astype(np.int32), label, view.astype(np.float32), int(ids.max()) + 1


def central(row):
    """the exact central second moments of a table row as Python-int numerators over Q^2: (Q, Q Qrr - Qr^2, Q Qrc - Qr Qc, Q Qcc - Qc^2)"""
    Q, Qr, Qc, Qrr, Qrc, Qcc = (int(v) for v in row[3:9])
    return Q, Q * Qrr - Qr * Qr, Q * Qrc - Qr * Qc, Q * Qcc - Qc * Qc


def shape_of(row):
    """dict(centroid, covariance, extent, axis, linearity) of one table row, NaN where Q == 0"""
    nan = float("nan")
    Q, nrr, nrc, ncc = central(row)
    if Q == 0:
        return dict(centroid=(nan, nan), covariance=((nan, nan), (nan, nan)), extent=(nan, nan), axis=(nan, nan), linearity=nan)
    srr, src, scc = nrr / (Q * Q), nrc / (Q * Q), ncc / (Q * Q)   # int / int: one rounding
    half, diff = (srr + scc) / 2, (srr - scc) / 2
    root = math.hypot(diff, src)
    major, minor = half + root, max(half - root, 0.0)
    if src == 0 and diff == 0:
        axis = (0.0, 1.0)
    elif src == 0:
        axis = (1.0, 0.0) if srr > scc else (0.0, 1.0)
    else:
        dr, dc = major - scc, src                                 # (S - minor-side) eigenvector of the major eigenvalue
        if abs(major - srr) > abs(major - scc):
            dr, dc = src, major - srr
        n = math.hypot(dr, dc)
        dr, dc = dr / n, dc / n
        if dc < 0 or (dc == 0 and dr < 0):
            dr, dc = -dr, -dc
        axis = (dr, dc)
    return dict(centroid=(int(row[4]) / Q, int(row[5]) / Q), covariance=((srr, src), (src, scc)),
                extent=(math.sqrt(major), math.sqrt(minor)), axis=axis, linearity=(1 - minor / major) if major > 0 else nan)
