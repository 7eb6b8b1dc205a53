"""The numpy reference of libubresnet_match.so (include/ubresnet_match.h): the candidates by a plain filter of the cluster table,
the profile and the pixel counts by np.add.at, the candidate rows and the pair table by whole-array minimum and sums in int64.
Everything is integer: the GPU tests compare whole buffers bit for bit.  The weight of a pixel is tests/moment_ref.weight."""
import numpy as np

import cluster_ref as CR
import moment_ref as MR

TILE = 64
CHUNK_BINS = 64
CAND_COLUMNS = 6
PAIR_COLUMNS = 4
CLUSTER_FIXED = 8
MIN_SLOTS, MAX_SLOTS = 64, 4096
MAX_TIME_BIN = 64
MAX_SHIFT = 4096
MAX_WEIGHT = MR.MAX_WEIGHT
CAND_NAMES = ("cluster", "plane", "Q", "bins", "t_min", "t_max")
PAIR_NAMES = ("both", "I", "Qi_in", "Qj_in")
SENTINEL = -0x0123456789ABCDEF


def time_bins(rows, time_bin):
    return -(-rows // time_bin)


def match(ids, table, count, capacity, view, adc_scale, min_pixels, time_bin, row_shift, slots, sentinel=SENTINEL):
    """what ubu_match stores, for buffers prefilled with `sentinel` where the library leaves them alone:
    dict(profile uint32 [S, T], occ int64 [S, T], candidates int64 [S, 6], pairs int64 [S, S, 4], ncand, status [2] (the two
    amounts ADDED), n = min(ncand, S))"""
    P, rows, cols = ids.shape
    assert time_bin in (1, 2, 4, 8, 16, 32, 64) and slots % TILE == 0 and MIN_SLOTS <= slots <= MAX_SLOTS and len(row_shift) == P
    S, T, log2 = slots, time_bins(rows, time_bin), time_bin.bit_length() - 1
    nrows = min(int(count), int(capacity), ids.size)
    k_all = np.flatnonzero(table[:nrows, 1] >= min_pixels)
    ncand, n = len(k_all), min(len(k_all), S)
    slot_of = np.full(max(nrows, 1), -1, np.int64)
    slot_of[k_all[:n]] = np.arange(n)
    flat = ids.reshape(-1).astype(np.int64)
    q = np.flatnonzero((flat >= 0) & (flat < nrows))
    q = q[slot_of[flat[q]] >= 0]
    slot = slot_of[flat[q]]
    shifted = q % (rows * cols) // cols + np.asarray(row_shift, np.int64)[q // (rows * cols)]
    inside = (shifted >= 0) & (shifted < rows)
    dropped = int((~inside).sum())
    q, slot, t = q[inside], slot[inside], shifted[inside] >> log2
    w, _, _ = MR.weight(view.reshape(-1)[q], adc_scale)
    profile, occ = np.zeros((S, T), np.int64), np.zeros((S, T), np.int64)
    np.add.at(profile, (slot, t), w)
    np.add.at(occ, (slot, t), 1)
    assert profile.max(initial=0) < 2 ** 32
    cand = np.zeros((S, CAND_COLUMNS), np.int64)
    held = occ[:n] > 0
    cand[:n, 0] = k_all[:n]
    cand[:n, 1] = table[k_all[:n], 0] // (rows * cols)
    cand[:n, 2] = profile[:n].sum(1)
    cand[:n, 3] = held.sum(1)
    cand[:n, 4] = np.where(held.any(1), held.argmax(1), T)
    cand[:n, 5] = np.where(held.any(1), T - 1 - held[:, ::-1].argmax(1), -1)
    pairs = np.full((S, S, PAIR_COLUMNS), sentinel, np.int64)
    for i in range(n):
        j = np.arange(i + 1, n)
        if not len(j):
            continue
        both = held[i][None] & held[j]
        rows_ = np.stack([both.sum(1), np.minimum(profile[i][None], profile[j]).sum(1), (profile[i][None] * both).sum(1),
                          (profile[j] * both).sum(1)], 1)
        rows_[cand[j, 1] == cand[i, 1]] = 0
        pairs[i, j] = rows_
    return dict(profile=profile.astype(np.uint32), occ=occ, candidates=cand, pairs=pairs, ncand=ncand, status=[max(ncand - S, 0), dropped],
                n=n)


SEGMENT_PITCH = 8


def segments(shape, counts, seed=0, row_ranges=None, lengths=(3, 6)):
    """a uint8 label map (CR.FILL where dark) with exactly counts[p] clusters in plane p: horizontal segments of lengths[0]..
    lengths[1] pixels on every second row of row_ranges[p] (the whole plane if None) and every SEGMENT_PITCH-th column, so that no
    two touch; which places of that grid are taken, the lengths and the classes are drawn from `seed`"""
    P, rows, cols = shape
    assert len(counts) == P and lengths[1] <= SEGMENT_PITCH - 2 and cols >= lengths[1]
    rng = np.random.default_rng(seed)
    label = np.full(shape, CR.FILL, np.uint8)
    for p in range(P):
        r0, r1 = (0, rows) if row_ranges is None else row_ranges[p]
        places = [(r, c) for r in range(r0, r1, 2) for c in range(0, cols - lengths[1] + 1, SEGMENT_PITCH)]
        assert counts[p] <= len(places), "plane %d has %d places for %d segments" % (p, len(places), counts[p])
        for at in rng.permutation(len(places))[:counts[p]]:
            r, c = places[at]
            label[p, r, c:c + rng.integers(lengths[0], lengths[1] + 1)] = rng.integers(0, CR.C4)
    return label


def clustered(label, seed=7):
    """the ids, table and count a clusterer (8-connected, not by class) gives for a uint8 label map with CR.FILL where dark"""
    ref = CR.reference(label, CR.confidence_bits(label.shape, seed), CR.C4, CR.FILL, 8, False)
    return ref["ids"], ref["table"], ref["count"]


def label_of(image, label, threshold=0.0):
    """the uint8 class map of a synthetic event as the clusterer takes it: CR.FILL where the image is dark"""
    return np.where(image > threshold, label, CR.FILL).astype(np.uint8)


def truth_pairs(ids, table, instance, min_pixels):
    """{(ka, kb)}: the pairs of candidate clusters from different planes that hold the same instance, for an event whose clusters
    are its objects -- every cluster of at least min_pixels pixels is mapped to the instance most of its pixels carry"""
    P = ids.shape[0]
    of = {}
    for k in np.flatnonzero(table[:, 1] >= min_pixels):
        inst = instance[ids == k]
        of[int(k)] = int(np.bincount(inst[inst >= 0]).argmax())
    plane = {k: int(table[k, 0]) // (ids.shape[1] * ids.shape[2]) for k in of}
    ks = sorted(of)
    return {(a, b) for a in ks for b in ks if a < b and plane[a] != plane[b] and of[a] == of[b]}, of
