"""The references of libubresnet_overlap.so (include/ubresnet_overlap.h).

table(): the numpy reference -- the pair keys packed into uint64, np.unique(return_index, return_counts), the weights of
tests/moment_ref.py summed with np.add.at, the rows ordered by `first`.  Everything is integer: the GPU tests compare bit for bit.

occupied() / longest_run(): a pure-Python model of the hash table in scratch, with the hash and the probe limit of
csrc/ubr_overlap_plan.h: the set of slots a key set occupies when inserted in a given order, and the longest cyclic run of occupied
slots.  While that run is below the probe limit, no insertion order can leave a key without a slot: a key probes forward from its
home slot over occupied slots only, and a run shorter than the limit ends in a free slot before the limit does."""
import numpy as np

import moment_ref as MR

COLUMNS = 6
COLUMN_NAMES = ("a", "b", "first", "pixels", "weighted", "Q")
MAX_PROBES = 128
MIN_SLOTS = 64
MAX_WEIGHT = MR.MAX_WEIGHT
TRIP_PIXELS = 2048
LDS_SLOTS = 64
GOLDEN = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1


def keys_of(ids_a, ids_b):
    """uint64 per pixel: (a + 1) << 32 | (b + 1) with every negative id as -1; 0 where the pixel does not take part"""
    a = np.maximum(ids_a.reshape(-1).astype(np.int64), -1) + 1
    b = np.maximum(ids_b.reshape(-1).astype(np.int64), -1) + 1
    return (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)


def table(ids_a, ids_b, view=None, adc_scale=16):
    """int64 [total, 6], every pair, in ascending order of first: the rows ubh_overlap stores below min(total, capacity)"""
    assert ids_a.dtype == np.int32 and ids_b.dtype == np.int32 and ids_a.shape == ids_b.shape
    key = keys_of(ids_a, ids_b)
    q = np.flatnonzero(key != 0)
    uniq, first, inverse, pixels = np.unique(key[q], return_index=True, return_inverse=True, return_counts=True)
    out = np.zeros((len(uniq), COLUMNS), np.int64)
    out[:, 0] = (uniq >> np.uint64(32)).astype(np.int64) - 1
    out[:, 1] = (uniq & np.uint64(0xFFFFFFFF)).astype(np.int64) - 1
    out[:, 2] = q[first]                                          # np.unique returns the first occurrence
    out[:, 3] = pixels
    if view is not None:
        w, _, _ = MR.weight(view.reshape(-1)[q], adc_scale)
        np.add.at(out[:, 4], inverse.reshape(-1), (w > 0).astype(np.int64))
        np.add.at(out[:, 5], inverse.reshape(-1), w)
    return out[np.argsort(out[:, 2], kind="stable")]


# ---- the hash table in scratch ----
def default_slots(capacity):
    s = 1024
    while s < 2 * capacity:
        s *= 2
    return s


def probes(slots):
    return min(slots, MAX_PROBES)


def home_slot(key, slots):
    assert slots >= 2 and slots & (slots - 1) == 0
    return ((int(key) * GOLDEN) & MASK64) >> (64 - (slots.bit_length() - 1))


def insert(table_keys, key):
    """table_keys: dict(slots=n, held={slot: key}).  -> the slot that holds `key` after the insert, or -1 if its probes are taken"""
    slots, held = table_keys["slots"], table_keys["held"]
    h = home_slot(key, slots)
    for p in range(probes(slots)):
        s = (h + p) & (slots - 1)
        if held.setdefault(s, key) == key:
            return s
    return -1


def lookup(table_keys, key):
    slots, held = table_keys["slots"], table_keys["held"]
    h = home_slot(key, slots)
    for p in range(probes(slots)):
        s = (h + p) & (slots - 1)
        if s not in held:
            return -1
        if held[s] == key:
            return s
    return -1


def occupied(keys, slots):
    """(the set of slots the keys occupy when inserted in the order given, the keys that found none)"""
    t = dict(slots=slots, held={})
    dropped = [int(k) for k in keys if insert(t, int(k)) < 0]
    return set(t["held"]), dropped


def longest_run(occupied_slots, slots):
    """the longest cyclic run of occupied slots"""
    if len(occupied_slots) >= slots:
        return slots
    if not occupied_slots:
        return 0
    free = next(s for s in range(slots) if s not in occupied_slots)
    best = run = 0
    for i in range(1, slots + 1):
        if (free + i) & (slots - 1) in occupied_slots:
            run += 1
            best = max(best, run)
        else:
            run = 0
    return best


# ---- the brute force of the adjusted Rand index, for tiny images ----
def ari_brute_force(ids_a, ids_b):
    a, b = ids_a.reshape(-1), ids_b.reshape(-1)
    q = [i for i in range(a.size) if a[i] >= 0 and b[i] >= 0]
    if len(q) < 2:
        return float("nan")
    same_both = same_a = same_b = total = 0
    for x in range(len(q)):
        for y in range(x + 1, len(q)):
            sa, sb = a[q[x]] == a[q[y]], b[q[x]] == b[q[y]]
            same_both += int(sa and sb)
            same_a += int(sa)
            same_b += int(sb)
            total += 1
    expected = same_a * same_b / total
    top = (same_a + same_b) / 2
    return 1.0 if top == expected else (same_both - expected) / (top - expected)


# ---- the exact cases of tests/test_gpu_overlap_exact.py, built here so that tests/test_cpu_overlap.py can hold their key sets
# against the hash model: name -> (label uint8 [P, rows, cols], (connectivity, by_class) of a, the same of b, capacity) ----
RAGGED = (1, 1201, 1801)
ALL_LIT = (2, 200, 300)
MODE_A, MODE_B = (8, False), (4, True)


def ragged_label():
    """3 % lit with a slab that spans trips and workgroups and the last pixels of the view lit; 1057 trips, above the grid cap"""
    import cluster_ref as CR
    rng = np.random.default_rng(31)
    label = np.full(RAGGED, CR.FILL, np.uint8)
    lit = rng.random(RAGGED) < 0.03
    lit[0, 100:140, 200:900] = True
    lit[0, -1, -5:] = True
    label[lit] = rng.integers(0, CR.C4, int(lit.sum())).astype(np.uint8)
    return label


def clustered_cases():
    import cluster_ref as CR
    cases = {}
    for view in sorted(CR.VIEWS):
        for pattern in sorted(CR.PATTERNS):
            label = CR.PATTERNS[pattern](*CR.VIEWS[view])
            cases["%s/%s" % (pattern, view)] = (label, MODE_A, MODE_B, label.size)
    four = CR.VIEWS["four-tiles"]
    cases["self"] = (CR.PATTERNS["random-41"](*four), MODE_A, MODE_A, four[0] * four[1] * four[2])
    for pattern in ("checker", "random-41"):
        cases["direct/" + pattern] = (CR.PATTERNS[pattern](*four), (4, False), (8, False), four[0] * four[1] * four[2])
    cases["all-lit-contended"] = (CR.PATTERNS["all-lit"](*ALL_LIT), (8, False), (4, False), 7)
    cases["ragged"] = (ragged_label(), MODE_A, MODE_B, 1 << 18)
    return cases


def raw_maps():
    """two int32 maps that no clusterer made, on the four-tiles view: large ids near 2^31 - 1, values below -1, ids that are not
    contiguous, and pairs that differ only in the side that is none"""
    shape = (2, 67, 133)
    rng = np.random.default_rng(2024)
    big = np.array([2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30, 65536, 65535, 1, 0], np.int64)
    a = big[rng.integers(0, len(big), shape)]
    b = big[::-1][rng.integers(0, len(big), shape)]
    a[rng.random(shape) < 0.3] = -1
    b[rng.random(shape) < 0.3] = -1
    a[rng.random(shape) < 0.1] = -2 ** 31
    b[rng.random(shape) < 0.1] = -7
    a[0, 5:9, 10:90] = 2 ** 31 - 1                                # a run of one pair across many lanes
    b[0, 5:9, 10:90] = 2 ** 31 - 1
    return a.astype(np.int32), b.astype(np.int32)


def reference_ids(label, mode):
    """the ids map an EventClusterer of this mode writes, from the numpy reference of tests/cluster_ref.py"""
    import cluster_ref as CR
    return CR.reference(label, CR.confidence_bits(label.shape), connectivity=mode[0], by_class=mode[1])["ids"]
