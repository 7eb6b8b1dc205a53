"""numpy replay of libubresnet_stats.so (include/ubresnet_stats.h) on uint32 views: the scan as a test of the exponent field on
the bit pattern, the decision rule, and the move of every row in the decided direction.  Geometry and the control block's layout
are restated here so that tests hold the header, the binding and this file against each other."""
import numpy as np

BLOCK, SEG_GRID, CTL_BYTES = 256, 256, 32
OFFSETS = dict(keep=0, bad_rows=4, kept=8, restored=16, restored_for_stats=24)
APPLY_OFFSET = 20                        # `apply` in ubo_ctl and in ubg_ctl
KIND_F32, KIND_RAW = 0, 1
EXP = np.uint32(0x7f800000)


def scan(live, rows):
    """live: a uint32 array (the arena); rows: [(shadow offset, live offset, count, kind)] in units -> bad[] as int32"""
    bad = np.zeros(len(rows), dtype=np.int32)
    for r, (_, lo, count, kind) in enumerate(rows):
        if kind == KIND_F32 and count > 0:
            bad[r] = int(((live[lo:lo + count] & EXP) == EXP).sum())
    return bad


def decide(flag, check, bad_rows):
    """flag None: no optimizer flag.  -> (keep, for_stats)"""
    stepped = flag is None or flag != 0
    poisoned = bool(check) and bad_rows > 0
    return int(stepped and not poisoned), int(stepped and poisoned)


class Ctl(object):
    """the control block on the host"""

    def __init__(self):
        self.keep = self.bad_rows = self.kept = self.restored = self.restored_for_stats = 0

    def decide(self, bad, flag, check):
        self.bad_rows = int((np.asarray(bad) != 0).sum())
        self.keep, for_stats = decide(flag, check, self.bad_rows)
        if self.keep:
            self.kept += 1
        else:
            self.restored += 1
            self.restored_for_stats += for_stats
        return self.keep

    def fields(self):
        return (self.keep, self.bad_rows, self.kept, self.restored, self.restored_for_stats)


def note(seen, bad):
    """-> the new seen[]"""
    s = seen.astype(np.int64) + np.where(bad > 0, bad, 0)
    return np.minimum(s, 0x7fffffff).astype(np.int32)


def resolve(shadow, live, rows, keep):
    """in place on the two uint32 arenas"""
    for so, lo, count, _ in rows:
        if count > 0:
            if keep:
                shadow[so:so + count] = live[lo:lo + count]
            else:
                live[lo:lo + count] = shadow[so:so + count]

