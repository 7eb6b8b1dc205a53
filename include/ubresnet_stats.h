/*
 * ubresnet_stats.h -- C ABI of libubresnet_stats.so (a guard for the BatchNorm running statistics: a shadow copy of every
 * running_mean / running_var / num_batches_tracked, and after each optimizer step either shadow <- live, the step stands, or
 * live <- shadow, the statistics go back to what they were before the forward pass or passes of that step; which of the two is
 * decided on the device; gfx950 / MI355X).
 *
 * A tenth, small library next to libubresnet_hip.so, libubresnet_post.so, libubresnet_data.so, libubresnet_aug.so,
 * libubresnet_opt.so, libubresnet_weight.so, libubresnet_group.so, libubresnet_ema.so (include/ubresnet_ema.h) and
 * libubresnet_accum.so.  It links against none of them and shares no state with them: it has its own per-thread error string and
 * its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_ema.h: device pointers unless stated, `stream` is a hipStream_t passed as void*, arguments
 * are validated on the host before any launch, 0 on success or a negative UBS_E* code with a message in ubs_last_error().  No
 * function allocates, frees or synchronises, and no launch argument depends on what happened: the verdict and the counters sit in
 * the control block on the device, so a captured ubs_scan + ubs_note + ubs_decide + ubs_resolve sequence replays correctly.
 */
#ifndef UBRESNET_STATS_H
#define UBRESNET_STATS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBS_OK 0
#define UBS_EINVAL (-1)   /* bad argument */
#define UBS_ELAUNCH (-2)  /* hip launch error */

/* launch geometry (tests derive their sizes from it): ubs_scan and ubs_resolve run min(nseg, UBS_SEG_GRID) workgroups of
 * UBS_BLOCK lanes; workgroup g takes rows g, g + grid, g + 2 grid, ...; lane l of it takes units l, l + UBS_BLOCK, ... of a
 * row.  ubs_ctl_init, ubs_decide and ubs_note are one workgroup each. */
#define UBS_BLOCK 256
#define UBS_SEG_GRID 256

/* The control block: device memory, UBS_CTL_BYTES long, 16-byte aligned, allocated once by the caller and set up with
 * ubs_ctl_init.  Written by ubs_decide, read by ubs_resolve.  The offsets are fixed. */
typedef struct ubs_ctl {
  int32_t keep;               /*  0  the last verdict: != 0 commit (shadow <- live), 0 restore (live <- shadow) */
  int32_t bad_rows;           /*  4  rows with bad[r] != 0 at the last decision */
  int64_t kept;               /*  8  commits so far */
  int64_t restored;           /* 16  restores so far */
  int64_t restored_for_stats; /* 24  of these, the restores that the optimizer's flag alone would not have caused */
} ubs_ctl;
#define UBS_CTL_BYTES 32 /* sizeof(ubs_ctl) */

/* One row of the table: `count` 4-byte units at device address `shadow` and as many at device address `live`, both 4-byte
 * aligned; the two runs of a row do not overlap, and no run overlaps a run of another row.  A row with count <= 0 is passed
 * over.  An int64 scalar (num_batches_tracked) is a row of 2 units.  32 bytes. */
#define UBS_KIND_F32 0 /* fp32 values: scanned for non-finite ones */
#define UBS_KIND_RAW 1 /* raw units: never scanned */
typedef struct ubs_seg {
  uint64_t shadow;
  uint64_t live;
  int64_t count;
  int64_t kind;
} ubs_seg;

/* zero the block.  One launch. */
int ubs_ctl_init(void* ctl, void* stream);

/* bad[r] <- for a row of kind UBS_KIND_F32, the number of its LIVE units whose exponent field is all ones (infinities and NaNs
 * of either sign and any payload; tested on the bit pattern, no floating-point compare), at most INT32_MAX; 0 for a row of any
 * other kind and for an empty row.  `table`: `nseg` ubs_seg, 8-byte aligned; `bad`: int32[nseg], 4-byte aligned, not
 * overlapping the table.  A workgroup reduces a row's count in its local memory and stores it once: no atomics, the same result
 * on every run.  Only `bad` is written.  nseg >= 1. */
int ubs_scan(const void* table, int64_t nseg, int32_t* bad, void* stream);

/* seen[r] <- min(seen[r] + bad[r], INT32_MAX) for bad[r] > 0: what ubs_scan found, kept past the next clean scan so that a log
 * read at the end of an epoch can still name the site.  seen, bad: int32[nseg], 4-byte aligned, not overlapping.  One workgroup. */
int ubs_note(int32_t* seen, const int32_t* bad, int64_t nseg, void* stream);

/* Decide, in one launch of one workgroup (ubs::decide of csrc/ubr_stats_decide.h):
 *
 *   bad_rows = number of r < nseg with bad[r] != 0
 *   keep     = (apply_flag == NULL || *apply_flag != 0) && !(check && bad_rows > 0)
 *   keep:  kept += 1        else: restored += 1, and restored_for_stats += 1 if (apply_flag == NULL || *apply_flag != 0)
 *
 *   apply_flag  device address of an int32 (4-byte aligned, outside `ctl`), or NULL: what ube_advance takes, the `apply` field
 *               of a ubo_ctl or ubg_ctl, byte 20 of the block
 *   check       0: what `bad` holds is counted into bad_rows but never causes a restore
 * Each counter moves exactly once per call.  `bad` overlaps neither `ctl` nor the flag. */
int ubs_decide(void* ctl, const int32_t* bad, int64_t nseg, const int32_t* apply_flag, int32_t check, void* stream);

/* ctl->keep != 0: row.shadow[i] = row.live[i]; else row.live[i] = row.shadow[i], for i < row.count of every row.  All moves are
 * 32-bit integer loads and stores: every bit pattern survives (NaN payloads, -0.0, subnormals, the two halves of an int64).
 * `ctl` overlaps no part of the table.  One launch. */
int ubs_resolve(const void* table, int64_t nseg, const void* ctl, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubs_last_error(void);
int ubs_version(void);

#ifdef __cplusplus
}
#endif

#endif
