/*
 * ubresnet_ema.h -- C ABI of libubresnet_ema.so (exponential moving average of the parameters on the device: one streaming
 * launch per update over the flat parameter buffer, an in-place exchange of the live and the averaged buffer for evaluation,
 * and the same two operations over a table of small tensors for the BatchNorm statistics; gfx950 / MI355X).
 *
 * An eighth, small library next to libubresnet_hip.so, libubresnet_post.so, libubresnet_data.so, libubresnet_aug.so,
 * libubresnet_opt.so (include/ubresnet_opt.h), libubresnet_weight.so and libubresnet_group.so.  It links against none of them
 * and shares no state with them: it has its own per-thread error string and its launches are plain <<<>>> on the stream it is
 * given.
 *
 * Conventions are those of ubresnet_opt.h: device pointers unless stated, `stream` is a hipStream_t passed as void*, arguments
 * are validated on the host before any launch, 0 on success or a negative UBE_E* code with a message in ube_last_error().  No
 * function allocates, frees or synchronises, and no launch argument depends on how many updates have happened: the count, the
 * weight of this update and whether it is applied at all sit in the control block on the device, so a captured
 * ube_advance + ube_update (+ ube_update_segs) sequence replays correctly.
 */
#ifndef UBRESNET_EMA_H
#define UBRESNET_EMA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBE_OK 0
#define UBE_EINVAL (-1)   /* bad argument */
#define UBE_ELAUNCH (-2)  /* hip launch error */

/* launch geometry of ube_update and ube_swap (tests derive their sizes from it): a flat buffer is n / 4 float4 units; a
 * workgroup has UBE_BLOCK lanes and a lane takes UBE_UNROLL units per trip, so a workgroup's trip is UBE_BLOCK * UBE_UNROLL
 * units; the grid is min(ceil(units / (UBE_BLOCK * UBE_UNROLL)), UBE_MAX_GRID) workgroups -- a function of n alone -- and a
 * trip of the whole grid is grid * UBE_BLOCK * UBE_UNROLL units: unit base + u * grid * UBE_BLOCK (u < UBE_UNROLL) belongs to
 * lane (base mod grid * UBE_BLOCK).  The two table calls run min(nseg, UBE_SEG_GRID) workgroups of UBE_BLOCK lanes; workgroup g
 * takes rows g, g + grid, g + 2 grid, ... */
#define UBE_BLOCK 256
#define UBE_UNROLL 4
#define UBE_MAX_GRID 1024
#define UBE_SEG_GRID 256

/* The control block: device memory, UBE_CTL_BYTES long, 16-byte aligned, allocated once by the caller and set up with
 * ube_ctl_init.  Written by ube_advance, read by ube_update / ube_update_segs.  The offsets are fixed. */
typedef struct ube_ctl {
  int32_t apply;     /*  0  0: the update kernels return at once */
  float w;           /*  4  (float)(1 - d) of the last applied update: what (param - shadow) is multiplied by */
  float d;           /*  8  (float)d of the last applied update (for logs) */
  int32_t reserved;  /* 12 */
  int64_t updates;   /* 16  updates applied so far */
  int64_t held;      /* 24  updates withheld so far */
} ube_ctl;
#define UBE_CTL_BYTES 32 /* sizeof(ube_ctl) */

/* One row of the table of ube_update_segs / ube_swap_segs: `count` fp32 values at device address `shadow` and as many at
 * device address `live`, both 4-byte aligned; the two runs of a row do not overlap, and no run overlaps a run of another row.
 * A row with count <= 0 is passed over.  32 bytes. */
typedef struct ube_seg {
  uint64_t shadow;
  uint64_t live;
  int64_t count;
  int64_t reserved;
} ube_seg;

/* zero the block, then updates = `updates` (>= 0): the count a checkpoint carries.  One launch. */
int ube_ctl_init(void* ctl, int64_t updates, void* stream);

/* Decide this update, in one launch of one lane.
 *
 *   apply_flag  device address of an int32 (4-byte aligned, outside `ctl`), or NULL.  NULL: the update is applied.  Otherwise it
 *               is applied iff *apply_flag != 0.  (The `apply` field of a ubo_ctl or ubg_ctl, byte 20 of the block.)
 *   decay       the decay the average settles at; 0 <= decay < 1, NaN is refused
 *   warmup      >= 0; below 2 the decay is `decay` from the first update on
 *
 * With u = ctl->updates before the call (ube_schedule of csrc/ubr_ema_sched.h, fp64 throughout):
 *   d = warmup >= 2 ? min((double)decay, (1.0 + u) / (warmup + u)) : (double)decay
 *   w = (float)(1.0 - d)
 *   applied:  apply = 1; updates = u + 1; ctl->w = w; ctl->d = (float)d
 *   withheld: apply = 0; held += 1; w, d and updates stay */
int ube_advance(void* ctl, const int32_t* apply_flag, float decay, int64_t warmup, void* stream);

/* shadow = shadow + w * (param - shadow) element for element, w from `ctl`: three fp32 operations, each rounded to nearest
 * even, none contracted; subnormal operands and results are kept.  With ctl->apply == 0 the kernel returns before any load or
 * store of either buffer.  shadow, param: [n] fp32, n > 0, n % 4 == 0, 16-byte aligned, overlapping neither each other nor
 * `ctl`.  12 bytes of traffic per element. */
int ube_update(float* shadow, const float* param, int64_t n, const void* ctl, void* stream);

/* Exchange the contents of a and b in place, as 16-byte integer units: every bit pattern survives.  a, b: [n] fp32, n > 0,
 * n % 4 == 0, 16-byte aligned, not overlapping.  There is no control block: the call always acts. */
int ube_swap(float* a, float* b, int64_t n, void* stream);

/* ube_update's arithmetic over the rows of a device table of `nseg` ube_seg (8-byte aligned, not overlapping `ctl`):
 * row.shadow[i] = row.shadow[i] + w * (row.live[i] - row.shadow[i]) for i < row.count.  Scalar loads, one launch.  With
 * ctl->apply == 0 neither the table nor any run is read.  nseg >= 1. */
int ube_update_segs(const void* table, int64_t nseg, const void* ctl, void* stream);

/* ube_swap over the rows of such a table (32-bit integer loads and stores): row.shadow[i] <-> row.live[i]. */
int ube_swap_segs(const void* table, int64_t nseg, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ube_last_error(void);
int ube_version(void);

#ifdef __cplusplus
}
#endif

#endif
