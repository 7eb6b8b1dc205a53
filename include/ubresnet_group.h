/*
 * ubresnet_group.h -- C ABI of libubresnet_group.so (flat optimizer steps with parameter groups and frozen parameters: one
 * launch over a flat buffer whose per-parameter segments carry their own learning rate, weight decay, on/off switch and step
 * count; gfx950 / MI355X).
 *
 * A seventh, small library next to libubresnet_hip.so, libubresnet_post.so, libubresnet_data.so, libubresnet_aug.so,
 * libubresnet_opt.so (include/ubresnet_opt.h) and libubresnet_weight.so.  It links against none of them and shares no state
 * with them: it has its own per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_opt.h: device pointers unless stated, `stream` is a hipStream_t passed as void*, arguments
 * are validated on the host before any launch, 0 on success or a negative UBG_E* code with a message in ubg_last_error().  No
 * function allocates or frees, none but ubg_state_get synchronises, and no launch argument of a step depends on how many steps
 * were taken: the counts live on the device, one per segment, so a captured ubg_grad_norm + ubg_*_step pair replays correctly.
 *
 * The flat buffers (param, grad, moments) are n floats, n % 4 == 0, seen as n / 4 float4 UNITS.  A SEGMENT is a run of units
 * that belongs to one parameter (a parameter of numel floats occupies (numel + 3) / 4 units; padding floats are zero and stay
 * zero: a step maps a zero parameter with a zero gradient and zero state to zero).  Segments do not overlap.
 */
#ifndef UBRESNET_GROUP_H
#define UBRESNET_GROUP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBG_OK 0
#define UBG_EINVAL (-1)   /* bad argument */
#define UBG_ELAUNCH (-2)  /* hip launch or copy error */

#define UBG_BLOCK 256        /* lanes of a workgroup */
#define UBG_TILE_UNITS 1024  /* UBG_BLOCK lanes x 4 units: the most a tile holds */
#define UBG_MAX_GRID 1024    /* workgroups of the first launch of ubg_grad_norm, and fp64 partials in the control block */
#define UBG_STEP_GRID 2048   /* most workgroups of a step launch */

/* One tile: `units` (1 .. UBG_TILE_UNITS) consecutive units from unit `unit0`, all of segment `seg`.  16 bytes. */
typedef struct ubg_tile {
  int64_t unit0;
  int32_t units;
  int32_t seg;
} ubg_tile;

/* Written by the host, read by the kernels: what a segment's step uses.  16 bytes. */
typedef struct ubg_hyper {
  float lr;
  float weight_decay;
  int32_t active;   /* 0: the segment takes no part in this step: not in the norm, no byte of it read or written */
  int32_t reserved;
} ubg_hyper;

/* Written by the kernels only (ubg_state_set, ubg_grad_norm, ubg_advance): a segment's own past.  16 bytes.  Kept apart from
 * ubg_hyper so that an upload of hyper-parameters cannot overwrite a count. */
typedef struct ubg_state {
  int64_t applied;  /* steps applied to this segment so far */
  float bc1;        /* Adam: 1 - beta1^applied        (0 while applied == 0) */
  float sqrt_bc2;   /* Adam: sqrt(1 - beta2^applied)  (0 while applied == 0) */
} ubg_state;

/* The control block: device memory, UBG_CTL_BYTES long, 16-byte aligned, zeroed by the caller before its first use.  Its head
 * has the layout of ubo_ctl (include/ubresnet_opt.h), field for field at the same offsets and with the same meaning, so that
 * whatever reads a ubo_ctl reads this one; bc1 and sqrt_bc2 of the head are not used here (they are per segment, in ubg_state)
 * and `applied` counts the steps that were applied to whichever segments were active. */
typedef struct ubg_ctl {
  double sumsq;             /*  0  sum of the squares of the gradient of the ACTIVE segments */
  float norm;               /*  8  (float)(|grad_scale| * sqrt(sumsq)) */
  float scale;              /* 12  the clip coefficient */
  float gscale;             /* 16  grad_scale * scale: what the step multiplies gradients by */
  int32_t apply;            /* 20  0: the step kernels touch nothing */
  int32_t clipped;          /* 24  this step: scale < 1 */
  float bc1;                /* 28  unused (see ubg_state) */
  float sqrt_bc2;           /* 32  unused */
  int32_t reserved;         /* 36 */
  int64_t applied;          /* 40  steps applied so far, this one included */
  int64_t skipped;          /* 48  steps skipped so far */
  int64_t clipped_total;    /* 56  applied steps that were clipped */
  float row[4];             /* 64  norm, scale, apply as 0.0f / 1.0f, gscale: one fp32 row for recorders */
} ubg_ctl;
#define UBG_CTL_HEAD_BYTES 80                                  /* sizeof(ubg_ctl); the partials follow */
#define UBG_CTL_BYTES (UBG_CTL_HEAD_BYTES + 8 * UBG_MAX_GRID)  /* then UBG_MAX_GRID fp64 partials */

/* Cut segments into tiles.  Pure host code: HOST pointers, no HIP call.
 *
 *   seg_unit0, seg_units  [nseg] first unit and number of units of each segment; seg_units[s] >= 1, seg_unit0[0] >= 0 and
 *                         seg_unit0[s] >= seg_unit0[s - 1] + seg_units[s - 1] (ascending, no overlap); nseg >= 1
 *   tiles                 [cap] written: segment 0's tiles first, each segment cut into ceil(units / UBG_TILE_UNITS) tiles of
 *                         UBG_TILE_UNITS units but for a shorter last one; a tile never crosses a segment boundary and the
 *                         table is in ascending unit order
 * -> the number of tiles (>= 1), or UBG_EINVAL; with `cap` too small nothing is written at or past tiles[cap] (the tiles that
 *    fit are) and the call is refused.  Upload the table once; the step and norm calls take its device address. */
int64_t ubg_plan_tiles(const int64_t* seg_unit0, const int64_t* seg_units, int64_t nseg, ubg_tile* tiles, int64_t cap);

/* Seed the step counts of segments seg0 .. seg0 + count - 1 from a checkpoint: state[seg0 + i] = {applied[i], bc_table row of
 * applied[i]} (zeros for applied[i] == 0).  `applied` is a DEVICE array of `count` int64, each >= 0 (a negative one is stored
 * as 0).  0 <= seg0, count >= 1, seg0 + count <= nseg.  One launch.  (A fresh optimizer needs no call: zeroed state is count 0.)
 * bc_table as for ubg_grad_norm. */
int ubg_state_set(void* state, int64_t nseg, int64_t seg0, int64_t count, const int64_t* applied, const float* bc_table,
                  int64_t bc_len, void* stream);

/* Copy state[0 .. nseg) to the HOST array `out` after everything queued on `stream` has finished.  Synchronises the stream (not
 * for use under graph capture). */
int ubg_state_get(const void* state, int64_t nseg, ubg_state* out, void* stream);

/* Norm of the gradient of the active segments and the decision about the step, in two launches.
 *
 *   grad           [n] fp32, read; n > 0, n % 4 == 0, 16-byte aligned
 *   tiles, ntiles  the tile table on the device (ubg_plan_tiles); ntiles >= 1.  A tile that does not lie inside the n / 4 units,
 *                  or whose seg is not in [0, nseg), is ignored by every kernel
 *   hyper, state   [nseg] ubg_hyper (read) and ubg_state (updated); nseg >= 1; 16-byte aligned
 *   grad_scale, max_norm, skip_nonfinite, bc_table, bc_len, ctl: as for ubo_grad_norm
 *
 * First launch, grid = min(ntiles, UBG_MAX_GRID) workgroups of UBG_BLOCK lanes.  Workgroup w takes tiles w, w + grid,
 * w + 2 grid, ... in that order; a tile of an inactive segment is passed over without a load of the gradient.  Lane l of the
 * workgroup has ONE fp64 accumulator, 0.0 at the start, that lives across all tiles of the workgroup.  In a tile the lane takes
 * units unit0 + l, unit0 + l + 256, unit0 + l + 512, unit0 + l + 768, in that order, those below unit0 + units; of a unit it
 * takes the floats x, y, z, w in that order; each float f does acc = acc + (double)f * (double)f, the square exact, the sum
 * rounded once.  Then s[l] = acc, and for h = 128, 64, .., 1: s[l] = s[l] + s[l + h] for l < h (all lanes of a round read
 * before any writes); partial[w] = s[0].  There are no atomics.
 * Second launch, one workgroup:
 *   sumsq  = partial[0] + partial[1] + ... + partial[grid - 1] in index order, starting from 0.0
 *   norm   = (float)(|grad_scale| * sqrt(sumsq))
 *   scale  = max_norm < 0 ? 1.0f : fminf(max_norm / (norm + 1e-6f), 1.0f)        in fp32 (torch's clip_grad_norm_)
 *   gscale = grad_scale * scale
 *   apply  = !(skip_nonfinite && !isfinite(sumsq))
 *   applied:     applied += 1; clipped = scale < 1; clipped_total += clipped; and for EVERY ACTIVE segment s:
 *                state[s].applied += 1; (state[s].bc1, state[s].sqrt_bc2) = bc_table[min(state[s].applied, bc_len) - 1]
 *   not applied: skipped += 1; clipped = 0; no segment's state changes
 *   row    = norm, scale, apply as 0.0f / 1.0f, gscale
 * The result is the same bits from run to run. */
int ubg_grad_norm(const float* grad, int64_t n, const void* tiles, int64_t ntiles, const void* hyper, void* state, int64_t nseg,
                  float grad_scale, float max_norm, int skip_nonfinite, const float* bc_table, int64_t bc_len, void* ctl,
                  void* stream);

/* The second launch alone, for an optimizer without a guard: sumsq = 0, norm = 0, scale = 1, gscale = grad_scale, apply = 1,
 * clipped = 0, applied += 1, every active segment advances as above.  The gradient is not read. */
int ubg_advance(const void* hyper, void* state, int64_t nseg, float grad_scale, const float* bc_table, int64_t bc_len, void* ctl,
                void* stream);

/* One torch.optim.Adam step (L2 weight decay, no amsgrad) over the tiles of the active segments, one launch.  The arithmetic is
 * ubo_adam_step's operation for operation, with lr and weight_decay from hyper[seg], bc1 and sqrt_bc2 from state[seg], gscale
 * from ctl.  With ctl->apply == 0 nothing is loaded or stored; a tile of an inactive segment loads and stores nothing of the
 * four buffers.  Buffers are [n] fp32, 16-byte aligned, none overlapping ctl. */
int ubg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const void* tiles,
                  int64_t ntiles, const void* hyper, const void* state, int64_t nseg, float beta1, float beta2, float eps,
                  const void* ctl, void* stream);

/* One torch.optim.SGD step likewise (ubo_sgd_step's arithmetic); a segment's first step, which copies the gradient into the
 * momentum buffer without reading it, is the one with state[seg].applied == 1.  momentum_buf is NULL iff momentum == 0. */
int ubg_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, const void* tiles, int64_t ntiles,
                 const void* hyper, const void* state, int64_t nseg, float momentum, float dampening, int nesterov,
                 const void* ctl, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubg_last_error(void);
int ubg_version(void);

#ifdef __cplusplus
}
#endif

#endif
