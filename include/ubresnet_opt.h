/*
 * ubresnet_opt.h -- C ABI of libubresnet_opt.so (guarded flat optimizer step: global gradient norm, clipping by that norm and
 * the skip of a non-finite step, all decided on the device; gfx950 / MI355X).
 *
 * A fifth, small library next to libubresnet_hip.so (include/ubresnet_hip.h), libubresnet_post.so (include/ubresnet_post.h),
 * libubresnet_data.so (include/ubresnet_data.h) and libubresnet_aug.so (include/ubresnet_aug.h).  It links against none of
 * them and shares no state with them: it has its own per-thread error string and its launches are plain <<<>>> on the stream
 * it is given.
 *
 * Conventions are those of ubresnet_aug.h: device pointers unless stated, `stream` is a hipStream_t passed as void*, arguments
 * are validated on the host before any launch, 0 on success or a negative UBO_E* code with a message in ubo_last_error().  No
 * function allocates, frees or synchronises, and no launch argument depends on how many steps were taken: what a step needs to
 * know about the past sits in the control block on the device, so a captured ubo_grad_norm + ubo_*_step pair replays correctly.
 */
#ifndef UBRESNET_OPT_H
#define UBRESNET_OPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBO_OK 0
#define UBO_EINVAL (-1)   /* bad argument */
#define UBO_ELAUNCH (-2)  /* hip launch error */

/* launch geometry of the first launch of ubo_grad_norm (tests derive their sizes from it): the gradient is n / 4 float4 units;
 * a workgroup has UBO_BLOCK lanes and a lane takes UBO_UNROLL units per trip, so a workgroup's trip is UBO_BLOCK * UBO_UNROLL
 * units; the grid is min(ceil(units / (UBO_BLOCK * UBO_UNROLL)), UBO_MAX_GRID) workgroups -- a function of n alone -- and a
 * trip of the whole grid is grid * UBO_BLOCK * UBO_UNROLL units: unit base + u * grid * UBO_BLOCK (u < UBO_UNROLL) belongs to
 * lane (base mod grid * UBO_BLOCK).  Every workgroup writes one fp64 partial; there are no atomics. */
#define UBO_BLOCK 256
#define UBO_UNROLL 4
#define UBO_MAX_GRID 1024

/* The control block: device memory, UBO_CTL_BYTES long, 16-byte aligned, allocated once by the caller and set up with
 * ubo_ctl_init.  Written by ubo_grad_norm, read by ubo_adam_step / ubo_sgd_step.  (ubo_ctl is this layout for host code that
 * copies the block back; the offsets are fixed.) */
typedef struct ubo_ctl {
  double sumsq;             /*  0  sum of the squares of the gradient, each square and the sum in fp64 */
  float norm;               /*  8  (float)(|grad_scale| * sqrt(sumsq)) */
  float scale;              /* 12  the clip coefficient */
  float gscale;             /* 16  grad_scale * scale: what the step multiplies gradients by */
  int32_t apply;            /* 20  0: the step kernels return at once */
  int32_t clipped;          /* 24  this step: scale < 1 */
  float bc1;                /* 28  Adam: 1 - beta1^applied */
  float sqrt_bc2;           /* 32  Adam: sqrt(1 - beta2^applied) */
  int32_t reserved;         /* 36 */
  int64_t applied;          /* 40  steps applied so far, this one included */
  int64_t skipped;          /* 48  steps skipped so far */
  int64_t clipped_total;    /* 56  applied steps that were clipped */
  float row[4];             /* 64  norm, scale, apply as 0.0f / 1.0f, gscale: one fp32 row for recorders */
} ubo_ctl;
#define UBO_CTL_HEAD_BYTES 80                                  /* sizeof(ubo_ctl); the partials follow */
#define UBO_CTL_BYTES (UBO_CTL_HEAD_BYTES + 8 * UBO_MAX_GRID)  /* then UBO_MAX_GRID fp64 partials */

/* zero the whole block (partials included), then applied = `applied` (>= 0): the count a checkpoint carries.  One launch. */
int ubo_ctl_init(void* ctl, int64_t applied, void* stream);

/* Global norm of the flat gradient and the decision about the step, in two launches.
 *
 *   grad           [n] fp32, read; n > 0, n % 4 == 0, 16-byte aligned (padding inside the buffer must be zero)
 *   grad_scale     what the caller wants the gradient multiplied by before anything else (1 / loss scale, 1 / world size)
 *   max_norm       clip the scaled gradient to this global L2 norm; < 0: no clipping; NaN is refused
 *   skip_nonfinite nonzero: a step whose sumsq is NaN or infinite is not applied
 *   bc_table       [bc_len][2] fp32, read: Adam's bias corrections (1 - beta1^t, sqrt(1 - beta2^t)) for t = 1 .. bc_len, the
 *                  last row standing for every later t; bc_len >= 1.  (SGD: any one row.)
 *   ctl            the control block
 *
 * First launch: each square is formed in fp64 from the fp32 value (exact) and added in fp64; a lane adds its units in
 * ascending order, a workgroup adds its lanes in a fixed tree, and writes partial[workgroup].  Second launch, one workgroup:
 *   sumsq  = partial[0] + partial[1] + ... in index order
 *   norm   = (float)(|grad_scale| * sqrt(sumsq))
 *   scale  = max_norm < 0 ? 1.0f : fminf(max_norm / (norm + 1e-6f), 1.0f)        in fp32 (torch's clip_grad_norm_)
 *   gscale = grad_scale * scale
 *   apply  = !(skip_nonfinite && !isfinite(sumsq))
 *   applied:     applied += 1; clipped = scale < 1; clipped_total += clipped;
 *                (bc1, sqrt_bc2) = bc_table[min(applied, bc_len) - 1]
 *   not applied: skipped += 1; clipped = 0; bc1 and sqrt_bc2 stay
 * The result is the same bits from run to run. */
int ubo_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, int skip_nonfinite,
                  const float* bc_table, int64_t bc_len, void* ctl, void* stream);

/* One torch.optim.Adam step (L2 weight decay, no amsgrad) over flat buffers: the arithmetic of ubr_adam_step
 * (include/ubresnet_hip.h) operation for operation, with gscale, bc1 and sqrt_bc2 read from `ctl`.  With ctl->apply == 0 the
 * kernel returns before any load or store of the four buffers.  n > 0, n % 4 == 0; all buffers 16-byte aligned, none
 * overlapping `ctl`. */
int ubo_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, const void* ctl, void* stream);

/* One torch.optim.SGD step likewise (ubr_sgd_step's arithmetic); the first step, which copies the gradient into the momentum
 * buffer without reading it, is the one with ctl->applied == 1.  momentum_buf is NULL iff momentum == 0. */
int ubo_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                 float weight_decay, int nesterov, const void* ctl, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubo_last_error(void);
int ubo_version(void);

#ifdef __cplusplus
}
#endif

#endif
