/*
 * ubresnet_accum.h -- C ABI of libubresnet_accum.so (gradient accumulation over the flat gradient buffer on the device: the
 * first micro-batch of a cycle is copied into an accumulator, the ones in between are added to it, and the last call writes
 * the scaled sum back into the flat gradient buffer in place, where the optimizers read it; gfx950 / MI355X).
 *
 * A ninth, small library next to libubresnet_hip.so, libubresnet_post.so, libubresnet_data.so, libubresnet_aug.so,
 * libubresnet_opt.so, libubresnet_weight.so, libubresnet_group.so and libubresnet_ema.so (include/ubresnet_ema.h).  It links
 * against none of them and shares no state with them: it has its own per-thread error string and its launches are plain <<<>>>
 * on the stream it is given.
 *
 * Conventions are those of ubresnet_ema.h: device pointers, `stream` is a hipStream_t passed as void*, arguments are validated
 * on the host before any launch, 0 on success or a negative UBC_E* code with a message in ubc_last_error().  No function
 * allocates, frees or synchronises.  There is no control block: which of the three calls a micro-batch gets is known to the host
 * (it counts the micro-batches; nothing the device decides enters), so no launch argument depends on device state and a whole
 * cycle captures into a graph as it is.
 *
 * Arithmetic.  Every operation is one fp32 operation rounded to nearest even (__fadd_rn, __fmul_rn); none is contracted with
 * another.  Subnormal operands and results are kept, nothing is flushed.  A NaN operand gives a NaN result; which NaN (its
 * payload) is not part of the contract.  ubc_set looks at no value: it moves 16-byte integer units, so every bit pattern,
 * NaN payloads included, arrives as it was.
 */
#ifndef UBRESNET_ACCUM_H
#define UBRESNET_ACCUM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBC_OK 0
#define UBC_EINVAL (-1)   /* bad argument */
#define UBC_ELAUNCH (-2)  /* hip launch error */

/* launch geometry of the three calls (tests derive their sizes from it): a buffer is n / 4 float4 units; a workgroup has
 * UBC_BLOCK lanes and a lane takes UBC_UNROLL units per trip, so a workgroup's trip is UBC_BLOCK * UBC_UNROLL CONSECUTIVE
 * units (16 KiB of each buffer): trip t covers the units [t * UBC_BLOCK * UBC_UNROLL, (t + 1) * UBC_BLOCK * UBC_UNROLL), lane l
 * of the workgroup takes the units t * UBC_BLOCK * UBC_UNROLL + u * UBC_BLOCK + l (u < UBC_UNROLL).  The grid is
 * min(ceil(units / (UBC_BLOCK * UBC_UNROLL)), UBC_MAX_GRID) workgroups -- a function of n alone -- and workgroup g takes the
 * trips g, g + grid, g + 2 grid, ... */
#define UBC_BLOCK 256
#define UBC_UNROLL 4
#define UBC_MAX_GRID 1024

/* Every call below: acc, grad are [n] fp32 in device memory, n > 0, n % 4 == 0, both 16-byte aligned, not overlapping. */

/* acc[i] = grad[i], as 16-byte integer units (every bit pattern survives).  Only acc is written.  8 bytes of traffic per
 * element.  The first micro-batch of a cycle. */
int ubc_set(float* acc, const float* grad, int64_t n, void* stream);

/* acc[i] = acc[i] + grad[i].  Only acc is written.  12 bytes per element.  A micro-batch that is neither the first nor the last. */
int ubc_add(float* acc, const float* grad, int64_t n, void* stream);

/* grad[i] = (acc[i] + grad[i]) * scale: the sum is rounded, then the product.  Only grad is written; acc is left as it is.
 * `scale` is a launch argument, finite and > 0 (1 / micro-batches for the mean, 1 for the sum).  12 bytes per element.  The last
 * micro-batch of a cycle: the flat gradient buffer then holds what the optimizer steps on. */
int ubc_finish(float* grad, const float* acc, int64_t n, float scale, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubc_last_error(void);
int ubc_version(void);

#ifdef __cplusplus
}
#endif

#endif
