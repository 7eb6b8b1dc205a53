/*
 * ubresnet_loss.h -- C ABI of libubresnet_loss.so (the pixel-wise focal loss of the segmentation head and its normalised means
 * on the device: -(1 - p_t)^gamma * log p_t per pixel, times a class weight and a pixel weight, divided by the number of pixels,
 * by the number of pixels that contributed or by the sum of their weights; gfx950 / MI355X).
 *
 * An eleventh, small library next to libubresnet_hip.so, libubresnet_post.so, libubresnet_data.so, libubresnet_aug.so,
 * libubresnet_opt.so, libubresnet_weight.so, libubresnet_group.so, libubresnet_ema.so, libubresnet_accum.so and
 * libubresnet_stats.so (include/ubresnet_stats.h).  It links against none of them and shares no state with them: it has its own
 * per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_accum.h and ubresnet_stats.h: device pointers, `stream` is a hipStream_t passed as void*,
 * arguments are validated on the host before any launch, 0 on success or a negative UBL_E* code with a message in
 * ubl_last_error().  No function allocates, frees or synchronises.  The denominator of the mean is known only on the device: the
 * forward leaves its reciprocal in a control block that the backward reads, so no launch argument depends on device state and a
 * forward and backward pair captures into a graph as it is.
 *
 * Arithmetic (ubresnet_amd/csrc/ubr_loss_term.h, the same inline functions on the host and on the device).  Every step is one
 * fp32 operation rounded to nearest even or one call of expf, expm1f, exp2f or log2f; none is contracted with another; subnormal
 * operands and results are kept.  With lp = predict[n, t, y, x] at the pixel's target class t, w_c = classw[t] (1 without class
 * weights), pw = pixelweights[n, y, x]:
 *
 *   p = expf(lp)
 *   x = -expm1f(lp);  q = x < 0 ? 0 : (x > 1 ? 1 : x)        (comparisons, so a NaN passes through; 1 - expf(lp) would cancel
 *                                                              where the pixel is easy, which is where the focal loss lives)
 *   m = q^gamma:  gamma == 0: 1;  gamma == 1: q;  gamma == 2: q * q;  otherwise q == 0 ? 0 : exp2f(gamma * log2f(q))
 *   term = ((-(lp * m)) * w_c) * pw                           (accumulated in fp64; at gamma == 0 this is nll_fwd_kernel's term
 *                                                              of libubresnet_hip.so, operation for operation)
 *   d = d term / d lp / (w_c pw):
 *       q == 0:  d = -m
 *       else     a = gamma * p;  b = lp / q;  c = p == 0 ? 0 : a * b;  d = m * (c - 1)
 *                (log-probabilities below the underflow of expf are normal here: c is then taken as 0.  The form
 *                q^(gamma-1) * lp is not used: it overflows for small gamma as q -> 0.)
 *   g = (((g_loss * inv_denom) * pw) * w_c) * d               (the products in the order of nll_bwd_kernel, -(g_loss / total) * pw
 *                                                              * w_c: at gamma == 0, d is exactly -1, and in UBL_MEAN_PIXELS mode
 *                                                              inv_denom = 1.0f / (float)total, so g equals that kernel's value
 *                                                              bit for bit wherever g_loss * (1 / total) == g_loss / total in
 *                                                              fp32 -- every power of two, the 1.0 of a train step among them)
 *
 * A pixel contributes iff its target is not ignore_index and lies in [0, C).  A target outside [0, C) other than ignore_index is a
 * bad label: it is counted (nll_fwd_kernel's rule) and contributes nothing.  A NaN lp at a contributing pixel gives a NaN loss and
 * a NaN gradient at that pixel, for every gamma; a guarded optimizer then skips the step.  lp = -inf gives a loss of +inf.
 *
 * The mean.  denom = N*H*W (UBL_MEAN_PIXELS, the reference's mean: ignored pixels stay in the denominator), the number of
 * contributing pixels (UBL_MEAN_VALID) or the fp64 sum of w_c * pw over them (UBL_MEAN_WEIGHTS, what torch's
 * nll_loss(weight=..., reduction="mean") divides by).  denom == 0: inv_denom = 0 and loss = 0 -- an all-ignored batch is a zero
 * loss with a zero gradient, not a NaN.  Otherwise inv_denom = 1.0f / (float)denom (one fp32 division) and
 * loss = (float)(loss_sum * (1.0 / denom)) in fp64.  A weight sum below 2^-128 has no fp32 reciprocal: inv_denom is then +inf,
 * the gradient is non-finite and a guarded optimizer skips the step.
 *
 * Reproducibility.  There is no atomic operation in the library: every workgroup of the streaming pass writes one row of fp64 /
 * u64 partials, and one workgroup adds the rows in a fixed order.  The grid is a function of N*H*W alone, so the same inputs
 * give the same bits from run to run.
 */
#ifndef UBRESNET_LOSS_H
#define UBRESNET_LOSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBL_OK 0
#define UBL_EINVAL (-1)   /* bad argument */
#define UBL_ELAUNCH (-2)  /* hip launch error */

#define UBL_MEAN_PIXELS 0   /* sum / (N*H*W) */
#define UBL_MEAN_VALID 1    /* sum / number of contributing pixels */
#define UBL_MEAN_WEIGHTS 2  /* sum / sum of classw[t] * pixelweights over the contributing pixels */

#define UBL_MAX_CLASSES 16

/* launch geometry of the streaming passes (tests derive their sizes from it): a unit is 4 consecutive pixels; a workgroup has
 * UBL_BLOCK lanes and a lane takes UBL_UNROLL units per trip, so a trip is UBL_BLOCK * UBL_UNROLL * 4 CONSECUTIVE pixels.  The
 * grid is min(ceil(N*H*W / (UBL_BLOCK * UBL_UNROLL * 4)), UBL_MAX_GRID) workgroups -- a function of N*H*W alone -- and workgroup g
 * takes the trips g, g + grid, g + 2 grid, ...  In the 4-pixel form lane l takes the units u * UBL_BLOCK + l (u < UBL_UNROLL) of
 * its trip; in the scalar form the pixels j * UBL_BLOCK + l (j < 4 * UBL_UNROLL).  The host picks the 4-pixel form iff
 * H*W % 4 == 0 and every pointer is 16-byte aligned; both forms do the same arithmetic. */
#define UBL_BLOCK 256
#define UBL_UNROLL 2
#define UBL_MAX_GRID 1024

/* one row of partials in the workspace, as 8-byte words: what one workgroup of the forward's streaming pass writes */
#define UBL_ROW_LOSS_SUM 0       /* f64 */
#define UBL_ROW_WEIGHT_SUM 1     /* f64: sum of classw[t] * pixelweights over the contributing pixels */
#define UBL_ROW_VALID 2          /* u64: contributing pixels */
#define UBL_ROW_BAD 3            /* u64: bad labels */
#define UBL_ROW_CLASS_LOSS 4     /* f64 [16] */
#define UBL_ROW_CLASS_PIXELS 20  /* u64 [16] */
#define UBL_ROW_WORDS 36
#define UBL_WORKSPACE_BYTES (UBL_MAX_GRID * UBL_ROW_WORDS * 8)   /* 16-byte aligned; its use is stream-ordered */

/* the control block, as 8-byte words: written whole by every ubl_focal_fwd, read (UBL_CTL_INV_DENOM) by ubl_focal_bwd */
#define UBL_CTL_LOSS_SUM 0       /* f64: sum of the terms */
#define UBL_CTL_WEIGHT_SUM 1     /* f64 */
#define UBL_CTL_VALID 2          /* u64 */
#define UBL_CTL_BAD 3            /* u64 (a whole word: it can be viewed as an int64 tensor) */
#define UBL_CTL_DENOM 4          /* f64: the denominator of `mode` */
#define UBL_CTL_INV_DENOM 5      /* fp32 in the low 4 bytes, the high 4 bytes zero */
#define UBL_CTL_LOSS 6           /* fp32 in the low 4 bytes, the high 4 bytes zero: what `loss` received */
#define UBL_CTL_MODE 7           /* u64: the mode of the call */
#define UBL_CTL_CLASS_LOSS 8     /* f64 [16]: per-class sums of the terms (classes >= C: 0) */
#define UBL_CTL_CLASS_PIXELS 24  /* u64 [16]: per-class contributing pixels */
#define UBL_CTL_WORDS 40
#define UBL_CTL_BYTES (UBL_CTL_WORDS * 8)

/* predict [N,C,H,W] fp32 log-probabilities, target [N,H,W] int64, pixelweights [N,H,W] fp32, classw [C] fp32 or NULL, all
 * contiguous; 1 <= C <= UBL_MAX_CLASSES; gamma finite and >= 0; mode one of UBL_MEAN_*.  workspace: UBL_WORKSPACE_BYTES, 16-byte
 * aligned; ctl: UBL_CTL_BYTES, 8-byte aligned; loss: one fp32.  Two launches: the streaming pass (rows into the workspace), then
 * one workgroup that adds the rows in row order and writes every word of ctl and *loss.  Only workspace, ctl and loss are
 * written. */
int ubl_focal_fwd(const float* predict, const int64_t* target, const float* pixelweights, const float* classw,
                  int N, int C, int H, int W, int64_t ignore_index, float gamma, int mode,
                  void* workspace, void* ctl, float* loss, void* stream);

/* g_predict [N,C,H,W] fp32 = d loss / d predict times *g_loss (a device fp32 scalar), with inv_denom read from ctl as the forward
 * over the same operands left it.  For every pixel all C channels are written: g at the target channel of a contributing pixel,
 * +0.0f everywhere else.  One launch.  Only g_predict is written. */
int ubl_focal_bwd(const float* g_loss, const void* ctl, const float* predict, const int64_t* target, const float* pixelweights,
                  const float* classw, int N, int C, int H, int W, int64_t ignore_index, float gamma,
                  float* g_predict, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubl_last_error(void);
int ubl_version(void);

#ifdef __cplusplus
}
#endif

#endif
