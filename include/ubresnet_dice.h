/*
 * ubresnet_dice.h -- C ABI of libubresnet_dice.so (the soft Dice / Tversky region loss of the segmentation head on the device:
 * one minus the class-weighted mean over the classes of (TP + eps) / (TP + alpha FP + beta FN + eps), with TP, FP and FN the
 * batch-wide soft counts; gfx950 / MI355X).
 *
 * A twelfth, small library next to libubresnet_hip.so, libubresnet_post.so, libubresnet_data.so, libubresnet_aug.so,
 * libubresnet_opt.so, libubresnet_weight.so, libubresnet_group.so, libubresnet_ema.so, libubresnet_accum.so, libubresnet_stats.so
 * and libubresnet_loss.so (include/ubresnet_loss.h).  It links against none of them and shares no state with them: it has its own
 * per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_loss.h: device pointers, `stream` is a hipStream_t passed as void*, arguments are validated on
 * the host before any launch, 0 on success or a negative UBK_E* code with a message in ubk_last_error().  No function allocates,
 * frees or synchronises.  The gradient of a pixel depends on the batch-wide sums: the forward leaves two coefficients per class in
 * a control block that the backward reads, so no launch argument depends on device state and a forward and backward pair captures
 * into a graph as it is.
 *
 * A pixel contributes iff its target is not ignore_index and lies in [0, C).  A target outside [0, C) other than ignore_index is a
 * bad label: it is counted and contributes nothing.
 *
 * The sums (ubresnet_amd/csrc/ubr_dice_term.h, the same inline functions on the host and on the device).  With lp_c =
 * predict[n, c, y, x], t the pixel's target and pw = pixelweights[n, y, x] (expected >= 0), at every contributing pixel:
 *
 *   p_c = expf(lp_c)                                            for every channel c
 *   x = -expm1f(lp_t);  q = x < 0 ? 0 : (x > 1 ? 1 : x)         (comparisons, so a NaN passes through; 1 - expf(lp_t) would cancel
 *                                                                where the pixel is easy)
 *   TP_t += pw * p_t;   FN_t += pw * q;   FP_c += pw * p_c  (c != t);   n_t += 1
 *
 * Each product is one fp32 multiply, not contracted with anything, promoted to fp64 afterwards; the sums are fp64 (n: u64) over the
 * whole batch.  Every addend is non-negative, so nothing cancels for any parameter.
 *
 * The finish (ubk::finish_class, fp64).  w_c = classw[c] (1 without class weights, expected >= 0); present_c = n_c > 0 if
 * present_only, else 1 -- the integer count, never a float; S = sum_c w_c present_c in class order; a_c = w_c present_c / S:
 *
 *   Nn_c = TP_c + eps;   M_c = alpha FP_c + beta FN_c;   Dn_c = TP_c + M_c + eps
 *   T_c = Nn_c / Dn_c                                           (Dn_c == 0: T_c = 1 and both coefficients 0)
 *   loss = (float) sum_c a_c (1 - T_c),  1 - T_c taken as M_c / Dn_c, the same number without the cancellation
 *   K1_c = (float)(-a_c (beta Nn_c + M_c) / Dn_c^2)             d loss / d lp_t = pw p_t K1_t at a pixel of class t
 *   K0_c = (float)( a_c alpha Nn_c / Dn_c^2)                    d loss / d lp_c = pw p_c K0_c at a pixel of another class
 *   S == 0 (nothing contributed under present_only, or all class weights zero): loss = 0 and every coefficient 0 -- an
 *   all-ignored batch is a zero loss with a zero gradient, not a NaN.
 *
 * alpha = beta = 0.5 is soft Dice, (2 TP + 2 eps) / (2 TP + FP + FN + 2 eps); alpha < beta prices a missed pixel above a false
 * alarm.  The coefficients are formed in fp64 from positive terms only and rounded to fp32 once.
 *
 * The backward.  g_c = ((g_loss * pw) * p_c) * (c == t ? K1_c : K0_c) at a contributing pixel, three fp32 multiplies in that order,
 * p_c = expf(lp_c) as in the forward; +0.0f in every channel of every other pixel.  The gradient is with respect to each
 * log-probability as an independent input: the log-softmax backward follows it.
 *
 * Non-finite values.  A NaN lp_c at a contributing pixel makes TP_c, FP_c or FN_c NaN: the loss is NaN, and K1_c and K0_c are NaN,
 * so channel c's gradient is NaN at every contributing pixel; the other channels stay finite.  A guarded optimizer then skips the
 * step.  lp = -inf gives p = 0 and q = 1, and everything stays finite.  Nothing of a pixel that does not contribute is looked at.
 *
 * Reproducibility.  There is no atomic operation in the library: every workgroup of the streaming pass writes one row of fp64 /
 * u64 partials, and one workgroup adds the rows in a fixed order.  The grid is a function of N*H*W alone, so the same inputs give
 * the same bits from run to run.
 */
#ifndef UBRESNET_DICE_H
#define UBRESNET_DICE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBK_OK 0
#define UBK_EINVAL (-1)   /* bad argument */
#define UBK_ELAUNCH (-2)  /* hip launch error */

#define UBK_MAX_CLASSES 16
#define UBK_REG_CLASSES 4   /* C <= UBK_REG_CLASSES: a forward instantiated for that C; above: one generic instantiation */

/* launch geometry of the streaming passes (tests derive their sizes from it): a unit is 4 consecutive pixels; a workgroup has
 * UBK_BLOCK lanes and a lane takes UBK_UNROLL units per trip, so a trip is UBK_BLOCK * UBK_UNROLL * 4 CONSECUTIVE pixels.  The
 * grid is min(ceil(N*H*W / (UBK_BLOCK * UBK_UNROLL * 4)), UBK_MAX_GRID) workgroups -- a function of N*H*W alone -- and workgroup g
 * takes the trips g, g + grid, g + 2 grid, ...  In the 4-pixel form lane l takes the units u * UBK_BLOCK + l (u < UBK_UNROLL) of
 * its trip, 16 bytes per channel and unit; in the scalar form the pixels j * UBK_BLOCK + l (j < 4 * UBK_UNROLL).  The host picks
 * the 4-pixel form iff H*W % 4 == 0 and every pointer is 16-byte aligned; both forms do the same arithmetic.  The forward moves
 * 4 C + 12 bytes per pixel, the backward 8 C + 12. */
#define UBK_BLOCK 256
#define UBK_UNROLL 2
#define UBK_MAX_GRID 1024

/* one row of partials in the workspace, as 8-byte words: what one workgroup of the forward's streaming pass writes */
#define UBK_ROW_TP 0         /* f64 [16] */
#define UBK_ROW_FP 16        /* f64 [16] */
#define UBK_ROW_FN 32        /* f64 [16] */
#define UBK_ROW_PIXELS 48    /* u64 [16]: contributing pixels per class */
#define UBK_ROW_VALID 64     /* u64: contributing pixels */
#define UBK_ROW_BAD 65       /* u64: bad labels */
#define UBK_ROW_WORDS 66
#define UBK_WORKSPACE_BYTES (UBK_MAX_GRID * UBK_ROW_WORDS * 8)   /* 16-byte aligned; its use is stream-ordered */

/* the control block, as 8-byte words: written whole by every ubk_dice_fwd, read (UBK_CTL_K1, UBK_CTL_K0) by ubk_dice_bwd.  Words
 * 0 .. 65 are the row words above, summed; classes >= C hold 0. */
#define UBK_CTL_TP 0         /* f64 [16] */
#define UBK_CTL_FP 16        /* f64 [16] */
#define UBK_CTL_FN 32        /* f64 [16] */
#define UBK_CTL_PIXELS 48    /* u64 [16] */
#define UBK_CTL_VALID 64     /* u64 */
#define UBK_CTL_BAD 65       /* u64 (a whole word: it can be viewed as an int64 tensor) */
#define UBK_CTL_T 66         /* f64 [16]: the Tversky index of the class */
#define UBK_CTL_K1 82        /* [16], fp32 in the low 4 bytes, the high 4 bytes zero */
#define UBK_CTL_K0 98        /* [16], likewise */
#define UBK_CTL_S 114        /* f64: sum of classw[c] * present_c */
#define UBK_CTL_LOSS 115     /* fp32 in the low 4 bytes, the high 4 bytes zero: what `loss` received */
#define UBK_CTL_WORDS 116
#define UBK_CTL_BYTES (UBK_CTL_WORDS * 8)

/* predict [N,C,H,W] fp32 log-probabilities, target [N,H,W] int64, pixelweights [N,H,W] fp32, classw [C] fp32 or NULL, all
 * contiguous; 1 <= C <= UBK_MAX_CLASSES; alpha, beta and eps finite and >= 0; present_only 0 or 1.  workspace:
 * UBK_WORKSPACE_BYTES, 16-byte aligned; ctl: UBK_CTL_BYTES, 8-byte aligned; loss: one fp32.  Two launches: the streaming pass (rows
 * into the workspace), then one workgroup that adds the rows in a fixed order and writes every word of ctl and *loss.  Only
 * workspace, ctl and loss are written. */
int ubk_dice_fwd(const float* predict, const int64_t* target, const float* pixelweights, const float* classw,
                 int N, int C, int H, int W, int64_t ignore_index, float alpha, float beta, float eps, int present_only,
                 void* workspace, void* ctl, float* loss, void* stream);

/* g_predict [N,C,H,W] fp32 = d loss / d predict times *g_loss (a device fp32 scalar), with K1 and K0 read from ctl as the forward
 * over the same operands left them.  For every pixel all C channels are written.  One launch.  Only g_predict is written. */
int ubk_dice_bwd(const float* g_loss, const void* ctl, const float* predict, const int64_t* target, const float* pixelweights,
                 int N, int C, int H, int W, int64_t ignore_index, float* g_predict, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubk_last_error(void);
int ubk_version(void);

#ifdef __cplusplus
}
#endif

#endif
