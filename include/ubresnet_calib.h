/*
 * ubresnet_calib.h -- C ABI of libubresnet_calib.so (temperature calibration of the class scores, gfx950 / MI355X).
 *
 * A small library next to libubresnet_hip.so (include/ubresnet_hip.h).  It links against none of the others and shares no
 * state with them: it has its own per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_post.h: device pointers unless stated, `stream` is a hipStream_t passed as void*,
 * arguments are validated on the host before anything touches the device, 0 on success or a negative UBF_E* code with a
 * message in ubf_last_error().  No function allocates, frees or synchronises.  No atomic operation is used and no workgroup
 * waits for another: the same call on the same data gives the same bits.
 *
 * The model.  beta = 1 / T is the inverse temperature.  For the C scores l_c of a pixel (log-probabilities or any logits)
 * with truth t, p = softmax(beta l) and lse = log-sum-exp:
 *     NLL(beta) = lse_c(beta l_c) - beta l_t        (convex in beta)
 *     g = dNLL / dbeta     = E_p[l] - l_t
 *     h = d2NLL / dbeta2   = Var_p[l] >= 0
 * All three are unchanged when a constant is added to the l_c of a pixel; the kernels subtract the pixel's maximum first:
 * d_c = l_c - max_c l_c (fp32), e_c = expf(beta d_c), S = sum_c e_c in class order, and
 *     NLL = logf(S) - beta d_t,   g = (sum_c e_c d_c) / S - d_t,   h = (sum_c e_c (d_c - mean)^2) / S,   mean = (sum_c e_c d_c) / S,
 * every operation a separate fp32 operation (no contraction).
 */
#ifndef UBRESNET_CALIB_H
#define UBRESNET_CALIB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBF_OK 0
#define UBF_EINVAL (-1)   /* bad argument */
#define UBF_ELAUNCH (-2)  /* hip launch error */

#define UBF_MAX_CLASSES 16
#define UBF_REG_CLASSES 4  /* C <= UBF_REG_CLASSES: kernels with the class count a constant; above: one kernel, runtime C */
#define UBF_MAX_TEMPS 64   /* K: one lane of a wave per inverse temperature */
#define UBF_MAX_GROUPS 256
#define UBF_MAX_IMAGES 65535
#define UBF_TRUTH_U8 0     /* truth is uint8_t */
#define UBF_TRUTH_I64 1    /* truth is int64_t */

/* bytes of scratch ubf_accumulate needs for N images of H x W and K inverse temperatures (a multiple of 8), or 0 with a message
 * for what the call refuses (N outside 1..UBF_MAX_IMAGES, H or W < 1, N * H * W above 2^40, K outside 1..UBF_MAX_TEMPS). */
int64_t ubf_scratch_bytes(int N, int H, int W, int K);

/* Add one batch to a fit.
 *
 *   scores     [N][C][H][W] float32
 *   truth      [N][H][W] uint8_t (truth_kind UBF_TRUTH_U8) or int64_t (UBF_TRUTH_I64); a class <=> 0 <= t < C on the full
 *              width of the type
 *   lit        [N][H][W] float32 or NULL.  A pixel COUNTS <=> lit == NULL or lit[n][y][x] > lit_threshold (strict; NaN does
 *              not count).  lit_threshold must not be NaN.
 *   group      [N] uint8_t: the group (wire plane) of image n.  An image whose group is >= G adds nothing.
 *   betas      [K] float32, positive and finite (not checked: they are on the device)
 *   table      double [G][K][3]: {sum NLL, sum g, sum h} per group and inverse temperature; ADDED to
 *   counters   uint64 [G][3]: {counted, ignored, non-finite}; ADDED to
 *   scratch    ubf_scratch_bytes(N, H, W, K) bytes, 8-byte aligned, overlapping nothing else; it need not be cleared
 *
 * Per counting pixel: truth not a class: ignored += 1, its scores are not read.  Otherwise its C scores are read; one of them
 * NaN or +-inf: non-finite += 1, nothing summed.  Otherwise counted += 1 and for every k < K the pixel's NLL, g and h at
 * betas[k] (fp32, formulas above) are added to table[group[n]][k] in fp64.  The scores of a pixel that does not count are
 * not read.  A finite score whose distance to the pixel's maximum overflows fp32 gives what the formulas give.
 *
 * Two launches.  The first has a grid of (gx, N) workgroups; workgroup (x, n) walks trips x, x + gx, .. of image n, a trip
 * being 2048 consecutive pixels, and every wave meets its counting pixels in a fixed order; lane k of the wave keeps the three
 * fp64 sums of betas[k].  The workgroup's four waves are added in order into one partial row of scratch.  The second launch is
 * one workgroup that adds, image by image in ascending n, the image's rows (four interleaved sequences, then those in order)
 * and adds that sum onto the table entry of the image's group (gx = min(trips, 768 / N), at least 1).  The order is fixed by N, H, W and K alone.
 */
int ubf_accumulate(const float* scores, const void* truth, int truth_kind, const float* lit, float lit_threshold,
                   const uint8_t* group, const float* betas, int K, int N, int C, int H, int W, int G,
                   double* table, unsigned long long* counters, void* scratch, int64_t scratch_bytes, void* stream);

/* Rescale n tiles of log-probabilities in one streaming launch:  out[i][c] = beta_i in[i][c] - lse_c(beta_i in[i][c]).
 *
 *   in, out    [n][C][th][tw] float32; out == in (in place) or the two do not overlap
 *   betas      [n] float32: the inverse temperature of tile i, positive and finite (not checked: on the device)
 *
 * Per pixel, with m = max_c in_c:  d_c = in_c - m, z_c = beta d_c, S = sum_c expf(z_c) in class order, out_c = z_c - logf(S);
 * S >= 1 because the maximum's term is 1, so finite inputs give finite outputs or -inf, never NaN.
 *   an input of -inf beside a finite maximum:   out_c = -inf (probability 0), the others as if it were absent
 *   all C inputs -inf:                          all C outputs -inf (the pixel is copied)
 *   any input NaN or +inf:                      all C outputs are the quiet NaN 0x7FC00000
 * The vector path (th * tw a multiple of 4, both pointers 16-byte aligned) moves 16 bytes per access; otherwise one float. */
int ubf_apply(const float* in, float* out, const float* betas, int n, int C, int th, int tw, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubf_last_error(void);
int ubf_version(void);

#ifdef __cplusplus
}
#endif

#endif
