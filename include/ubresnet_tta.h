/*
 * ubresnet_tta.h -- C ABI of libubresnet_tta.so (flip test-time augmentation of tiled and pre-cropped inference on the device:
 * a batch of input planes is written flipped, the network runs on it as on any batch, and its log-probabilities are read back
 * un-flipped into a running merge that ends as the log of the arithmetic mean of the views' probabilities; gfx950 / MI355X).
 *
 * A thirteenth, small library next to libubresnet_hip.so, libubresnet_post.so, libubresnet_data.so, libubresnet_aug.so,
 * libubresnet_opt.so, libubresnet_weight.so, libubresnet_group.so, libubresnet_ema.so, libubresnet_accum.so,
 * libubresnet_stats.so, libubresnet_loss.so and libubresnet_dice.so.  It links against none of them and shares no state with
 * them: it has its own per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_accum.h: device pointers, `stream` is a hipStream_t passed as void*, arguments are validated
 * on the host before any launch, 0 on success or a negative UBT_E* code with a message in ubt_last_error().  No function
 * allocates, frees or synchronises.  Which view a call belongs to (k of K) is known to the host, so no launch argument depends on
 * device state and the calls capture into a graph, or sit between the replays of one, as they are.
 *
 * `flip` is a bit mask: bit 0 (UBT_FLIP_ROWS) reverses the rows, y -> H - 1 - y; bit 1 (UBT_FLIP_COLS) reverses the columns,
 * x -> W - 1 - x.  A flip is its own inverse, so the same mask writes a flipped input and reads the output back un-flipped.
 *
 * Arithmetic.  ubt_flip_planes and the first view of a merge (k == 0) look at no value: they move 32-bit patterns, so NaN
 * payloads, -0.0 and subnormals arrive as they were.  The later views combine two log-probabilities a and b with
 *     lae(a, b):  NaN if either is NaN;  hi = max(a, b), lo = min(a, b);  lo == -inf -> hi;  hi == lo -> hi + (float)M_LN2;
 *                 otherwise hi + log1pf(expf(lo - hi)),
 * every step one fp32 operation rounded to nearest even or one library call, none contracted with another, subnormals kept.
 * lae is symmetric in (a, b) by construction, and nothing is exponentiated on its own: the result is finite wherever both
 * operands are.  (+inf, x) gives +inf.  Which NaN comes out (its payload) is not part of the contract.
 */
#ifndef UBRESNET_TTA_H
#define UBRESNET_TTA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBT_OK 0
#define UBT_EINVAL (-1)   /* bad argument */
#define UBT_ELAUNCH (-2)  /* hip launch error */

#define UBT_FLIP_ROWS 1
#define UBT_FLIP_COLS 2
#define UBT_MAX_VIEWS 4

/* launch geometry of both calls (tests derive their sizes from it).  A unit is 4 consecutive floats of a row where W % 4 == 0
 * and every pointer is 16-byte aligned (the vector path), one float otherwise (the scalar path).  A workgroup has UBT_BLOCK lanes
 * and a lane takes UBT_UNROLL units per trip, so a trip is UBT_BLOCK * UBT_UNROLL CONSECUTIVE units of the destination; the grid
 * is min(ceil(units / (UBT_BLOCK * UBT_UNROLL)), UBT_MAX_GRID) workgroups and workgroup g takes the trips g, g + grid, ...
 * The flipped side is the load: on the vector path a column flip mirrors the unit index within the row and reverses the four
 * lanes of the unit; every store is linear. */
#define UBT_BLOCK 256
#define UBT_UNROLL 2
#define UBT_MAX_GRID 1024

/* dst[p][y][x] = src[p][fy(y)][fx(x)] for p < nplanes, fy / fx the reversals `flip` selects; fp32 moved as 32-bit patterns.
 * src, dst: [nplanes][H][W] in device memory, not overlapping; nplanes, H, W > 0; 0 <= flip <= 3 (0 is a plain copy).
 * Only dst is written.  8 bytes of traffic per element. */
int ubt_flip_planes(const float* src, float* dst, int64_t nplanes, int H, int W, int flip, void* stream);

/* One view's log-probabilities into the running merge.  logp, acc: [nplanes][H][W] fp32 (nplanes = tiles * classes), not
 * overlapping.  Per element, with u = logp read at the flipped position:
 *     k == 0             : v = u                     (bit pattern moved; 8 bytes per element)
 *     0 < k < K          : v = lae(acc, u)           (12 bytes per element)
 *     k == K - 1, K > 1  : v = v - log_k             (log_k = (float)log((double)K), given by the caller; finite)
 *     acc <- v
 * After the call with k == K - 1 acc holds the log of the arithmetic mean of the K views' probabilities; K == 1 stores the one
 * view untouched.  The views are merged in the order of the calls, so the result is reproducible bit for bit.
 * 1 <= K <= UBT_MAX_VIEWS, 0 <= k < K, 0 <= flip <= 3.  Only acc is written. */
int ubt_merge_view(const float* logp, float* acc, int64_t nplanes, int H, int W, int flip, int k, int K, float log_k, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubt_last_error(void);
int ubt_version(void);

#ifdef __cplusplus
}
#endif

#endif
