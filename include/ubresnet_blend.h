/*
 * ubresnet_blend.h -- C ABI of libubresnet_blend.so (blended stitching of overlapping tiles in whole-view inference on the
 * device: every tile of a call is added, with a weight per tile row and per tile column, into a view-sized buffer of
 * log-probabilities, which ends as the log of the weighted mean of the covering tiles' probabilities; gfx950 / MI355X).
 *
 * A small library next to the others of the package.  It links against none of them and shares no state with them: it has its
 * own per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_tta.h: device pointers, `stream` is a hipStream_t passed as void*, all arguments are
 * validated on the host before any launch, 0 on success or a negative UBV_E* code with a message in ubv_last_error().  No
 * function allocates, frees or synchronises.  The tile descriptors are read on the host, during the call, and travel as launch
 * arguments; no launch argument depends on device state, so the calls capture into a graph, or sit between the replays of one,
 * as they are.
 *
 * Arithmetic.  ubv_blend_begin stores the bit pattern of -inf.  ubv_blend_tiles combines the running value a of a view pixel
 * with a tile's log-probability x and the logs of its row and column weight, lwr and lwc, as
 *     a <- lae(a, fl(x + fl(lwr + lwc)))
 * where lae is exactly the rule of ubresnet_tta.h:
 *     lae(a, b):  NaN if either is NaN;  hi = max(a, b), lo = min(a, b);  lo == -inf -> hi;  hi == lo -> hi + (float)M_LN2;
 *                 otherwise hi + log1pf(expf(lo - hi)),
 * every step one fp32 operation rounded to nearest even or one library call, none contracted with another, subnormals kept.
 * Nothing is exponentiated on its own: the result is finite wherever the operands are.  (+inf, x) gives +inf.  Which NaN comes
 * out (its payload) is not part of the contract.  Consequences: a weight of -inf (lwr or lwc) leaves a untouched unless x is
 * +inf or NaN; the first tile to reach a pixel after ubv_blend_begin stores fl(x + fl(lwr + lwc)), which for weights +0 is x's
 * bit pattern (only -0.0 becomes +0.0).
 *
 * Order.  The kernel is gather-form over view pixels: the lane of the first tile of the call (in descriptor order) that covers
 * a pixel reads the pixel once, applies every covering tile of the call in ascending descriptor order and stores it once.
 * Tiles of one call may therefore overlap, tiles of different calls meet through `out` in the order of the calls, there is no
 * atomic and the result is reproducible bit for bit.
 */
#ifndef UBRESNET_BLEND_H
#define UBRESNET_BLEND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBV_OK 0
#define UBV_EINVAL (-1)   /* bad argument */
#define UBV_ELAUNCH (-2)  /* hip launch error */

#define UBV_MAX_TILES 64
#define UBV_MAX_CLASSES 16

/* launch geometry of both calls (tests derive their sizes from it).  A unit is 4 consecutive floats of a row on the vector
 * path, one float on the scalar path.  ubv_blend_begin: units of `out`; vector where nelem % 4 == 0 and out is 16-byte aligned.
 * ubv_blend_tiles: units of the tiles, n * th * (tw / 4 or tw) of them, every class of a unit's pixels handled by its lane;
 * vector where tw % 4 == 0, cols % 4 == 0, every col0 % 4 == 0 and logp, lw_cols and out are 16-byte aligned (a unit is then
 * whole inside or whole outside every tile and the view, and every 16-byte access is aligned), scalar otherwise; the choice is
 * uniform over the launch.  A workgroup has UBV_BLOCK lanes, a trip is UBV_BLOCK consecutive units, the grid is
 * min(ceil(units / UBV_BLOCK), UBV_MAX_GRID) workgroups and workgroup g takes the trips g, g + grid, ... */
#define UBV_BLOCK 256
#define UBV_MAX_GRID 2048

/* out[i] = -inf for i < nelem.  out: device memory, 4-byte aligned; 0 < nelem <= 2^40.  4 bytes of traffic per element. */
int ubv_blend_begin(float* out, int64_t nelem, void* stream);

/* The n tiles of logp into the view-sized buffer out.
 *   logp       [n][C][th][tw] fp32 log-probabilities, 1 <= C <= UBV_MAX_CLASSES, th, tw > 0, th * tw <= 2^24
 *   desc_host  n x 3 int32 {plane, row0, col0} in HOST memory, read during the call; 1 <= n <= UBV_MAX_TILES,
 *              0 <= plane < P and the origin inside the view: 0 <= row0 < rows, 0 <= col0 < cols
 *   lw_rows    [n][th], lw_cols [n][tw] fp32: the log of tile t's weight at tile row y is lw_rows[t][y], at tile column x
 *              lw_cols[t][x]; the log of its weight at (y, x) is their fp32 sum.  -inf is a weight of zero.
 *   out        [P][C][rows][cols] fp32, P >= 1, rows, cols > 0, P * C * rows * cols <= 2^40; overlaps no input
 * Tile t covers the view pixels (plane, row0 + y, col0 + x), y < th, x < tw, that lie inside the view; the parts of a tile
 * outside the view are skipped.  For every view pixel covered by at least one tile of the call and every class c, with the
 * covering tiles t in ascending order:
 *     out[plane][c][r][q] <- lae(out[plane][c][r][q], fl(logp[t][c][r - row0][q - col0] + fl(lw_rows[t][r - row0] + lw_cols[t][q - col0])))
 * Pixels that no tile of the call covers are not written.  Only out is written.  Per covered pixel and class: 8 bytes of out
 * and 4 bytes of logp per covering tile. */
int ubv_blend_tiles(const float* logp, int C, int th, int tw, const int32_t* desc_host, int n, const float* lw_rows,
                    const float* lw_cols, float* out, int P, int rows, int cols, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubv_last_error(void);
int ubv_version(void);

#ifdef __cplusplus
}
#endif

#endif
