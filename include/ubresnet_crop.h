/*
 * ubresnet_crop.h -- C ABI of libubresnet_crop.so (training crops cut from a whole labelled view on the device: an occupancy
 * table of the view's counting pixels, seeded crop positions drawn against it, and the gather of image, label and weight into
 * the training batch; gfx950 / MI355X).
 *
 * A small library next to the others of the package.  It links against none of them and shares no state with them: it has its
 * own per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_sparse.h: device pointers unless stated, `stream` is a hipStream_t passed as void*, all
 * arguments are validated on the host before any HIP call, 0 on success or a negative UBN_E* code with a message in
 * ubn_last_error().  No function allocates, frees or synchronises.  No launch argument depends on device state (the table is
 * read by the kernels), so the calls capture into a graph as they are.  No workgroup waits for another, and the only atomic
 * is one integer atomic add on the status word of ubn_gather.  Pointers need natural alignment only; a region that is 16-byte
 * aligned is read and written with 16-byte accesses, any other with element accesses.
 *
 * Geometry.  A view is P planes of rows x cols pixels, P * rows * cols < 2^31; a crop is H x W.  The sampler works on cells of
 * `cell` x `cell` pixels: cell is a power of two, UBN_MIN_CELL <= cell <= UBN_MAX_CELL, and divides H, W, rows - H and
 * cols - W (a zero difference divides), hence rows and cols as well.  With g = cell:
 *   CR = rows / g, CC = cols / g                      cells of the view
 *   NR = (rows - H) / g + 1, NC = (cols - W) / g + 1  crop positions
 * Crop positions are multiples of g, so the number of counting pixels of any crop is four reads of the table.
 *
 * Counting pixels.  Per-plane mode (stacked == 0): pixel (p, r, c) COUNTS iff
 *   lit    <=> image[p][r][c] > adc_threshold (strict; NaN is not lit)
 * and, where a label is given, its converted label L is in 0..31 with bit L of class_mask set.  Stacked mode (stacked != 0:
 * the P planes are the channels of one image and there is one label image [rows][cols]): one count plane; pixel (r, c) counts
 * iff any of its P values is lit and, where a label is given, its label passes the mask.
 *
 * Labels are uint8, int64 or fp32 (UBN_LABEL_*).  The converted label of a value v with label_offset:
 *   uint8, int64      v + label_offset                          (64-bit two's complement)
 *   fp32, |v| < 2^31  (int64) trunc(v) + label_offset           (toward zero: -0.0 and subnormals give label_offset)
 *   fp32 otherwise    INT64_MIN                                 (NaN and the infinities included)
 * which for fp32 is the rule of ubd_prep_batch (ubresnet_data.h).
 */
#ifndef UBRESNET_CROP_H
#define UBRESNET_CROP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBN_OK 0
#define UBN_EINVAL (-1)   /* bad argument */
#define UBN_ELAUNCH (-2)  /* hip launch error */

#define UBN_LANES 256          /* lanes of every workgroup */
#define UBN_MIN_CELL 4
#define UBN_MAX_CELL 64
#define UBN_MAX_CELL_COLS 4096 /* cols / cell at most: one workgroup scans a row of cells in its LDS */
#define UBN_MAX_PLANES 64      /* P at most */
#define UBN_MAX_CROPS 4096     /* K at most */
#define UBN_MAX_TRIES 64       /* T at most */
#define UBN_TABLE_FIELDS 8     /* int32 per table row: plane, row0, col0, lit, try, accepted, flip_rows, flip_cols */
#define UBN_PHILOX_TAG 0x43524F50u /* "CROP": the fourth counter word of every draw */

#define UBN_LABEL_NONE 0
#define UBN_LABEL_U8 1
#define UBN_LABEL_I64 2
#define UBN_LABEL_F32 3

/* The summed-area table of the counting pixels: sat[q][i][j] = number of counting pixels of count plane q with row < i * cell
 * and col < j * cell, int32 [Q][CR + 1][CC + 1], Q = P (per-plane) or 1 (stacked).  Every element is written, the zero row and
 * column included.
 *   image        fp32 [P][rows][cols]
 *   label        [P][rows][cols] (stacked: [rows][cols]) of label_kind, or NULL with UBN_LABEL_NONE: no class mask
 *   class_mask   bit L set: label L counts; read only where a label is given
 *   cell         divides rows and cols; cols / cell <= UBN_MAX_CELL_COLS
 *   sat          overlaps no input
 * Two launches: one workgroup per count plane and cell row counts its cells (a wave per cell, wave ballots) and scans them
 * along the row; one thread per count plane and cell column then walks down the rows.  No atomic.
 * Bytes: 4 per pixel of image, plus the label's 1 / 8 / 4 per pixel where a mask is on. */
int ubn_occupancy(const float* image, const void* label, int label_kind, int32_t label_offset, uint32_t class_mask, int stacked,
                  float adc_threshold, int P, int rows, int cols, int cell, int32_t* sat, void* stream);

/* K crop positions, one launch, one thread per crop.  For crop k < K and try t = 0 .. T - 1:
 *   w = Philox4x32-10(key = (seed_lo, seed_hi), counter = (number, k, t, UBN_PHILOX_TAG))
 *   plane = planes[w0 % nplanes]   (stacked, Q == 1: plane 0)
 *   i = w1 % NR, j = w2 % NC
 *   n = sat[plane][i + H/g][j + W/g] - sat[plane][i][j + W/g] - sat[plane][i + H/g][j] + sat[plane][i][j]
 * The first try with n >= min_lit is taken (accepted = 1); if there is none, the try with the largest n, the earliest on
 * ties (accepted = 0).  flip_rows = bit 0 and flip_cols = bit 1 of the taken try's w3, each AND-ed with its enable.
 * Row k of table: plane, row0 = i * g, col0 = j * g, lit = n, try, accepted, flip_rows, flip_cols.
 * The modulo is part of the rule: a value v of w % N is drawn with probability floor or ceil of 2^32 / N over 2^32, a relative
 * bias below N / 2^32.  Two crops may be the same; min_lit = 0 takes try 0 of every crop, which is uniform sampling.
 *   sat          int32 [Q][CR + 1][CC + 1] as ubn_occupancy wrote it
 *   planes       HOST array of nplanes distinct planes in 0..Q-1, the planes a crop may come from; NULL: all Q in order
 *   K            1..UBN_MAX_CROPS;  T 1..UBN_MAX_TRIES;  min_lit >= 0
 *   number       the event's number: the result is a pure function of (seed, number) and the table
 *   table        int32 [K][UBN_TABLE_FIELDS], written */
int ubn_choose(const int32_t* sat, int Q, int rows, int cols, int H, int W, int cell, const int32_t* planes, int nplanes, int K,
               int T, int32_t min_lit, uint32_t seed_lo, uint32_t seed_hi, uint32_t number, int flip_rows, int flip_cols,
               int32_t* table, void* stream);

/* The crops of `table` out of the view, one launch.  With (plane, row0, col0, fr, fc) of row k and, for output pixel (y, x),
 * the source pixel (sr, sc) = (row0 + (fr ? H-1-y : y), col0 + (fc ? W-1-x : x)):
 *   out_image    fp32 [K][1][H][W] = image[plane][sr][sc]; stacked: [K][P][H][W] = image[p][sr][sc].  Bit copies.
 *   out_label    int64 [K][H][W], the converted label of label[plane][sr][sc] (stacked: label[sr][sc])
 *   out_weight   fp32 [K][H][W], bit copies of weight[plane][sr][sc] (stacked: weight[sr][sc]); 1.0f where weight is NULL
 * table is read from the device, so a caller may supply rows of its own, at any in-range offsets.  Only the fields plane,
 * row0, col0, flip_rows and flip_cols are read.  A row is INVALID if plane is outside 0..P-1 (stacked: not 0), row0 outside
 * 0..rows-H, col0 outside 0..cols-W, or a flip field is not 0 or 1: nothing is read through it, its crop is +0.0f, label 0
 * and weight +0.0f, and one is ADDED to status[0].  W must be a multiple of 4.  No byte outside the three outputs and the
 * status word is written.
 *   label        of label_kind, not NULL (UBN_LABEL_NONE is refused)
 *   status       uint64 on the device, ADDED to
 * Bytes per output pixel: 4 + 4 read and 4 + 8 + 4 written with an fp32 label and a weight view. */
int ubn_gather(const float* image, const void* label, int label_kind, int32_t label_offset, const float* weight, int stacked, int P,
               int rows, int cols, int H, int W, const int32_t* table, int K, float* out_image, int64_t* out_label,
               float* out_weight, unsigned long long* status, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubn_last_error(void);
int ubn_version(void);

#ifdef __cplusplus
}
#endif

#endif
