/*
 * ubresnet_score.h -- C ABI of libubresnet_score.so (scoring event products against a truth image, gfx950 / MI355X).
 *
 * A small library next to libubresnet_hip.so (include/ubresnet_hip.h) and libubresnet_post.so (include/ubresnet_post.h), whose
 * products it reads.  It links against neither and shares no state with them: it has its own per-thread error string and its
 * launch is a plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_post.h: device pointers unless stated, `stream` is a hipStream_t passed as void*,
 * arguments are validated on the host, 0 on success or a negative UBQ_E* code with a message in ubq_last_error().
 * No function allocates, frees or synchronises.  Everything is integer arithmetic: the table is reproducible bit for bit.
 */
#ifndef UBRESNET_SCORE_H
#define UBRESNET_SCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBQ_OK 0
#define UBQ_EINVAL (-1)   /* bad argument */
#define UBQ_ELAUNCH (-2)  /* hip launch error */

#define UBQ_MAX_CLASSES 16
#define UBQ_MAX_BINS 32
#define UBQ_MAX_RADIUS 8
#define UBQ_TRUTH_U8 0    /* truth is uint8_t */
#define UBQ_TRUTH_I64 1   /* truth is int64_t */

#define UBQ_TILE_H 32     /* a workgroup scores a UBQ_TILE_H x UBQ_TILE_W tile of one plane */
#define UBQ_TILE_W 128

/* uint64 words of one table: P * (2*C*C + 2*bins*3 + 4), or UBQ_EINVAL (P < 1, C outside 1..UBQ_MAX_CLASSES, bins outside
 * 1..UBQ_MAX_BINS, or a count that does not fit an int). */
int ubq_table_words(int P, int C, int bins);

/* Score one event's products against its truth image; every count is ADDED to `table`.
 *
 *   label           [P][rows][cols] uint8, as ubp_stitch_products writes it; label == fill_label: the pixel is not lit
 *   confidence      [P][rows][cols] IEEE half bits
 *   truth           [P][rows][cols] uint8_t (truth_kind UBQ_TRUTH_U8) or int64_t (UBQ_TRUTH_I64)
 *   C               1..UBQ_MAX_CLASSES; valid(t) <=> 0 <= t < C on the full width of the truth type (an int64 is compared on 64
 *                   bits before it is narrowed)
 *   fill_label      0..255
 *   radius          0..UBQ_MAX_RADIUS; interface_from 0..C
 *   edges_host      HOST pointer to bins - 1 strictly ascending bit patterns of positive finite halves (0x0001..0x7BFF);
 *                   1 <= bins <= UBQ_MAX_BINS; bins == 1: no edges, edges_host may be NULL
 *   table           ubq_table_words(P, C, bins) uint64, 8-byte aligned, per plane p in this order:
 *                     conf[p][s][t][l]  2*C*C words   s: 0 clear, 1 interface; t the truth, l the label
 *                     rel[p][s][b][3]   2*bins*3      {pixels, correct pixels, sum of confidence in units of 2^-24}
 *                     tally[p][4]       4             {scored, ignored, dark signal, non-finite confidence}
 *   P >= 1 (at most 65535), rows, cols >= 1; P * rows * cols may exceed 2^31
 *
 * Per pixel (p, y, x):
 *   not lit:  if valid(truth) and truth >= 1: tally.dark += 1 (signal the threshold hid from the network's score); nothing else
 *   lit and (!valid(truth) or label >= C):  tally.ignored += 1; nothing else
 *   otherwise: tally.scored += 1, conf[p][s][truth][label] += 1, where s = 1 needs all three of: radius > 0;
 *             truth >= interface_from; some pixel of the (2 radius + 1)^2 window around it, clipped at the view's edges, lit or
 *             not, has a valid truth t' >= interface_from with t' != truth (the contact rule of ubw_pixel_weights,
 *             include/ubresnet_weight.h, on the truth image of the whole view); s = 0 otherwise.
 *             Confidence bits h: the sign bit with any non-zero magnitude, or an exponent of all ones (inf, NaN):
 *             tally.nonfinite += 1 and the pixel is not binned.  0x8000 counts as zero.  Otherwise b = the number of edges <= h,
 *             compared as integers (monotone for non-negative halves), and rel[p][s][b] += {1, label == truth, fix(h)} with
 *             fix(h) = the half's value times 2^24 as an integer: a subnormal is its mantissa m, a normal is
 *             (1024 + m) << (e - 1).
 * Sums wrap modulo 2^64; this cannot happen below 2^23 pixels of confidence <= 1 (fix(h) <= 2^24 there; nor below 2^23 pixels
 * of any finite half, fix(h) < 2^41).  Integer adds commute: the table does not depend on scheduling. */
int ubq_score_event(const uint8_t* label, const uint16_t* confidence, const void* truth, int truth_kind,
                    int C, int fill_label, int radius, int interface_from,
                    const uint16_t* edges_host, int bins,
                    unsigned long long* table, int P, int rows, int cols, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubq_last_error(void);
int ubq_version(void);

#ifdef __cplusplus
}
#endif

#endif
