/*
 * ubresnet_sparse.h -- C ABI of libubresnet_sparse.so (sparse event I/O of whole-view inference on the device: a sorted list of
 * (pixel, value) pairs scattered into a dense view, dense event products compacted into the list of their lit pixels, and that
 * list expanded back; gfx950 / MI355X).
 *
 * A small library next to the others of the package.  It links against none of them and shares no state with them: it has its
 * own per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_post.h: device pointers, `stream` is a hipStream_t passed as void*, all arguments are
 * validated on the host before any HIP call, 0 on success or a negative UBZ_E* code with a message in ubz_last_error().  No
 * function allocates, frees or synchronises.  No launch argument depends on device state (`count` is read by the kernels), so
 * the calls capture into a graph as they are.  The three calls only move data: every byte they store is a byte they loaded,
 * or the fill.
 *
 * A pixel index is the int32 linear offset (plane * rows + row) * cols + col into a [P][rows][cols] image; images of
 * 2^31 pixels or more are refused.
 *
 * Entry lists.  ubz_scatter_view and ubz_expand read the first m = min(*count, n) entries of their lists (m = n where count is
 * NULL).  Entry i < m is VALID iff 0 <= index[i] < P * rows * cols and (i == 0 or index[i] > index[i - 1]), where index[i - 1]
 * is the raw predecessor, valid or not.  Invalid entries are not written; their number is ADDED to status[0] (one integer
 * atomic add per workgroup at most, the only atomic of the library: the sum does not depend on the order).  With status[0]
 * unchanged the result is defined on every byte.  Otherwise the elements named by entries are unspecified (two valid entries
 * may name one element), every other element is as defined, and nothing outside the outputs is touched.
 */
#ifndef UBRESNET_SPARSE_H
#define UBRESNET_SPARSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBZ_OK 0
#define UBZ_EINVAL (-1)   /* bad argument */
#define UBZ_ELAUNCH (-2)  /* hip launch error */

/* launch geometry (tests derive their sizes from it; csrc/ubr_sparse_plan.h holds the plan).  Every workgroup has UBZ_LANES
 * lanes.  The count and write passes of ubz_compact give a workgroup UBZ_PIXEL_BLOCK consecutive pixels, UBZ_LANE_PIXELS
 * consecutive ones per lane; the scan is one workgroup that takes UBZ_SCAN_WIDTH block counts per trip.  The fill and scatter
 * launches have at most UBZ_MAX_GRID workgroups, which stride. */
#define UBZ_LANES 256
#define UBZ_LANE_PIXELS 4
#define UBZ_PIXEL_BLOCK 1024
#define UBZ_SCAN_WIDTH 1024
#define UBZ_MAX_GRID 4096
#define UBZ_MAX_VPLANES 64

/* view[e] = +0.0 for every element e of view, then view[index[i]] = value[i], bit for bit (NaN payloads, -0.0 and subnormals
 * kept), for every valid entry i.
 *   index   int32 [n], value fp32 [n]; may be NULL where n == 0; 0 <= n < 2^31
 *   count   uint64 on the device, or NULL
 *   view    fp32 [P][rows][cols]; overlaps no input
 *   status  uint64 on the device, ADDED to
 * Two launches (the fill, the scatter; one where n == 0).  4 bytes per element of view and 12 bytes per entry. */
int ubz_scatter_view(const int32_t* index, const float* value, int64_t n, const unsigned long long* count, float* view, int P,
                     int rows, int cols, unsigned long long* status, void* stream);

/* bytes of scratch ubz_compact needs for a [P][rows][cols] image; 0 (and a message) for an image it refuses */
int64_t ubz_compact_scratch_bytes(int P, int rows, int cols);

/* The lit pixels of event products, in ascending pixel-index order.
 *   label          [P][rows][cols] uint8
 *   confidence     [P][rows][cols] IEEE half bits
 *   adc            [P*vplanes][rows][cols] fp32, or NULL: every pixel is lit; 1 <= vplanes <= UBZ_MAX_VPLANES
 *   capacity       entries of the three outputs, >= 1
 *   out_index      int32 [capacity], out_label uint8 [capacity], out_confidence half bits [capacity]
 *   count          uint64 on the device, STORED
 *   scratch        ubz_compact_scratch_bytes(P, rows, cols) bytes, 16-byte aligned; scratch_bytes is what the caller has
 * The lit test is that of ubresnet_post.h:
 *   lit    <=> adc == NULL, or max over v < vplanes of adc[plane*vplanes + v][oy][ox] > adc_threshold (strict; NaN is not lit)
 * With total the number of lit pixels and q_k the index of the k-th of them in ascending order: count[0] = total, and for
 * k < min(total, capacity): out_index[k] = q_k, out_label[k] = label[q_k], out_confidence[k] = confidence[q_k].  Entries at
 * k >= min(total, capacity) are not written; count[0] > capacity is how the caller sees the overflow.
 * Three launches: a count per pixel block, an exclusive scan of the counts by one workgroup, a write pass that evaluates the
 * same predicate function again.  No atomic, and no workgroup waits for another. */
int ubz_compact(const uint8_t* label, const uint16_t* confidence, const float* adc, int vplanes, float adc_threshold, int P,
                int rows, int cols, int64_t capacity, int32_t* out_index, uint8_t* out_label, uint16_t* out_confidence,
                unsigned long long* count, void* scratch, int64_t scratch_bytes, void* stream);

/* The inverse of ubz_compact: out_label[e] = fill_label and out_confidence[e] = +0 for every element e, then
 * out_label[index[i]] = label[i] and out_confidence[index[i]] = confidence[i] for every valid entry i.
 *   index int32 [n], label uint8 [n], confidence half bits [n]; may be NULL where n == 0; 0 <= n < 2^31
 *   count, status as in ubz_scatter_view; fill_label 0..255
 *   out_label uint8 [P][rows][cols], out_confidence half bits [P][rows][cols]; overlap no input
 * Two launches (one where n == 0). */
int ubz_expand(const int32_t* index, const uint8_t* label, const uint16_t* confidence, int64_t n, const unsigned long long* count,
               int fill_label, uint8_t* out_label, uint16_t* out_confidence, int P, int rows, int cols,
               unsigned long long* status, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubz_last_error(void);
int ubz_version(void);

#ifdef __cplusplus
}
#endif

#endif
