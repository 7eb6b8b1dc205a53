/*
 * ubresnet_moment.h -- C ABI of libubresnet_moment.so (per-cluster charge and shape on the device: the ADC of every cluster of an
 * event summed into an integer table of charge, charge per class and first and second moments; gfx950 / MI355X).
 *
 * A small library next to the others of the package.  It links against none of them and shares no state with them: it has its
 * own per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_cluster.h: device pointers, `stream` is a hipStream_t passed as void*, all arguments are
 * validated on the host before any HIP call, 0 on success or a negative UBM_E* code with a message in ubm_last_error().  No
 * function allocates, frees or synchronises.  No launch argument depends on device state (the count is read by the kernels),
 * so the call captures into a graph as it is.  No kernel waits for another workgroup: there is no flag, no spinning and no
 * cooperative launch; every loop has a trip count the host computed or a fixed number of probes.
 *
 * A pixel index is the int32 linear offset q = (plane * rows + row) * cols + col into a [P][rows][cols] image.
 *
 * The weight of a pixel, for its float32 ADC v and a scale that is a power of two in 1..UBM_MAX_SCALE (so that t = v * scale is
 * exact in float32):
 *   NaN, or t < 0               w = 0, and the pixel counts into `odd`
 *   t > 65535 (+inf included)   w = 65535, and the pixel counts into `clipped`
 *   otherwise                   w = rint(t), ties to even; -0.0, +0.0 and whatever rounds to 0 give w = 0 and count into neither
 * Only the ADC of a pixel with ids[q] >= 0 is read at all.
 */
#ifndef UBRESNET_MOMENT_H
#define UBRESNET_MOMENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBM_OK 0
#define UBM_EINVAL (-1)   /* bad argument */
#define UBM_ELAUNCH (-2)  /* hip launch error */

/* launch geometry and limits (csrc/ubr_moment_plan.h holds the plan and derives the overflow bound).  A workgroup of UBM_LANES
 * lanes takes UBM_TRIP_PIXELS consecutive pixels per trip and a contiguous span of trips; there are at most UBM_MAX_GRID
 * workgroups.  The waves of a workgroup combine in an LDS table of UBM_SLOTS clusters. */
#define UBM_LANES 256
#define UBM_TRIP_PIXELS 2048
#define UBM_MAX_GRID 1024
#define UBM_SLOTS 64
#define UBM_MAX_CLASSES 16
#define UBM_TABLE_FIXED 9 /* columns of a table row before the class charges */
#define UBM_MAX_ROWS 4096
#define UBM_MAX_COLS 4096
#define UBM_MAX_PLANE_PIXELS 4194304 /* rows * cols of one plane: 2^22 */
#define UBM_MAX_WEIGHT 65535
#define UBM_MAX_SCALE 256

/* The charge and shape table of the clusters of an event.
 *   ids            int32 [P][rows][cols], 16-byte aligned: the map ubi_tabulate wrote -- the cluster number k >= 0 of a lit
 *                  pixel, -1 for every other
 *   label          uint8 [P][rows][cols], 4-byte aligned: the class map that was clustered
 *   view           float32 [P][rows][cols] (a [P][1][rows][cols] view is the same bytes), 16-byte aligned: the ADC
 *   C              1..UBM_MAX_CLASSES; adc_scale a power of two in 1..UBM_MAX_SCALE
 *   table          int64 [capacity][UBM_TABLE_FIXED + C], 8-byte aligned; capacity >= 1.  Row k < min(*count, capacity) is STORED
 *                  (cleared, then summed), so each call overwrites it:
 *                    {weighted, clipped, odd, Q, Qr, Qc, Qrr, Qrc, Qcc, Q_0 .. Q_{C-1}}
 *                  with w the weight and r, c the row and column of a pixel in its plane: weighted the number of pixels of
 *                  w > 0, Q the sum of w, Qr of w r, Qc of w c, Qrr of w r^2, Qrc of w r c, Qcc of w c^2, and Q_j the sum of w
 *                  over the pixels of label j.  A pixel of ids >= 0 whose label is >= C adds 1 to odd and nothing else.
 *                  Rows at or past min(*count, capacity) are not touched; pixels whose ids are at or past it are skipped.
 *   count          uint64 on the device, 8-byte aligned: the count ubi_tabulate stored; read by the kernels
 *   rows, cols     1..UBM_MAX_ROWS / 1..UBM_MAX_COLS with rows * cols <= UBM_MAX_PLANE_PIXELS, and P * rows * cols < 2^31: a
 *                  cluster lies in one plane, so with w < 2^16 and r^2, r c, c^2 < 2^24 every column stays below 2^62
 * Two launches: a clear of the rows below min(*count, capacity), and the accumulation.  There a lane loads the ids of four
 * consecutive pixels in one 16-byte load and the view and label of the group only if one of the four is lit; the lanes of a wave
 * that share a cluster are combined first; the waves of the workgroup then add into an LDS table keyed by the cluster number, and
 * its occupied slots go to the table in memory with 64-bit integer atomic adds when the table fills and when the workgroup ends.
 * A cluster that finds no slot goes to memory directly.  Zero columns are not sent.  Every operation is an integer add: the
 * table is the same bits for every schedule, slot assignment and grid size. */
int ubm_moments(const int32_t* ids, const uint8_t* label, const float* view, int C, float adc_scale, long long* table,
                int64_t capacity, const unsigned long long* count, int P, int rows, int cols, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubm_last_error(void);
int ubm_version(void);

#ifdef __cplusplus
}
#endif

#endif
