/*
 * ubresnet_match.h -- C ABI of libubresnet_match.so (clusters of different wire planes matched by their time profiles on the
 * device: the charge of every large cluster per time bin, and for every pair of them from two planes the shared bins, the
 * overlap of the two profiles and each side's charge inside the shared bins; gfx950 / MI355X).
 *
 * A small library next to the others of the package.  It links against none of them and shares no state with them: it has its
 * own per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_moment.h and ubresnet_overlap.h: device pointers, `stream` is a hipStream_t passed as void*,
 * all arguments are validated on the host before any HIP call, 0 on success or a negative UBU_E* code with a message in
 * ubu_last_error().  No function allocates, frees or synchronises.  No launch argument depends on device state (the counts are
 * read by the kernels), so the call captures into a graph as it is, together with ubi_label and ubi_tabulate.  No kernel waits
 * for another workgroup: there is no flag, no spinning and no cooperative launch; every loop has a trip count the host computed
 * or a fixed one.  Every operation is an integer operation, so the outputs are the same bytes on every run, stream and graph
 * replay.
 *
 * A pixel index is the int32 linear offset q = (plane * rows + row) * cols + col into a [P][rows][cols] image.  The planes of
 * an event share the time axis, which is the image row.
 *
 * The weight of a pixel is that of ubresnet_moment.h, for its float32 ADC v and a scale that is a power of two in
 * 1..UBU_MAX_SCALE (so that t = v * scale is exact in float32):
 *   NaN, or t < 0               w = 0
 *   t > 65535 (+inf included)   w = 65535
 *   otherwise                   w = rint(t), ties to even; -0.0, +0.0 and whatever rounds to 0 give w = 0
 * Only the ADC of a pixel of a candidate is read at all.
 */
#ifndef UBRESNET_MATCH_H
#define UBRESNET_MATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBU_OK 0
#define UBU_EINVAL (-1)   /* bad argument */
#define UBU_ELAUNCH (-2)  /* hip launch error */

/* launch geometry and limits (csrc/ubr_match_plan.h holds the plan and derives the bounds).  The profile launch walks the pixels
 * as ubm_moments does: a workgroup of UBU_LANES lanes takes UBU_TRIP_PIXELS consecutive pixels per trip, at most UBU_MAX_GRID
 * workgroups.  The match launch gives a workgroup a UBU_TILE x UBU_TILE tile of pairs and walks the bins UBU_CHUNK_BINS at a
 * time. */
#define UBU_LANES 256
#define UBU_TRIP_PIXELS 2048
#define UBU_MAX_GRID 1024
#define UBU_TILE 64
#define UBU_CHUNK_BINS 64
#define UBU_MIN_PLANES 2
#define UBU_MAX_PLANES 4
#define UBU_MIN_SLOTS 64
#define UBU_MAX_SLOTS 4096
#define UBU_MAX_TIME_BIN 64
#define UBU_MAX_SHIFT 4096
#define UBU_MAX_ROWS 4096
#define UBU_MAX_COLS 4096
#define UBU_MAX_PLANE_PIXELS 4194304 /* rows * cols of one plane: 2^22 */
#define UBU_MAX_BIN_PIXELS 65536     /* time_bin * cols: a bin holds at most time_bin * cols * 65535 < 2^32 */
#define UBU_MAX_CLASSES 16
#define UBU_CLUSTER_FIXED 8 /* UBI_TABLE_FIXED: columns of a cluster table row before the class counts */
#define UBU_CAND_COLUMNS 6
#define UBU_PAIR_COLUMNS 4
#define UBU_MAX_WEIGHT 65535
#define UBU_MAX_SCALE 256

/* bytes of scratch for an image, a time bin, a number of slots and the capacity of the cluster table; 0 for arguments ubu_match
 * refuses */
int64_t ubu_scratch_bytes(int P, int rows, int cols, int time_bin, int64_t slots, int64_t capacity);

/* The time profiles of the large clusters of an event and the pair table of those from different planes.
 *   ids            int32 [P][rows][cols], 16-byte aligned: the map ubi_tabulate wrote -- the cluster number k >= 0 of a lit
 *                  pixel, -1 for every other
 *   clusters       int64 [capacity][cluster_width], 8-byte aligned: the table ubi_tabulate wrote; cluster_width is
 *                  UBU_CLUSTER_FIXED + C for its 1..UBU_MAX_CLASSES classes.  Column 0 (root) and column 1 (pixels) are read.
 *   count          uint64 on the device, 8-byte aligned: the count ubi_tabulate stored; read by the kernels.  capacity >= 1
 *   view           float32 [P][rows][cols] (a [P][1][rows][cols] view is the same bytes), 16-byte aligned: the ADC
 *   adc_scale      a power of two in 1..UBU_MAX_SCALE
 *   P              UBU_MIN_PLANES..UBU_MAX_PLANES; rows, cols 1..4096 with rows * cols <= UBU_MAX_PLANE_PIXELS
 *   min_pixels     >= 1: a cluster k < min(*count, capacity) whose pixels column is >= min_pixels is a candidate
 *   time_bin       a power of two in 1..UBU_MAX_TIME_BIN with time_bin * cols <= UBU_MAX_BIN_PIXELS.  T = ceil(rows / time_bin)
 *                  is the number of time bins.
 *   row_shift      int [P] on the HOST, each in -UBU_MAX_SHIFT..UBU_MAX_SHIFT: the time offset of every plane.  The time bin
 *                  of a pixel is t = (row + row_shift[plane]) >> log2(time_bin); a pixel of a candidate whose shifted row is
 *                  outside [0, rows) is dropped and counted in status[1].
 *   slots          S: the candidate capacity, a multiple of UBU_TILE in UBU_MIN_SLOTS..UBU_MAX_SLOTS
 *   profile        uint32 [S][T], 4-byte aligned, STORED whole: profile[c][t] is the summed weight of candidate c in time bin t;
 *                  rows at or past the number of candidates are zero
 *   candidates     int64 [S][UBU_CAND_COLUMNS], 8-byte aligned, STORED whole: row c < min(ncand, S) is
 *                    {cluster, plane, Q, bins, t_min, t_max}
 *                  the cluster number, plane = root / (rows * cols), Q the sum of the profile, bins the number of occupied bins
 *                  -- bins in which the candidate holds a pixel, whatever its weight -- and t_min, t_max the first and last of
 *                  them (T and -1 for a candidate without one).  Candidates are numbered in ascending cluster number, so those
 *                  of one plane are contiguous.  Rows at or past min(ncand, S) are zero.
 *   pairs          int64 [S][S][UBU_PAIR_COLUMNS], 8-byte aligned.  Entry (i, j) with i < j < min(ncand, S) is STORED:
 *                    {both, I, Qi_in, Qj_in}
 *                  both the number of bins both candidates occupy, I the sum over t of min(profile_i[t], profile_j[t]), Qi_in
 *                  and Qj_in the charge of i and of j inside the bins both occupy.  A pair from one plane is four zeros.
 *                  Entries with i >= j, or with j at or past min(ncand, S), are not touched.
 *   ncand          uint64 on the device, 8-byte aligned, STORED: the number of candidates, also where it exceeds S
 *   status         uint64 [2] on the device, 8-byte aligned, ADDED to: [0] the candidates past S, which are left out; [1] the
 *                  pixels of candidates dropped by row_shift
 *   scratch        ubu_scratch_bytes(...) bytes, 16-byte aligned
 * Five launches.  (1) Clear: profile, the pixel counts in scratch and the candidate table.  (2) Select, one workgroup: a scan of
 * the clusters that pass min_pixels numbers the candidates and writes slot_of (int32 per cluster below min(*count, capacity), -1
 * for none) into scratch, the cluster and plane columns, ncand and status[0].  (3) Profile: a lane loads the ids of four consecutive pixels in one 16-byte
 * load and the view only if one of the four belongs to a candidate; the lanes of a wave that share (candidate, t) are combined,
 * and the first of them makes one 32-bit integer atomic add of the weight and one of the pixel count.  (4) Summarise: a wave per
 * candidate sums its profile, ballots the occupancy word of every chunk of UBU_CHUNK_BINS bins into scratch and writes Q, bins,
 * t_min and t_max.  (5) Match: the upper triangle of (S / UBU_TILE)^2 tiles, a workgroup of UBU_LANES lanes per tile and a
 * 4 x 4 block of pairs per lane.  A tile past ncand returns after one read of ncand.  A tile whose candidates all lie in one
 * plane, or whose two [t_min, t_max] hulls do not meet, stores its zeros without loading a profile.  Every other tile walks the
 * chunks inside both hulls, stages both strips of profiles in LDS, accumulates in 64 bits and writes each pair once; there are no
 * atomics. */
int ubu_match(const int32_t* ids, const long long* clusters, int cluster_width, const unsigned long long* count, int64_t capacity,
              const float* view, float adc_scale, int P, int rows, int cols, int64_t min_pixels, int time_bin, const int* row_shift,
              int64_t slots, uint32_t* profile, long long* candidates, long long* pairs, unsigned long long* ncand,
              unsigned long long* status, void* scratch, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubu_last_error(void);
int ubu_version(void);

#ifdef __cplusplus
}
#endif

#endif
