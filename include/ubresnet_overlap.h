/*
 * ubresnet_overlap.h -- C ABI of libubresnet_overlap.so (two clusterings of an event matched on the device: the contingency table
 * of two id maps over the same pixels, one row per pair of cluster numbers with its pixel count and charge; gfx950 / MI355X).
 *
 * A small library next to the others of the package.  It links against none of them and shares no state with them: it has its
 * own per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_moment.h: device pointers, `stream` is a hipStream_t passed as void*, all arguments are
 * validated on the host before any HIP call, 0 on success or a negative UBH_E* code with a message in ubh_last_error().  No
 * function allocates, frees or synchronises.  No launch argument depends on device state, so the call captures into a graph as
 * it is.  No kernel waits for another workgroup: there is no flag, no spinning and no cooperative launch; every loop has a trip
 * count the host computed or a fixed number of probes.
 *
 * A pixel index is the int32 linear offset q = (plane * rows + row) * cols + col into a [P][rows][cols] image.
 *
 * The rule.  ids_a and ids_b are two int32 maps over the same pixels.  A value >= 0 is a cluster number and any negative value
 * means "none".  A pixel takes part if at least one side is >= 0, and its pair is (a, b) with -1 for none.  Either map may be
 * the `ids` map ubi_tabulate wrote or any caller's instance-id image.
 *
 * The weight of a pixel is that of ubresnet_moment.h, for its float32 ADC v and a scale that is a power of two in
 * 1..UBH_MAX_SCALE (so that t = v * scale is exact in float32):
 *   NaN, or t < 0               w = 0
 *   t > 65535 (+inf included)   w = 65535
 *   otherwise                   w = rint(t), ties to even; -0.0, +0.0 and whatever rounds to 0 give w = 0
 * Only the ADC of a pixel that takes part is read at all.  Without a view (NULL) every w is 0.
 */
#ifndef UBRESNET_OVERLAP_H
#define UBRESNET_OVERLAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBH_OK 0
#define UBH_EINVAL (-1)   /* bad argument */
#define UBH_ELAUNCH (-2)  /* hip launch error */

/* launch geometry and limits (csrc/ubr_overlap_plan.h holds the plan, the key, the hash and the probe sequence, and derives the
 * overflow bound: pixels < 2^31 and Q < 2^47, so no column can overflow).  A workgroup of UBH_LANES lanes takes UBH_TRIP_PIXELS
 * consecutive pixels per trip and a contiguous span of trips; there are at most UBH_MAX_GRID workgroups.  The waves of a
 * workgroup combine in an LDS table of UBH_LDS_SLOTS pairs.  A pair probes at most UBH_PROBES = min(slots, UBH_MAX_PROBES) slots
 * of the table in scratch. */
#define UBH_LANES 256
#define UBH_TRIP_PIXELS 2048
#define UBH_MAX_GRID 1024
#define UBH_LDS_SLOTS 64
#define UBH_COLUMNS 6
#define UBH_SLOT_WORDS 5 /* uint64 words of a slot in scratch */
#define UBH_MAX_PROBES 128
#define UBH_MIN_SLOTS 64
#define UBH_MAX_SLOTS 1073741824 /* 2^30 */
#define UBH_MAX_WEIGHT 65535
#define UBH_MAX_SCALE 256

/* the smallest power of two >= 2 * capacity and at least 1024 (a load of at most 0.5 when the table fills); 0 if capacity < 1
 * or the slots would pass UBH_MAX_SLOTS */
int64_t ubh_default_slots(int64_t capacity);

/* bytes of scratch for an image and a number of slots (a power of two in UBH_MIN_SLOTS..UBH_MAX_SLOTS): the slots, then the block
 * counts of the numbering; 0 for arguments ubh_overlap refuses */
int64_t ubh_scratch_bytes(int P, int rows, int cols, int64_t slots);

/* The pair table of two id maps.
 *   ids_a, ids_b   int32 [P][rows][cols], 16-byte aligned, P * rows * cols < 2^31
 *   view           float32 [P][rows][cols] (a [P][1][rows][cols] view is the same bytes), 16-byte aligned: the ADC; or NULL, and
 *                  then `weighted` and `Q` are 0
 *   adc_scale      a power of two in 1..UBH_MAX_SCALE (checked with or without a view)
 *   table          int64 [capacity][UBH_COLUMNS], 8-byte aligned; capacity >= 1.  With `total` the number of pairs, row
 *                  k < min(total, capacity) is STORED:
 *                    {a, b, first, pixels, weighted, Q}
 *                  first the smallest pixel index of the pair, pixels its pixel count, weighted the number of its pixels with
 *                  w > 0, Q the sum of w.  Rows are numbered in ascending order of `first`, so the table is a property of the two
 *                  maps and not of the schedule.  The pair (a, -1) holds the pixels of a that no cluster of b covers, and the
 *                  other way round, so both marginals follow from the table alone.  Rows at or past min(total, capacity) are
 *                  not written.
 *   count          uint64 on the device, 8-byte aligned, STORED: the total number of pairs, also where it exceeds capacity
 *   status         uint64 [2] on the device, 8-byte aligned, ADDED to: [0] counts the pixels whose pair found no slot; [1] is
 *                  reserved and stays 0
 *   scratch        ubh_scratch_bytes(P, rows, cols, slots) bytes, 16-byte aligned; slots as there
 * Five launches.  (1) The slots are cleared: key 0, first at its maximum, sums 0.  (2) Insert: a lane loads four consecutive ids
 * of each map in 16-byte loads and reads the view only where one of the four takes part; the lanes of a wave that share a pair are
 * combined; the waves of the workgroup then add into an LDS table keyed by the pair, whose occupied slots go to memory when the
 * table is more than half full at the end of a trip and when the workgroup ends.  A pair that finds no LDS slot goes to memory
 * directly.  Going to memory is an open-addressing insert: the key (a + 1) << 32 | (b + 1) is never 0, its home slot is
 * (key * 0x9E3779B97F4A7C15) >> (64 - log2 slots), probing is linear over at most UBH_PROBES slots, and a slot that holds the key
 * or whose 64-bit compare-and-swap of 0 to the key succeeded belongs to the pair; then come 64-bit atomic adds of the three sums
 * and an atomic minimum of first.  Zero columns are not sent.  A group that finds no slot adds its pixel count to status[0] and
 * is dropped; slots are never freed, so a pair is either wholly in the table or wholly dropped.  (3) The pair roots are counted
 * per block of 1024 pixels: a pixel that takes part looks its key up, read-only, along the same probe sequence, ending at an
 * empty slot or at the probe limit, and is a root if and only if the slot's first equals its own index.  (4) One workgroup scans
 * the block counts and stores count.  (5) Root k writes row k from its slot if k < capacity.
 * With status[0] == 0 the table, count and status are the same bytes on every run, stream and graph replay; the slot layout in
 * scratch is not, and nobody reads it.  With status[0] != 0 the table is unspecified beyond staying inside its buffer (count is
 * then at most slots). */
int ubh_overlap(const int32_t* ids_a, const int32_t* ids_b, const float* view_or_null, float adc_scale, long long* table,
                int64_t capacity, unsigned long long* count, unsigned long long* status, void* scratch, int64_t slots, int P, int rows,
                int cols, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubh_last_error(void);
int ubh_version(void);

#ifdef __cplusplus
}
#endif

#endif
