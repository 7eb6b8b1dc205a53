/*
 * ubresnet_cluster.h -- C ABI of libubresnet_cluster.so (connected components of event products on the device: the lit pixels
 * of a class map grouped into clusters, numbered in a fixed order and summarised in an integer table; gfx950 / MI355X).
 *
 * A small library next to the others of the package.  It links against none of them and shares no state with them: it has its
 * own per-thread error string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_sparse.h: device pointers, `stream` is a hipStream_t passed as void*, all arguments are
 * validated on the host before any HIP call, 0 on success or a negative UBI_E* code with a message in ubi_last_error().  No
 * function allocates, frees or synchronises.  No launch argument depends on device state (the counts are read by the kernels),
 * so the calls capture into a graph as they are.  No kernel waits for another workgroup: there is no flag, no spinning and no
 * cooperative launch, and every find / union loop strictly decreases a pixel index on each trip.
 *
 * A pixel index is the int32 linear offset q = (plane * rows + row) * cols + col into a [P][rows][cols] image; images of
 * 2^31 pixels or more are refused.
 *
 * Pixel kinds, for a view `label` (uint8, as ubp_stitch_products writes it), C classes and a fill label:
 *   dark     label == fill_label
 *   lit      label != fill_label and label < C
 *   foreign  label != fill_label and label >= C: treated as dark, and counted into status[0], which is only ever ADDED to
 * Adjacency.  Two lit pixels are adjacent iff they lie in the same plane, and max(|dy|, |dx|) == 1 (connectivity 8) or
 * |dy| + |dx| == 1 (connectivity 4), and -- with by_class -- their labels are equal.  A row does not wrap into the next row and
 * a plane does not wrap into the next plane.
 * A cluster is a connected component of that graph.  Its root is the smallest pixel index in it, so the root map does not depend
 * on scheduling.  Clusters are numbered k = 0, 1, .. in ascending root order (plane-major, then row-major).
 */
#ifndef UBRESNET_CLUSTER_H
#define UBRESNET_CLUSTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBI_OK 0
#define UBI_EINVAL (-1)   /* bad argument */
#define UBI_ELAUNCH (-2)  /* hip launch error */

/* launch geometry (tests derive their sizes from it; csrc/ubr_cluster_plan.h holds the plan).  ubi_label gives one workgroup of
 * UBI_LANES lanes a UBI_TILE_H x UBI_TILE_W tile of one plane, a wave per tile row; its border pass has UBI_BORDER_LANES lanes
 * per tile.  The pixel passes give a workgroup UBI_PIXEL_BLOCK consecutive pixels; the scan is one workgroup that takes
 * UBI_SCAN_WIDTH block counts per trip.  ubi_gather_ids has at most UBI_MAX_GRID workgroups, which stride. */
#define UBI_TILE_H 32
#define UBI_TILE_W 64
#define UBI_LANES 256
#define UBI_BORDER_LANES 128
#define UBI_PIXEL_BLOCK 1024
#define UBI_SCAN_WIDTH 1024
#define UBI_MAX_GRID 4096
#define UBI_MAX_CLASSES 16
#define UBI_TABLE_FIXED 8 /* columns of a table row before the class counts */

/* bytes of scratch ubi_tabulate needs for a [P][rows][cols] image; 0 (and a message) for an image it refuses */
int64_t ubi_scratch_bytes(int P, int rows, int cols);

/* The root map: root[q] = the smallest pixel index of q's cluster for a lit pixel q, -1 for every other.  Every element of root
 * is written.  The number of foreign pixels is ADDED to status[0].
 *   label          [P][rows][cols] uint8
 *   C              1..UBI_MAX_CLASSES; fill_label 0..255; connectivity 4 or 8; by_class 0 or 1
 *   root           int32 [P][rows][cols], 4-byte aligned; overlaps no input
 *   status         uint64 on the device, ADDED to (one atomic add per workgroup at most)
 * Three launches: (1) a workgroup labels its tile in LDS -- row runs by wave ballot, then one union per adjacent pixel of the
 * row above -- and stores the index of the smallest pixel of each pixel's in-tile component; (2) every lit pixel of a tile's
 * last row and last column is united with its adjacent pixels of the neighbouring tiles, by find and atomicMin on root; (3)
 * root[q] = find(q), in place.  The result is the same for every schedule: the smallest index of a component is a property of
 * the image. */
int ubi_label(const uint8_t* label, int C, int fill_label, int connectivity, int by_class, int32_t* root,
              unsigned long long* status, int P, int rows, int cols, void* stream);

/* The clusters of a root map, numbered and summarised.
 *   label, confidence   [P][rows][cols] uint8 / IEEE half bits, the view that ubi_label read
 *   root                the root map of ubi_label(label, C, fill_label, ...)
 *   ids                 int32 [P][rows][cols]: the cluster number k of a lit pixel, -1 for every other.  Every element is
 *                       written, whatever the capacity.
 *   table               int64 [capacity][UBI_TABLE_FIXED + C], 8-byte aligned; capacity >= 1.  Row k < min(total, capacity):
 *                         {root, pixels, row_min, row_max, col_min, col_max, conf_sum, nonfinite, n_0 .. n_{C-1}}
 *                       conf_sum is the sum of fix(h) of ubresnet_score.h over the cluster's confidence bits h: the half's value
 *                       times 2^24 as an integer (a subnormal is its mantissa m, a normal is (1024 + m) << (e - 1)).  A half
 *                       with the sign bit and a non-zero magnitude, or an exponent of all ones (inf, NaN), adds nothing to
 *                       conf_sum and 1 to nonfinite.  0x8000 counts as zero.  n_c is the number of pixels of label c.
 *                       Rows at or past min(total, capacity) are not written.
 *   count               uint64 on the device, STORED: the total number of clusters, also where it exceeds capacity
 *   scratch             ubi_scratch_bytes(P, rows, cols) bytes, 16-byte aligned
 * Four launches: a count of the roots (root[q] == q) per pixel block, an exclusive scan of the counts by one workgroup, a
 * numbering pass (ids and the table row's constants at the roots, -1 at every pixel that is not lit), and a tally pass
 * (ids[q] = ids[root[q]], and integer atomicAdd / atomicMin / atomicMax into row k after the lanes of a wave that share k were
 * combined).  Every column is an integer sum, minimum or maximum: the table does not depend on scheduling. */
int ubi_tabulate(const uint8_t* label, const uint16_t* confidence, const int32_t* root, int C, int fill_label, int32_t* ids,
                 long long* table, int64_t capacity, unsigned long long* count, void* scratch, int P, int rows, int cols,
                 void* stream);

/* The cluster number of every entry of a pixel list: out[i] = ids[index[i]] for i < min(*list_count, list_capacity); -1 where
 * index[i] lies outside 0..pixels-1.  Entries at or past that length are not written.
 *   ids            int32 [pixels]; index int32 [list_capacity]; out int32 [list_capacity]; 1 <= pixels < 2^31
 *   list_count     uint64 on the device (the count of ubz_compact), read by the kernel
 * One launch. */
int ubi_gather_ids(const int32_t* ids, const int32_t* index, const unsigned long long* list_count, int64_t list_capacity,
                   int32_t* out, int64_t pixels, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubi_last_error(void);
int ubi_version(void);

#ifdef __cplusplus
}
#endif

#endif
