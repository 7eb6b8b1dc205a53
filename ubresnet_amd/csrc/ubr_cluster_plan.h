// The launch plan of libubresnet_cluster.so (include/ubresnet_cluster.h) as plain C++: no HIP, so tests/cluster_host.cpp
// compiles it into a stand-alone program with the host sanitizers on.  The tile, the grids of the labelling launches and the cap
// of the gather are decided here and nowhere else; the numbering is the pixel-block count / scan / rank of ubr_scan_plan.h with
// "is a root" as the predicate, and host_count / host_number say what its launches do with the shared walk.  model_find /
// model_unite restate the kernels' find and union loops one memory operation at a time, for that program to hold against brute
// force.
#ifndef UBR_CLUSTER_PLAN_H
#define UBR_CLUSTER_PLAN_H

#include "ubr_scan_plan.h"

namespace ubi {

using namespace scanplan;                             // the constants, lane_pixel, host_scan: under their names here as well
constexpr int TILE_H = 32;                            // a workgroup of the local pass labels a TILE_H x TILE_W tile in LDS
constexpr int TILE_W = WAVE;                          // a wave holds one tile row, a lane one pixel of it
constexpr int TILE_PIXELS = TILE_H * TILE_W;
constexpr int BORDER_LANES = 128;                     // border pass: lanes 0..TILE_W-1 the tile's last row, the next TILE_H its last column
constexpr int MAX_GRID = 4096;                        // workgroups of the gather launch (they stride)
constexpr int MAX_CLASSES = 16;
constexpr int TABLE_FIXED = 8;                        // root, pixels, row_min, row_max, col_min, col_max, conf_sum, nonfinite
static_assert(TILE_W + TILE_H <= BORDER_LANES && TILE_H % WAVES == 0, "the border lanes cover a row and a column of the tile");

struct Plan : scanplan::BlockPlan {                   // blocks: the grid of the flatten, count, number and tally passes
  int64_t tiles_y, tiles_x;
  int64_t tiles;          // P * tiles_y * tiles_x: the grid of the local and of the border pass; tile t is
                          // (plane, ty, tx) = (t / (tiles_y * tiles_x), t / tiles_x % tiles_y, t % tiles_x)
};

// false (and nothing defined in *p) when the image has no pixel or too many for an int32 index
inline bool make_plan(int64_t P, int64_t rows, int64_t cols, Plan* p) {
  if (!scanplan::make_block_plan(P, rows, cols, p)) return false;
  p->tiles_y = (rows + TILE_H - 1) / TILE_H;
  p->tiles_x = (cols + TILE_W - 1) / TILE_W;
  p->tiles = P * p->tiles_y * p->tiles_x;              // <= pixels
  return true;
}

inline int64_t stride_grid(int64_t units) { return scanplan::stride_grid(units, LANES, MAX_GRID); }

// ---- count / scan / number on the host: the shared walk with the root test ----

// scratch[b] = roots (root[q] == q) of block b
inline void host_count(const Plan& p, const int32_t* root, uint32_t* scratch) {
  scanplan::host_count(p, [root](int64_t q) { return root[q] == (int32_t)q; }, scratch);
}

// ids[q] = the number of q's cluster at the roots, -1 where root[q] < 0; the other lit pixels are the tally pass's
inline void host_number(const Plan& p, const int32_t* root, const uint32_t* scratch, int32_t* ids) {
  for (int64_t q = 0; q < p.pixels; ++q)
    if (root[q] < 0) ids[q] = -1;
  scanplan::host_rank(p, [root](int64_t q) { return root[q] == (int32_t)q; }, scratch, [ids](int64_t q, int64_t k) { ids[q] = (int32_t)k; });
}

// ---- the find and union loops of the kernels, one memory operation at a time ----
// parent[x] <= x for every lit x, parent[x] == x at a root.  A loop leaves when an index fails to decrease, so neither can run
// longer than the index it starts from, whatever another workgroup stores meanwhile.  `trips` counts loop trips.

inline int32_t model_find(const int32_t* parent, int32_t x, int64_t* trips) {
  for (;;) {
    ++*trips;
    const int32_t p = parent[x];
    if (p >= x || p < 0) return x;
    x = p;
  }
}

inline int32_t model_atomic_min(int32_t* word, int32_t v) {
  const int32_t old = *word;
  if (v < old) *word = v;
  return old;
}

// `between`, if not null, is called before every memory operation of the union loop: the other workgroups of the model
template <typename Between>
inline void model_unite(int32_t* parent, int32_t a, int32_t b, int64_t* trips, Between between) {
  for (;;) {
    ++*trips;
    between();
    a = model_find(parent, a, trips);
    between();
    b = model_find(parent, b, trips);
    if (a == b) return;
    if (a > b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    between();
    const int32_t old = model_atomic_min(parent + b, a);     // b: the larger root
    if (old >= b) return;                                    // b was a root still: linked
    b = old;                                                 // old < b: b had been linked meanwhile; unite its old parent with a
  }
}

}  // namespace ubi

#endif
