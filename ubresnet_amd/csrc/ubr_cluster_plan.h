// The launch plan of libubresnet_cluster.so (include/ubresnet_cluster.h) as plain C++: no HIP, so tests/cluster_host.cpp
// compiles it into a stand-alone program with the host sanitizers on.  The tile, the pixel block, the grids and the scratch
// layout are decided here and nowhere else; host_count / host_scan / host_number restate the numbering launches over the same
// plan, and model_find / model_unite restate the kernels' find and union loops one memory operation at a time, for that
// program to hold against brute force.  (The pixel-block count and scan are those of ubr_sparse_plan.h, restated: the two
// libraries share no header.)
#ifndef UBR_CLUSTER_PLAN_H
#define UBR_CLUSTER_PLAN_H

#include <stdint.h>

namespace ubi {

constexpr int WAVE = 64;
constexpr int LANES = 256;                            // lanes of every workgroup but the border pass's: four waves
constexpr int WAVES = LANES / WAVE;
constexpr int TILE_H = 32;                            // a workgroup of the local pass labels a TILE_H x TILE_W tile in LDS
constexpr int TILE_W = WAVE;                          // a wave holds one tile row, a lane one pixel of it
constexpr int TILE_PIXELS = TILE_H * TILE_W;
constexpr int BORDER_LANES = 128;                     // border pass: lanes 0..TILE_W-1 the tile's last row, the next TILE_H its last column
constexpr int LANE_PIXELS = 4;                        // pixels of one lane of the pixel passes
constexpr int PIXEL_BLOCK = LANES * LANE_PIXELS;      // pixels of one workgroup of the pixel passes
constexpr int SCAN_LANE_COUNTS = 4;                   // block counts of one lane of the scan per trip: one 16-byte load
constexpr int SCAN_WIDTH = LANES * SCAN_LANE_COUNTS;  // block counts of one trip of the one-workgroup scan
constexpr int MAX_GRID = 4096;                        // workgroups of the gather launch (they stride)
constexpr int MAX_CLASSES = 16;
constexpr int TABLE_FIXED = 8;                        // root, pixels, row_min, row_max, col_min, col_max, conf_sum, nonfinite
constexpr int64_t MAX_PIXELS = ((int64_t)1 << 31) - 1;  // a pixel index is an int32
static_assert(TILE_W + TILE_H <= BORDER_LANES && TILE_H % WAVES == 0, "the border lanes cover a row and a column of the tile");

struct Plan {
  int64_t pixels;         // P * rows * cols
  int64_t tiles_y, tiles_x;
  int64_t tiles;          // P * tiles_y * tiles_x: the grid of the local and of the border pass; tile t is
                          // (plane, ty, tx) = (t / (tiles_y * tiles_x), t / tiles_x % tiles_y, t % tiles_x)
  int64_t blocks;         // ceil(pixels / PIXEL_BLOCK): the grid of the flatten, count, number and tally passes
  int64_t scan_trips;     // ceil(blocks / SCAN_WIDTH): trips of the scan's single workgroup
  int64_t scratch_words;  // uint32 words of scratch: blocks rounded up to SCAN_LANE_COUNTS; word b is block b's root count
                          // after the count pass and the number of roots before block b after the scan
  int64_t scratch_bytes;
};

// false (and nothing defined in *p) when the image has no pixel or too many for an int32 index
inline bool make_plan(int64_t P, int64_t rows, int64_t cols, Plan* p) {
  if (P < 1 || rows < 1 || cols < 1) return false;
  if (rows > MAX_PIXELS / P || cols > MAX_PIXELS / (P * rows)) return false;
  p->pixels = P * rows * cols;
  p->tiles_y = (rows + TILE_H - 1) / TILE_H;
  p->tiles_x = (cols + TILE_W - 1) / TILE_W;
  p->tiles = P * p->tiles_y * p->tiles_x;              // <= pixels
  p->blocks = (p->pixels + PIXEL_BLOCK - 1) / PIXEL_BLOCK;
  p->scan_trips = (p->blocks + SCAN_WIDTH - 1) / SCAN_WIDTH;
  p->scratch_words = (p->blocks + SCAN_LANE_COUNTS - 1) / SCAN_LANE_COUNTS * SCAN_LANE_COUNTS;
  p->scratch_bytes = 4 * p->scratch_words;
  return true;
}

// workgroups of a striding launch over `units` units of LANES lanes each; 0 when there is nothing to do
inline int64_t stride_grid(int64_t units) {
  const int64_t trips = (units + LANES - 1) / LANES;
  return trips > MAX_GRID ? MAX_GRID : trips;
}

// ---- count / scan / number on the host, block by block and lane by lane as the kernels walk them ----

// the pixel of lane `lane`, slot j of block b in the count and number passes: a lane holds LANE_PIXELS consecutive pixels
inline int64_t lane_pixel(int64_t b, int lane, int j) { return b * PIXEL_BLOCK + (int64_t)lane * LANE_PIXELS + j; }

// scratch[b] = roots (root[q] == q) of block b
inline void host_count(const Plan& p, const int32_t* root, uint32_t* scratch) {
  for (int64_t b = 0; b < p.blocks; ++b) {
    uint32_t c = 0;
    for (int lane = 0; lane < LANES; ++lane)
      for (int j = 0; j < LANE_PIXELS; ++j) {
        const int64_t q = lane_pixel(b, lane, j);
        if (q < p.pixels && root[q] == (int32_t)q) ++c;
      }
    scratch[b] = c;
  }
}

// an exclusive scan in place, SCAN_WIDTH counts per trip with the carry of the trips before; -> the total
inline uint64_t host_scan(const Plan& p, uint32_t* scratch) {
  uint32_t carry = 0;
  for (int64_t t = 0; t < p.scan_trips; ++t) {
    uint32_t lane_sum[LANES];
    for (int lane = 0; lane < LANES; ++lane) {
      lane_sum[lane] = 0;
      for (int k = 0; k < SCAN_LANE_COUNTS; ++k) {
        const int64_t i = t * SCAN_WIDTH + (int64_t)lane * SCAN_LANE_COUNTS + k;
        if (i < p.blocks) lane_sum[lane] += scratch[i];
      }
    }
    uint32_t before = carry;
    for (int lane = 0; lane < LANES; ++lane) {
      uint32_t run = before;
      for (int k = 0; k < SCAN_LANE_COUNTS; ++k) {
        const int64_t i = t * SCAN_WIDTH + (int64_t)lane * SCAN_LANE_COUNTS + k;
        if (i < p.blocks) {
          const uint32_t c = scratch[i];
          scratch[i] = run;
          run += c;
        }
      }
      before += lane_sum[lane];
    }
    carry = before;
  }
  return carry;
}

// ids[q] = the number of q's cluster at the roots, -1 where root[q] < 0; the other lit pixels are the tally pass's
inline void host_number(const Plan& p, const int32_t* root, const uint32_t* scratch, int32_t* ids) {
  for (int64_t b = 0; b < p.blocks; ++b) {
    int64_t k = scratch[b];
    for (int lane = 0; lane < LANES; ++lane)
      for (int j = 0; j < LANE_PIXELS; ++j) {
        const int64_t q = lane_pixel(b, lane, j);
        if (q >= p.pixels) continue;
        if (root[q] < 0) ids[q] = -1;
        if (root[q] == (int32_t)q) ids[q] = (int32_t)k++;
      }
  }
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
