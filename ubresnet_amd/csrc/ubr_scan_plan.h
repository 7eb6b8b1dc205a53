// The pixel-block compaction the event-product libraries share (ubz_compact of libubresnet_sparse.so, the numbering of
// libubresnet_cluster.so), as plain C++: no HIP and no other header of the project, so the stand-alone host programs of tests/
// compile it with the host sanitizers on.  Three launches: every workgroup counts the pixels of its block that a predicate names;
// ONE workgroup scans the block counts in place; every workgroup ranks its named pixels from its block's offset.  The pixel
// block, the number of blocks, the scan's trip count and the scratch layout are decided here and nowhere else; host_count /
// host_scan / host_rank restate the three launches over the same plan, for tests/scan_host.cpp to hold against brute force.  The
// device side of the same launches is ubr_wave.h.
#ifndef UBR_SCAN_PLAN_H
#define UBR_SCAN_PLAN_H

#include <stdint.h>

namespace scanplan {

constexpr int WAVE = 64;
constexpr int LANES = 256;                            // lanes of a workgroup: four waves
constexpr int WAVES = LANES / WAVE;
constexpr int LANE_PIXELS = 4;                        // consecutive pixels of one lane: one 16-byte load
constexpr int PIXEL_BLOCK = LANES * LANE_PIXELS;      // B: pixels of one workgroup of the count and rank passes
constexpr int SCAN_LANE_COUNTS = 4;                   // block counts of one lane of the scan per trip: one 16-byte load
constexpr int SCAN_WIDTH = LANES * SCAN_LANE_COUNTS;  // S: block counts of one trip of the one-workgroup scan
constexpr int64_t MAX_PIXELS = ((int64_t)1 << 31) - 1;  // a pixel index is an int32

struct BlockPlan {
  int64_t pixels;         // P * rows * cols
  int64_t blocks;         // ceil(pixels / PIXEL_BLOCK): the grid of the count and of the rank pass
  int64_t scan_trips;     // ceil(blocks / SCAN_WIDTH): trips of the scan's single workgroup
  int64_t scratch_words;  // uint32 words of scratch: blocks rounded up to SCAN_LANE_COUNTS; word b is block b's count after
                          // the count pass and the number of named pixels before block b after the scan
  int64_t scratch_bytes;
};

// false (and nothing defined in *p) when the image has no pixel or too many for an int32 index
inline bool make_block_plan(int64_t P, int64_t rows, int64_t cols, BlockPlan* p) {
  if (P < 1 || rows < 1 || cols < 1) return false;
  if (rows > MAX_PIXELS / P || cols > MAX_PIXELS / (P * rows)) return false;
  p->pixels = P * rows * cols;
  p->blocks = (p->pixels + PIXEL_BLOCK - 1) / PIXEL_BLOCK;
  p->scan_trips = (p->blocks + SCAN_WIDTH - 1) / SCAN_WIDTH;
  p->scratch_words = (p->blocks + SCAN_LANE_COUNTS - 1) / SCAN_LANE_COUNTS * SCAN_LANE_COUNTS;
  p->scratch_bytes = 4 * p->scratch_words;
  return true;
}

// workgroups of a striding launch over `units` units of `lanes` lanes each, `max_grid` at most; 0 when there is nothing to do
inline int64_t stride_grid(int64_t units, int64_t lanes, int64_t max_grid) {
  const int64_t trips = (units + lanes - 1) / lanes;
  return trips > max_grid ? max_grid : trips;
}

// ---- the three launches on the host, block by block and lane by lane as the kernels walk them ----

// the pixel of lane `lane`, slot j of block b in the count and rank passes: a lane holds LANE_PIXELS consecutive pixels
inline int64_t lane_pixel(int64_t b, int lane, int j) { return b * PIXEL_BLOCK + (int64_t)lane * LANE_PIXELS + j; }

// launch 1: scratch[b] = the pixels q of block b with named(q)
template <typename Named>
inline void host_count(const BlockPlan& p, Named named, uint32_t* scratch) {
  for (int64_t b = 0; b < p.blocks; ++b) {
    uint32_t c = 0;
    for (int lane = 0; lane < LANES; ++lane)
      for (int j = 0; j < LANE_PIXELS; ++j) {
        const int64_t q = lane_pixel(b, lane, j);
        if (q < p.pixels && named(q)) ++c;
      }
    scratch[b] = c;
  }
}

// launch 2: an exclusive scan in place, SCAN_WIDTH counts per trip with the carry of the trips before; -> the total
inline uint64_t host_scan(const BlockPlan& p, uint32_t* scratch) {
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

// launch 3: put(q, k) for the k-th named pixel q of the image, in ascending order of q
template <typename Named, typename Put>
inline void host_rank(const BlockPlan& p, Named named, const uint32_t* scratch, Put put) {
  for (int64_t b = 0; b < p.blocks; ++b) {
    int64_t k = scratch[b];
    for (int lane = 0; lane < LANES; ++lane)
      for (int j = 0; j < LANE_PIXELS; ++j) {
        const int64_t q = lane_pixel(b, lane, j);
        if (q < p.pixels && named(q)) put(q, k++);
      }
  }
}

}  // namespace scanplan

#endif
