// The launch plan and the limits of libubresnet_match.so (include/ubresnet_match.h) as plain C++: no HIP, so
// tests/match_host.cpp compiles it into a stand-alone program with the host sanitizers on.  What is refused, the time bins, the
// chunks, the tile enumeration of the match launch, the scratch layout and the overflow bounds are decided here and nowhere else;
// the trip, the grid and the span of the profile launch are the pixel walk of ubr_walk_plan.h.
//
// The bounds.  A weight is at most MAX_WEIGHT = 2^16 - 1.  A time bin of one candidate covers time_bin rows of one plane, so it
// holds at most time_bin * cols pixels and at most time_bin * cols * 65535 charge, which is below 2^32 for
// time_bin * cols <= MAX_BIN_PIXELS = 65536: bin_bound() below.  Larger products are refused, so a 32-bit bin cannot wrap; the
// pixel count of a bin is at most 65536 and fits 32 bits as well.  A candidate has at most MAX_ROWS = 4096 bins, so Q, I, Qi_in
// and Qj_in are below 2^12 * 2^32 = 2^44 and are summed in 64 bits.  Within one wave round a wave holds WAVE * LANE_PIXELS = 256
// pixels: their charge (below 2^24) and their count are summed in 32 bits.  slot * T + t is below 2^12 * 2^12 = 2^24.
#ifndef UBR_MATCH_PLAN_H
#define UBR_MATCH_PLAN_H

#include "ubr_scan_plan.h"                            // MAX_PIXELS, the bound of an int32 pixel index, and nothing else
#include "ubr_walk_plan.h"

#if defined(__HIPCC__)
#define UBU_HD __host__ __device__ __forceinline__
#else
#define UBU_HD inline
#endif

namespace ubu {

using walk::WAVE; using walk::LANES; using walk::LANE_PIXELS; using walk::TRIP_PIXELS;
using walk::MAX_GRID;                                 // workgroups of the profile walk and of the clear
using walk::MAX_WEIGHT; using walk::MAX_SCALE; using walk::valid_scale;
using scanplan::MAX_PIXELS;
constexpr int WAVES = LANES / WAVE;                   // candidates of one workgroup of the summary: a wave each
constexpr int TILE = 64;                              // candidates of one side of a tile of pairs
constexpr int LANE_TILE = 4;                          // a lane owns LANE_TILE x LANE_TILE pairs of its tile
constexpr int CHUNK_BINS = 64;                        // time bins of one staged chunk: one occupancy word per candidate
constexpr int STRIP_STRIDE = CHUNK_BINS + 1;          // words of one candidate's chunk in LDS: odd, so a column of a strip spreads over the banks
constexpr int MIN_PLANES = 2, MAX_PLANES = 4;
constexpr int64_t MIN_SLOTS = 64, MAX_SLOTS = 4096;
constexpr int MAX_TIME_BIN = 64;
constexpr int MAX_SHIFT = 4096;                       // |row_shift[p]|
constexpr int64_t MAX_ROWS = 4096, MAX_COLS = 4096;
constexpr int64_t MAX_PLANE_PIXELS = (int64_t)1 << 22;
constexpr int64_t MAX_BIN_PIXELS = 65536;             // time_bin * cols
constexpr int CLUSTER_FIXED = 8;                      // columns of a row of ubi_tabulate's table before the class counts
constexpr int MAX_CLASSES = 16;
constexpr int CAND_COLUMNS = 6;                       // cluster, plane, Q, bins, t_min, t_max
constexpr int PAIR_COLUMNS = 4;                       // both, I, Qi_in, Qj_in
static_assert(LANES == (TILE / LANE_TILE) * (TILE / LANE_TILE), "the lanes of a workgroup cover a tile in 4 x 4 blocks");
static_assert(CHUNK_BINS == WAVE, "a wave ballots the occupancy word of a chunk");
static_assert(MAX_SLOTS * MAX_ROWS <= ((int64_t)1 << 24), "slot * T + t is a 32-bit index");
static_assert(2 * TILE * STRIP_STRIDE * 4 + 2 * TILE * 8 <= 64 * 1024, "both strips and their occupancy words fit the LDS of a workgroup");

// what the image may be; the reason it is refused in *why if not: the limits of ubr_moment_plan.h, and 2..4 planes
inline bool valid_image(int64_t P, int64_t rows, int64_t cols, const char** why) {
  *why = "P must be 2..4 and rows and cols positive";
  if (P < MIN_PLANES || P > MAX_PLANES || rows < 1 || cols < 1) return false;
  *why = "rows must be at most 4096 and cols at most 4096";
  if (rows > MAX_ROWS || cols > MAX_COLS) return false;
  *why = "rows * cols must be at most 2^22";
  if (rows * cols > MAX_PLANE_PIXELS) return false;
  *why = "";
  return true;                                        // 4 * 2^22 pixels are below 2^31
}

// log2 of a power of two in 1..MAX_TIME_BIN; -1 for anything else
inline int log2_time_bin(int64_t time_bin) {
  for (int l = 0; (1 << l) <= MAX_TIME_BIN; ++l)
    if (time_bin == ((int64_t)1 << l)) return l;
  return -1;
}

inline bool valid_slots(int64_t slots) { return slots >= MIN_SLOTS && slots <= MAX_SLOTS && slots % TILE == 0; }

// the most a 32-bit bin can hold: time_bin * cols pixels at the largest weight
inline uint64_t bin_bound(int64_t time_bin, int64_t cols) { return (uint64_t)(time_bin * cols) * (uint64_t)MAX_WEIGHT; }

// ---- the tiles of the match launch: the upper triangle of nt x nt tiles, row by row ----
inline int64_t tile_count(int64_t nt) { return nt * (nt + 1) / 2; }

// tile b < tile_count(nt) -> (ti, tj), ti <= tj < nt; at most nt trips
UBU_HD void tile_of(int b, int nt, int* ti, int* tj) {
  int i = 0;
  for (int trip = 0; trip < nt; ++trip) {
    const int in_row = nt - i;
    if (b < in_row) break;
    b -= in_row;
    ++i;
  }
  *ti = i;
  *tj = i + b;
}

struct Plan : walk::Walk {   // pixels = P * rows * cols, and its trips, span and grid: the profile launch
  int64_t T;             // time bins: ceil(rows / time_bin)
  int log2_bin;
  int64_t chunks;        // ceil(T / CHUNK_BINS): trips of the summary and of the match over the bins
  int64_t rows_max;      // min(capacity, pixels): the rows of the cluster table that can exist
  int64_t select_trips;  // ceil(rows_max / LANES): trips of the one workgroup of the select
  int64_t clear_grid;    // workgroups of the clear: they stride over slots * T words (twice) and the candidate table
  int64_t summary_grid;  // slots / WAVES
  int64_t tiles;         // slots / TILE
  int64_t match_grid;    // tile_count(tiles)
  // scratch: the occupancy words uint64 [slots][chunks], the pixel counts uint32 [slots][T], slot_of int32 [rows_max]
  int64_t mask_bytes, occ_offset, occ_bytes, slot_offset, slot_bytes, scratch_bytes;
};

// false (and *why set) for what ubu_match refuses of these arguments
inline bool make_plan(int64_t P, int64_t rows, int64_t cols, int64_t time_bin, int64_t slots, int64_t capacity, Plan* p, const char** why) {
  if (!valid_image(P, rows, cols, why)) return false;
  *why = "time_bin must be a power of two in 1..64";
  const int l = log2_time_bin(time_bin);
  if (l < 0) return false;
  *why = "time_bin * cols must be at most 65536 (a bin is 32 bits)";
  if (time_bin * cols > MAX_BIN_PIXELS) return false;
  *why = "slots must be a multiple of 64 in 64..4096";
  if (!valid_slots(slots)) return false;
  *why = "capacity must be >= 1";
  if (capacity < 1) return false;
  *why = "";
  static_cast<walk::Walk&>(*p) = walk::make_walk(P * rows * cols);
  p->log2_bin = l;
  p->T = (rows + time_bin - 1) / time_bin;
  p->chunks = (p->T + CHUNK_BINS - 1) / CHUNK_BINS;
  p->rows_max = capacity < p->pixels ? capacity : p->pixels;
  p->select_trips = (p->rows_max + LANES - 1) / LANES;
  p->clear_grid = scanplan::stride_grid(slots * p->T, LANES, MAX_GRID);
  p->summary_grid = slots / WAVES;
  p->tiles = slots / TILE;
  p->match_grid = tile_count(p->tiles);
  p->mask_bytes = 8 * slots * p->chunks;
  p->occ_offset = p->mask_bytes;
  p->occ_bytes = (4 * slots * p->T + 15) / 16 * 16;
  p->slot_offset = p->occ_offset + p->occ_bytes;
  p->slot_bytes = (4 * p->rows_max + 15) / 16 * 16;
  p->scratch_bytes = p->slot_offset + p->slot_bytes;
  return true;
}

}  // namespace ubu

#endif
