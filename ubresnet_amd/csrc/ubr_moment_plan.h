// The launch plan and the limits of libubresnet_moment.so (include/ubresnet_moment.h) as plain C++: no HIP, so
// tests/moment_host.cpp compiles it into a stand-alone program with the host sanitizers on.  What is refused, the LDS table, the
// clear grid and the overflow bound are decided here and nowhere else; the trip, the grid and the span of trips of a workgroup are
// the pixel walk of ubr_walk_plan.h, which libubresnet_overlap.so shares.
//
// The overflow bound.  A weight is at most MAX_WEIGHT = 2^16 - 1.  A row or column index is at most MAX_ROWS - 1 = 2^12 - 1, so
// r^2, r c and c^2 are below 2^24.  A cluster lies in one plane and a plane has at most MAX_PLANE_PIXELS = 2^22 pixels.  So the
// largest column of a row, Qrr or Qcc or Qrc, is at most MAX_WEIGHT * rows * cols * (max(rows, cols) - 1)^2 -- worst_column()
// below -- which is below 2^16 * 2^22 * 2^24 = 2^62 for every accepted shape; the partial sums in a lane, a wave and the LDS
// table are sums over a subset of the same pixels and so are below it as well.  Within one wave round a lane holds at most
// LANE_PIXELS pixels and a wave WAVE * LANE_PIXELS = 256: the pixel counts (three fields of COUNT_BITS bits in one word, each
// at most 256) and the charge (at most 256 * MAX_WEIGHT < 2^24) are summed in 32 bits, everything else in 64.
#ifndef UBR_MOMENT_PLAN_H
#define UBR_MOMENT_PLAN_H

#include "ubr_scan_plan.h"                            // MAX_PIXELS, the bound of an int32 pixel index, and nothing else
#include "ubr_walk_plan.h"

namespace ubm {

using walk::WAVE; using walk::LANES; using walk::LANE_PIXELS; using walk::TRIP_LOADS; using walk::TRIP_PIXELS;
using walk::MAX_GRID;                                 // workgroups of the accumulation and of the clear
using walk::COUNT_BITS;                               // weighted | clipped << 10 | odd << 20 within one wave round
using walk::MAX_WEIGHT; using walk::MAX_SCALE; using walk::valid_scale;
constexpr int SLOTS = 64;                             // clusters of the LDS table of a workgroup
constexpr int PROBES = 4;                             // slots a cluster tries, from k % SLOTS on, before it goes to memory directly
constexpr int FLUSH_ABOVE = SLOTS / 2;                // the table is sent and emptied at the end of a trip that leaves more slots taken
constexpr int MAX_CLASSES = 16;
constexpr int TABLE_FIXED = 9;                        // weighted, clipped, odd, Q, Qr, Qc, Qrr, Qrc, Qcc
constexpr int SLOT_WORDS = TABLE_FIXED + MAX_CLASSES; // uint64 words of one LDS slot
constexpr int64_t MAX_ROWS = 4096, MAX_COLS = 4096;
constexpr int64_t MAX_PLANE_PIXELS = (int64_t)1 << 22;
using scanplan::MAX_PIXELS;
static_assert((SLOTS & (SLOTS - 1)) == 0 && SLOTS <= LANES && PROBES <= SLOTS, "k % SLOTS is a mask; one lane resets one slot key");

// what the image may be; the reason it is refused in *why (a format for rows, cols or the pixel count) if not
inline bool valid_image(int64_t P, int64_t rows, int64_t cols, const char** why) {
  *why = "P, rows and cols must be positive";
  if (P < 1 || rows < 1 || cols < 1) return false;
  *why = "rows must be at most 4096 and cols at most 4096";
  if (rows > MAX_ROWS || cols > MAX_COLS) return false;
  *why = "rows * cols must be at most 2^22 (the overflow bound of a table column)";
  if (rows * cols > MAX_PLANE_PIXELS) return false;
  *why = "P * rows * cols must be below 2^31 pixels (int32 pixel index)";
  if (P > MAX_PIXELS / (rows * cols)) return false;
  *why = "";
  return true;
}

// the largest value a column of a table row can reach on a rows x cols plane (see the head of this file)
inline uint64_t worst_column(int64_t rows, int64_t cols) {
  const uint64_t far = (uint64_t)((rows > cols ? rows : cols) - 1);
  return (uint64_t)MAX_WEIGHT * (uint64_t)(rows * cols) * far * far;
}

struct Plan : walk::Walk {   // pixels = P * rows * cols, and its trips, span and grid
  int64_t clear_grid;  // workgroups of the clear: they stride over min(*count, capacity) * width words
};

// false (and nothing defined in *p) for an image valid_image refuses, capacity < 1 or C outside 1..MAX_CLASSES
inline bool make_plan(int64_t P, int64_t rows, int64_t cols, int64_t capacity, int64_t C, Plan* p) {
  const char* why;
  if (!valid_image(P, rows, cols, &why) || capacity < 1 || C < 1 || C > MAX_CLASSES) return false;
  static_cast<walk::Walk&>(*p) = walk::make_walk(P * rows * cols);
  // the rows that can be cleared are no more than the pixels: a cluster has a pixel
  const int64_t rows_max = capacity < p->pixels ? capacity : p->pixels;
  const int64_t units = (rows_max * (TABLE_FIXED + C) + LANES - 1) / LANES;
  p->clear_grid = units < MAX_GRID ? units : MAX_GRID;
  return true;
}

}  // namespace ubm

#endif
