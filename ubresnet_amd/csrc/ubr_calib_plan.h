// The launch plans of libubresnet_calib.so (ubf_accumulate and ubf_apply of include/ubresnet_calib.h) as plain C++: no HIP, so
// tests/calib_host.cpp compiles it into a stand-alone program with the host sanitizers on.  The trip, the grids, the layout of
// the per-workgroup partial rows and the order in which the finish adds them are decided here and nowhere else; host_walk and
// host_finish restate the two launches of ubf_accumulate over the same plan, for that program to hold against brute force.
#ifndef UBR_CALIB_PLAN_H
#define UBR_CALIB_PLAN_H

#include <stdint.h>

namespace ubf {

constexpr int WAVE = 64;
constexpr int BLOCK = 256;                            // lanes of a streaming workgroup: four waves
constexpr int WAVES = BLOCK / WAVE;
constexpr int LANE_PIXELS = 4;                        // consecutive pixels of a unit: one 16-byte load of a float plane
constexpr int UNROLL = 2;                             // units of one lane per trip
constexpr int TRIP_UNITS = BLOCK * UNROLL;
constexpr int TRIP_PIXELS = TRIP_UNITS * LANE_PIXELS; // 2048 consecutive pixels of one image
constexpr int MAX_TEMPS = 64;                         // K: lane k of every wave keeps the sums of inverse temperature k
constexpr int MAX_GROUPS = 256;                       // G: a group index is a uint8
constexpr int MAX_CLASSES = 16;
constexpr int REG_CLASSES = 4;                        // C <= REG_CLASSES: the class loops are unrolled over a constant
constexpr int MAX_IMAGES = 65535;                     // N: the second dimension of the grid
constexpr int MAX_ROWS = 768;                         // partial rows of one call, unless N alone exceeds it (one per image then):
                                                      // the one-workgroup finish reads them, a few dependent loads per lane at a time
constexpr int FINISH_SUB = 4;                         // the finish adds FINISH_SUB interleaved row sequences, then those in order
constexpr int FINISH_WORDS = 256;                     // lanes per sequence: >= the 3 K + 3 words of a row
constexpr int FINISH_BLOCK = FINISH_SUB * FINISH_WORDS;
constexpr int APPLY_MAX_GRID = 2048;                  // workgroups of ubf_apply: they walk consecutive trips, a grid apart
constexpr int64_t MAX_PIXELS = (int64_t)1 << 40;      // N * H * W

// ubf_accumulate.  The grid is (gx, N): the workgroups of row y take image y only, so the group of every pixel a workgroup
// meets is one number.  Workgroup (x, y) walks the trips x, x + gx, .. of image y and leaves partial row y * gx + x:
//   words 0 .. 3 K - 1   double [K][3]   {NLL, g, h} of inverse temperature k
//   words 3 K .. 3 K + 2 uint64 [3]      {counted, ignored, non-finite}
// Every workgroup writes its whole row, so the scratch needs no clearing.
struct Plan {
  int64_t hw;             // H * W
  int64_t trips;          // ceil(hw / TRIP_PIXELS): trips of one image
  int64_t gx;             // workgroups per image
  int64_t rows;           // N * gx partial rows
  int64_t row_words;      // 3 K + 3
  int64_t scratch_bytes;  // 8 * rows * row_words
};

// false (and nothing defined in *p) for what ubf_accumulate refuses
inline bool make_plan(int64_t N, int64_t H, int64_t W, int64_t K, Plan* p) {
  if (N < 1 || N > MAX_IMAGES || H < 1 || W < 1 || K < 1 || K > MAX_TEMPS) return false;
  if (H > MAX_PIXELS / N || W > MAX_PIXELS / (N * H)) return false;
  p->hw = H * W;
  p->trips = (p->hw + TRIP_PIXELS - 1) / TRIP_PIXELS;
  int64_t per_image = MAX_ROWS / N;
  if (per_image < 1) per_image = 1;
  p->gx = p->trips < per_image ? p->trips : per_image;
  p->rows = N * p->gx;
  p->row_words = 3 * K + 3;
  p->scratch_bytes = 8 * p->rows * p->row_words;
  return true;
}

// pixel q of slot (unit u, lane) of trip t, within the image; the kernel checks it against hw
inline int64_t pixel_of(int64_t trip, int u, int lane, int q) {
  return (trip * TRIP_UNITS + (int64_t)u * BLOCK + lane) * LANE_PIXELS + q;
}

// launch 1 on the host, as the workgroups walk it: seen[n * hw + p] += 1 for every pixel a lane would look at, and row
// (n * gx + x) of `rows` gets word 0 of every k = the number of pixels it met (as a double), counters = {met, 0, 0}
inline void host_walk(const Plan& p, int64_t N, int64_t K, uint8_t* seen, uint64_t* rows) {
  for (int64_t n = 0; n < N; ++n)
    for (int64_t x = 0; x < p.gx; ++x) {
      uint64_t met = 0;
      for (int64_t t = x; t < p.trips; t += p.gx)
        for (int u = 0; u < UNROLL; ++u)
          for (int lane = 0; lane < BLOCK; ++lane)
            for (int q = 0; q < LANE_PIXELS; ++q) {
              const int64_t px = pixel_of(t, u, lane, q);
              if (px < p.hw) {
                seen[n * p.hw + px] += 1;
                ++met;
              }
            }
      uint64_t* row = rows + (n * p.gx + x) * p.row_words;
      for (int64_t k = 0; k < K; ++k) {
        const double v = (double)met;
        uint64_t bits;
        __builtin_memcpy(&bits, &v, 8);
        row[3 * k] = bits;
        row[3 * k + 1] = 0;
        row[3 * k + 2] = 0;
      }
      row[3 * K] = met;
      row[3 * K + 1] = 0;
      row[3 * K + 2] = 0;
    }
}

// launch 2 on the host, in the finish kernel's order.  Per image n in ascending order: word w of its gx rows is added as
// FINISH_SUB sequences (rows s, s + FINISH_SUB, ..), the sequences in order, and the sum is added onto group[n]'s word of the
// table (doubles) or of the counters (integers).  An image whose group is not below G is left out.
inline void host_finish(const Plan& p, int64_t N, int64_t K, int64_t G, const uint8_t* group, const uint64_t* rows, double* table,
                        uint64_t* counters) {
  for (int64_t n = 0; n < N; ++n) {
    if (group[n] >= G) continue;
    for (int64_t w = 0; w < p.row_words; ++w) {
      const bool integer = w >= 3 * K;
      uint64_t ai = 0;
      double ad = 0.0;
      for (int s = 0; s < FINISH_SUB; ++s) {
        uint64_t si = 0;
        double sd = 0.0;
        for (int64_t r = s; r < p.gx; r += FINISH_SUB) {
          const uint64_t v = rows[(n * p.gx + r) * p.row_words + w];
          double d;
          __builtin_memcpy(&d, &v, 8);
          if (integer) si += v; else sd += d;
        }
        ai += si;
        ad += sd;
      }
      if (integer)
        counters[group[n] * 3 + (w - 3 * K)] += ai;
      else
        table[group[n] * 3 * K + w] += ad;
    }
  }
}

// ubf_apply: units of LANE_PIXELS pixels (vector path) or single pixels, UNROLL of them per lane and trip
struct ApplyPlan {
  int64_t units;          // n * th * tw / LANE_PIXELS on the vector path, n * th * tw otherwise
  int64_t trips;          // ceil(units / TRIP_UNITS)
  int64_t grid;           // min(trips, APPLY_MAX_GRID)
};

inline bool make_apply_plan(int64_t n, int64_t th, int64_t tw, bool vec, ApplyPlan* p) {
  if (n < 1 || th < 1 || tw < 1) return false;
  if (th > MAX_PIXELS / n || tw > MAX_PIXELS / (n * th)) return false;
  const int64_t pixels = n * th * tw;
  if (vec && (th * tw) % LANE_PIXELS) return false;
  p->units = vec ? pixels / LANE_PIXELS : pixels;
  p->trips = (p->units + TRIP_UNITS - 1) / TRIP_UNITS;
  p->grid = p->trips < APPLY_MAX_GRID ? p->trips : APPLY_MAX_GRID;
  return true;
}

}  // namespace ubf

#endif
