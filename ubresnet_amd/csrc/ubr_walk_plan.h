// The pixel walk that libubresnet_moment.so and libubresnet_overlap.so share, as plain C++: no HIP and no other header of the
// project, so the stand-alone host programs of tests/ compile it with the host sanitizers on.  A workgroup of LANES lanes takes a
// contiguous span of trips; a trip is TRIP_LOADS loads of LANE_PIXELS consecutive pixels per lane.  The trip, the span, the grid,
// the bounds of one wave round and the scales of the weight rule (ubr_adc_rule.h) are decided here and nowhere else;
// tests/walk_host.cpp holds the tiling against a marking loop.  The device side of the same walk is ubr_walk.h.
#ifndef UBR_WALK_PLAN_H
#define UBR_WALK_PLAN_H

#include <stdint.h>

namespace walk {

constexpr int WAVE = 64;
constexpr int LANES = 256;                            // lanes of a workgroup: four waves
constexpr int LANE_PIXELS = 4;                        // pixels of one lane per load: one 16-byte load of each id map
constexpr int TRIP_LOADS = 2;                         // loads of one lane per trip, all issued before any is used
constexpr int TRIP_PIXELS = LANES * LANE_PIXELS * TRIP_LOADS;
constexpr int MAX_GRID = 1024;                        // workgroups of the walk (and of the clear before it)
constexpr int COUNT_BITS = 10;                        // a pixel count of one wave round is a field of this many bits in one word
constexpr int64_t MAX_WEIGHT = 65535;
constexpr int MAX_SCALE = 256;
static_assert(WAVE * LANE_PIXELS < (1 << COUNT_BITS), "a count field holds the pixels of a wave round");
static_assert((uint64_t)WAVE * LANE_PIXELS * MAX_WEIGHT < ((uint64_t)1 << 32), "the charge of a wave round fits 32 bits");

// adc_scale: a power of two in 1..MAX_SCALE
inline bool valid_scale(float s) {
  for (int p = 1; p <= MAX_SCALE; p *= 2)
    if (s == (float)p) return true;
  return false;
}

struct Walk {
  int64_t pixels;
  int64_t trips;       // ceil(pixels / TRIP_PIXELS)
  int64_t span;        // consecutive trips of one workgroup: workgroup g takes trips g * span .. min((g + 1) * span, trips) - 1
  int64_t grid;        // ceil(trips / span) <= MAX_GRID: no workgroup is without a trip
};

// pixels >= 1 (the caller's valid_image)
inline Walk make_walk(int64_t pixels) {
  Walk w;
  w.pixels = pixels;
  w.trips = (pixels + TRIP_PIXELS - 1) / TRIP_PIXELS;
  const int64_t g = w.trips < MAX_GRID ? w.trips : MAX_GRID;
  w.span = (w.trips + g - 1) / g;
  w.grid = (w.trips + w.span - 1) / w.span;
  return w;
}

}  // namespace walk

#endif
