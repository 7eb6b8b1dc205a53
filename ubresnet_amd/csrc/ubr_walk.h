// The device side of the pixel walk of ubr_walk_plan.h, which moment_kernel (extra/ubr_moment.hip) and insert_kernel
// (extra/ubr_overlap.hip) share: the 16-byte id load of a lane with its ragged tail, the round that combines the lanes of a wave
// key by key, and the trip loop of a workgroup around an LDS table that it flushes.  What is summed, the LDS tables, where a
// group's sums go and the view load (moment loads view and label under one branch) are each library's own.  A function that says it holds a barrier is called by every lane of the workgroup.
// Device code only.
#ifndef UBR_WALK_H
#define UBR_WALK_H

#include <hip/hip_runtime.h>
#include "ubr_walk_plan.h"
#include "ubr_wave.h"

namespace walk {

constexpr int LOAD_PIXELS = LANES * LANE_PIXELS;      // pixels of one load of the workgroup

// four ids of one map from pixel p on (p a multiple of four, the map 16-byte aligned); -1 past the end of the image
__device__ __forceinline__ int4 load_ids(const int32_t* __restrict__ ids, unsigned p, unsigned pixels) {
  if (p + 3u < pixels) return *(const int4*)(ids + p);
  int4 r;
  r.x = p < pixels ? ids[p] : -1;
  r.y = p + 1u < pixels ? ids[p + 1u] : -1;
  r.z = p + 2u < pixels ? ids[p + 2u] : -1;
  r.w = -1;                                                       // p + 3 >= pixels
  return r;
}

// One wave round over the keys of the active lanes.  The lanes that share a key are found by ballot, one trip of the loop per
// distinct key: each trip clears at least one bit of `rem`.  group(g, lane) is called wave-uniformly for every group of two or
// more lanes (it sums over g.member and lets g.leader send the sums on); a lane alone with its key calls solo() after the loop,
// together with the other such lanes.
template <typename K, typename Group, typename Solo>
__device__ __forceinline__ void wave_round(K key, bool active, Group group, Solo solo) {
  const int lane = threadIdx.x & 63;
  wv::u64 rem = __ballot(active);
  bool alone = false;
  while (rem != 0ull) {                                           // wave-uniform
    const wv::KeyGroup<K> g = wv::next_key_group(rem, key, active);
    if (__popcll(g.lanes) == 1) {
      alone = alone || lane == g.leader;
      continue;
    }
    group(g, lane);
  }
  if (alone) solo();
}

// The trips blockIdx.x * span .. min(that + span, trips) - 1 of a workgroup.  A trip calls load(p) TRIP_LOADS times, all before
// any is used -- p (< 2^31 + TRIP_PIXELS) is the lane's first pixel of the load, and what load returns are the ids of its four
// pixels in the library's one or two maps -- then step(p, ids) once per load.  *s_used counts the taken slots of the workgroup's
// LDS table; flush() sends and empties the table, and begins with a barrier of its own.  Holds two barriers per trip.
template <typename Load, typename Step, typename Flush>
__device__ __forceinline__ void trip_loop(unsigned trips, unsigned span, const unsigned* s_used, unsigned flush_above, Load load,
                                          Step step, Flush flush) {
  const unsigned t0 = blockIdx.x * span;
  unsigned t1 = t0 + span;
  if (t1 > trips) t1 = trips;
  for (unsigned t = t0; t < t1; ++t) {                            // workgroup-uniform
    const unsigned p0 = t * (unsigned)TRIP_PIXELS + threadIdx.x * 4u;
    decltype(load(0u)) k[TRIP_LOADS];
#pragma unroll
    for (int u = 0; u < TRIP_LOADS; ++u) k[u] = load(p0 + (unsigned)u * LOAD_PIXELS);
#pragma unroll
    for (int u = 0; u < TRIP_LOADS; ++u) step(p0 + (unsigned)u * LOAD_PIXELS, k[u]);
    __syncthreads();                                              // every claim of this trip is counted
    const unsigned used = *s_used;
    __syncthreads();                                              // nobody claims a slot of the next trip before everybody has read
    if (used > flush_above) flush();                              // workgroup-uniform
  }
  flush();
}

}  // namespace walk

#endif
