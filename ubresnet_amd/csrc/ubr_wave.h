// The wave and workgroup primitives of the event-product libraries (extra/ubr_sparse.hip, ubr_cluster.hip, ubr_moment.hip,
// ubr_crop.hip, ubr_score.hip, ubr_overlap.hip): integer sums across a wave, the walk over the distinct keys of a wave, and the count, rank and
// scan of a workgroup of 64-lane waves through a few words of LDS -- the device side of the three launches ubr_scan_plan.h plans.
// Everything is integer arithmetic, so no order of additions is anybody's contract (the fixed-order sums of the loss libraries
// are ubr_rows.h).  A function that says it holds a barrier is called by every lane of the workgroup, wave-uniformly.  Device
// code only.  No other header of the project is included here.
#ifndef UBR_WAVE_H
#define UBR_WAVE_H

#include <hip/hip_runtime.h>

namespace wv {

typedef unsigned long long u64;

// ---- sums across a wave, in every lane of it ----
__device__ __forceinline__ unsigned sum_all(unsigned v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (unsigned)__shfl_xor((int)v, d);
  return v;
}

// 64 bits as a butterfly of 32-bit halves
__device__ __forceinline__ u64 sum_all(u64 v) {
  unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    v += ((u64)(unsigned)__shfl_xor((int)hi, d) << 32) | (unsigned)__shfl_xor((int)lo, d);
    lo = (unsigned)v; hi = (unsigned)(v >> 32);
  }
  return v;
}

// ---- the walk over the distinct keys of a wave ----
// One trip of `while (rem != 0)`, rem = the ballot of the active lanes at first: the first remaining lane leads, the active lanes
// that hold its key are its group, and the group leaves rem -- so the loop makes one trip per distinct key.  Wave-uniform but for
// `member`.
template <typename K>
struct KeyGroup {
  int leader;     // the group's first lane
  K key;          // its key
  u64 lanes;      // the ballot of the group
  bool member;    // this lane belongs to it
};

template <typename K>
__device__ __forceinline__ KeyGroup<K> next_key_group(u64& rem, K key, bool active) {
  KeyGroup<K> g;
  g.leader = __ffsll((long long)rem) - 1;
  g.key = (K)__shfl((int)key, g.leader);
  g.member = active && key == g.key;
  g.lanes = __ballot(g.member);
  rem &= ~g.lanes;
  return g;
}

// the same for a 64-bit key, which travels as two 32-bit halves
__device__ __forceinline__ KeyGroup<u64> next_key_group(u64& rem, u64 key, bool active) {
  KeyGroup<u64> g;
  g.leader = __ffsll((long long)rem) - 1;
  g.key = ((u64)(unsigned)__shfl((int)(key >> 32), g.leader) << 32) | (unsigned)__shfl((int)key, g.leader);
  g.member = active && key == g.key;
  g.lanes = __ballot(g.member);
  rem &= ~g.lanes;
  return g;
}

// ---- a workgroup of WAVES waves; s_wave: WAVES words of LDS that the workgroup gives and nothing else uses meanwhile ----

// the set bits among bits 0..BITS-1 of the masks of a wave, in every lane of it
template <int BITS>
__device__ __forceinline__ unsigned mask_count(unsigned m) {
  unsigned c = 0;
  for (int j = 0; j < BITS; ++j) c += (unsigned)__popcll(__ballot((m >> j) & 1u));
  return c;
}

// then(the sum over the waves of a wave-uniform value), in thread 0 alone.  Holds a barrier.
template <int WAVES, typename Then>
__device__ __forceinline__ void block_total(unsigned of_wave, unsigned* s_wave, Then then) {
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = of_wave;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int w = 0; w < WAVES; ++w) t += s_wave[w];
    then(t);
  }
}

// the set bits among bits 0..BITS-1 of the masks of the lanes before this one in the workgroup: those of the waves before its
// own (LDS) + those of the lanes before it in its wave (mbcnt of the BITS ballots); < 64 WAVES BITS.  Holds a barrier.
template <int WAVES, int BITS>
__device__ __forceinline__ unsigned block_rank(unsigned m, unsigned* s_wave) {
  const int wave = threadIdx.x >> 6;
  unsigned in_wave = 0, lanes_before = 0;
  for (int j = 0; j < BITS; ++j) {
    const u64 b = __ballot((m >> j) & 1u);
    in_wave += (unsigned)__popcll(b);
    lanes_before += __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
  }
  if ((threadIdx.x & 63) == 0) s_wave[wave] = in_wave;
  __syncthreads();
  unsigned waves_before = 0;
  for (int w = 0; w < WAVES; ++w)
    if (w < wave) waves_before += s_wave[w];
  return waves_before + lanes_before;
}

// The sum of v over the lanes of the workgroup up to and including this one; *total = the sum over all of them, the same in
// every lane.  Holds a barrier after its store to s_wave: a caller that comes again puts one before that.
template <int WAVES, typename T>
__device__ __forceinline__ T block_scan(T v, T* s_wave, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  T before = 0, all = 0;
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave) before += s_wave[w];
    all += s_wave[w];
  }
  *total = all;
  return before + inc;
}

// The whole of launch 2 of ubr_scan_plan.h, for ONE workgroup of 64 WAVES lanes: an exclusive scan of the `blocks` block counts
// in place, four per lane and 256 WAVES per trip; count[0] = total.  Holds two barriers per trip.
template <int WAVES>
__device__ __forceinline__ void scan_block_counts(unsigned* __restrict__ scratch, long blocks, long trips, u64* __restrict__ count,
                                                  unsigned* s_wave) {
  unsigned carry = 0;
  for (long t = 0; t < trips; ++t) {
    const long i0 = t * (256 * WAVES) + (long)threadIdx.x * 4;
    uint4 c = make_uint4(0u, 0u, 0u, 0u);
    if (i0 < blocks) {                                         // i0 + 3 < scratch_words: the plan rounds the words up to four
      c = *(const uint4*)(scratch + i0);
      if (i0 + 1 >= blocks) c.y = 0u;                          // the words past the last block were never written
      if (i0 + 2 >= blocks) c.z = 0u;
      if (i0 + 3 >= blocks) c.w = 0u;
    }
    const unsigned sum = c.x + c.y + c.z + c.w;
    unsigned total;
    const unsigned ex = carry + block_scan<WAVES>(sum, s_wave, &total) - sum;
    if (i0 < blocks) *(uint4*)(scratch + i0) = make_uint4(ex, ex + c.x, ex + c.x + c.y, ex + c.x + c.y + c.z);
    carry += total;
    __syncthreads();                                           // s_wave is written again in the next trip
  }
  if (threadIdx.x == 0) count[0] = (u64)carry;
}

}  // namespace wv

#endif
