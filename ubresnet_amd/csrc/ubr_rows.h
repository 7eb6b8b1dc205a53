// The fixed-order sums of libubresnet_loss.so and libubresnet_dice.so (ubr_loss.hip, ubr_dice.hip): a streaming pass leaves one
// row of 64-bit words per workgroup, fp64 sums and integer counts side by side, and one workgroup adds the rows.  The order of
// the additions is part of those libraries' contract -- the same rows give the same bits -- so what is here is what the two
// sources add in the same order.  Device code only.  No other header of the project is included here.
#ifndef UBR_ROWS_H
#define UBR_ROWS_H

#include <hip/hip_runtime.h>

namespace rowsum {

typedef long long ll2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

// the lanes of a wave in the fixed order of the shuffle tree; lane 0 holds the sum
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// a target that is a class and is not the ignored one
__device__ __forceinline__ bool contributes(long long t, int C, long long ignore_index) {
  return t != ignore_index && t >= 0 && t < C;
}

// word `word` of a workgroup's row: the WAVES rows of its waves in order, as integers or as fp64
template <int WAVES, int WORDS>
__device__ __forceinline__ u64 add_wave_rows(const u64 (&wave_row)[WAVES][WORDS], int word, bool integer) {
  u64 out;
  if (integer) {
    out = 0ull;
    for (int w = 0; w < WAVES; ++w) out += wave_row[w][word];
  } else {
    double d = 0.0;
    for (int w = 0; w < WAVES; ++w) d += __longlong_as_double((long long)wave_row[w][word]);
    out = (u64)__double_as_longlong(d);
  }
  return out;
}

// The finish kernels' sum of `nrows` rows in two levels.  First lane (q, word), q < SUB, adds word `word` of the rows q,
// q + SUB, q + 2 SUB, .. in that order (sequence_sum); after a barrier lane `word` adds the SUB sequences in order
// (sequences_sum).  The kernels keep the LDS array between the two, the barrier and their guards.
template <int SUB, int WORDS>
__device__ __forceinline__ u64 sequence_sum(const u64* __restrict__ rows, int nrows, int q, int word, bool integer) {
  u64 ai = 0ull;
  double ad = 0.0;
#pragma unroll 8
  for (int r = q; r < nrows; r += SUB) {
    const u64 v = rows[(long)r * WORDS + word];
    ai += integer ? v : 0ull;
    ad += integer ? 0.0 : __longlong_as_double((long long)v);
  }
  return integer ? ai : (u64)__double_as_longlong(ad);
}

template <int SUB, int WORDS>
__device__ __forceinline__ u64 sequences_sum(const u64 (&sub)[SUB][WORDS], int word, bool integer) {
  u64 ai = 0ull;
  double ad = 0.0;
  for (int k = 0; k < SUB; ++k) {
    const u64 v = sub[k][word];
    ai += integer ? v : 0ull;
    ad += integer ? 0.0 : __longlong_as_double((long long)v);
  }
  return integer ? ai : (u64)__double_as_longlong(ad);
}

}  // namespace rowsum

#endif
