// libubresnet_tta.so: flip test-time augmentation of inference (include/ubresnet_tta.h).  It links against none of the
// other libraries and shares ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/ubresnet_tta.h"
#include "ubr_sat.h"

#define UBT_VERSION 1
#define UBT_TRIP (UBT_BLOCK * UBT_UNROLL)

SAT_RETURN_CODES(UBT);
SAT_EXPORTS(ubt, UBT_VERSION)
using namespace sat;

namespace {

// a unit: four floats of a row (vector path) or one (scalar path), handled as integers wherever no value is looked at
template <bool VEC> struct unit_of { typedef unsigned type; };
template <> struct unit_of<true> { typedef uint4 type; };

__device__ __forceinline__ unsigned zero_unit(unsigned) { return 0u; }
__device__ __forceinline__ uint4 zero_unit(uint4) { return make_uint4(0u, 0u, 0u, 0u); }
// the column flip inside a unit
__device__ __forceinline__ unsigned reversed(unsigned v) { return v; }
__device__ __forceinline__ uint4 reversed(uint4 v) { return make_uint4(v.w, v.z, v.y, v.x); }

// log(exp(a) + exp(b)) by the rules of the header.  The four steps of the last line are separate fp32 operations.
__device__ __forceinline__ float lae(float a, float b) {
  if (a != a || b != b) return a + b;
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  if (lo == -INFINITY) return hi;
  if (hi == lo) return __fadd_rn(hi, (float)M_LN2);
  return __fadd_rn(hi, log1pf(expf(__fsub_rn(lo, hi))));
}

__device__ __forceinline__ unsigned merged(unsigned acc, unsigned view, int last, float log_k) {
  const float v = lae(__uint_as_float(acc), __uint_as_float(view));
  return __float_as_uint(last ? __fsub_rn(v, log_k) : v);
}
__device__ __forceinline__ uint4 merged(uint4 acc, uint4 view, int last, float log_k) {
  return make_uint4(merged(acc.x, view.x, last, log_k), merged(acc.y, view.y, last, log_k), merged(acc.z, view.z, last, log_k),
                    merged(acc.w, view.w, last, log_k));
}

// Destination unit i = (row r of all nplanes * H rows, unit x of the WU units of a row) -> the source unit the flip reads.  The
// dividends are below 2^32 at every size the network runs, where the compiler's 64-bit division takes its 32-bit branch.
template <int FLIP>
__device__ __forceinline__ long source_unit(long i, int H, int WU) {
  if (FLIP == 0) return i;
  const long r = i / WU;
  const int x = (int)(i - r * WU);
  long sr = r;
  if (FLIP & UBT_FLIP_ROWS) sr = r + (H - 1 - 2 * (int)(r % H));       // same plane, row H - 1 - y
  return sr * WU + ((FLIP & UBT_FLIP_COLS) ? WU - 1 - x : x);
}

// The one kernel of the library.  MERGE = false: dst <- flipped src (ubt_flip_planes, and view 0 of a merge).  MERGE = true:
// dst <- lae(dst, flipped src), less log_k when `last`.  The walk is ubr_accum.hip's: a workgroup's trip is UBT_TRIP CONSECUTIVE
// destination units, unit t * UBT_TRIP + u * UBT_BLOCK + lane for u < UBT_UNROLL; workgroup g takes the trips g, g + grid, ..;
// the loads of a trip are issued before any is used.  A column flip reads a row's units in descending order, so a wave's load is
// still one contiguous piece.  Every index is checked against nunits: the last trip may be partly filled.
template <int FLIP, bool VEC, bool MERGE>
__global__ __launch_bounds__(UBT_BLOCK) void tta_kernel(const typename unit_of<VEC>::type* __restrict__ src,
                                                        typename unit_of<VEC>::type* __restrict__ dst, long nunits, int H, int WU,
                                                        int last, float log_k) {
  typedef typename unit_of<VEC>::type U;
  const long trips = (nunits + UBT_TRIP - 1) / UBT_TRIP;
  for (long t = blockIdx.x; t < trips; t += gridDim.x) {
    const long base = t * UBT_TRIP + threadIdx.x;
    U S[UBT_UNROLL], A[UBT_UNROLL];
#pragma unroll
    for (int u = 0; u < UBT_UNROLL; ++u) {
      const long i = base + u * UBT_BLOCK;
      S[u] = i < nunits ? src[source_unit<FLIP>(i, H, WU)] : zero_unit(U());
      if (MERGE) A[u] = i < nunits ? dst[i] : zero_unit(U());
    }
#pragma unroll
    for (int u = 0; u < UBT_UNROLL; ++u) {
      const long i = base + u * UBT_BLOCK;
      if (i >= nunits) continue;
      const U s = (FLIP & UBT_FLIP_COLS) ? reversed(S[u]) : S[u];
      dst[i] = MERGE ? merged(A[u], s, last, log_k) : s;
    }
  }
}

template <int FLIP, bool MERGE>
void launch(const float* src, float* dst, long rows, int H, int W, int last, float log_k, hipStream_t stream) {
  const bool vec = W % 4 == 0 && aligned(src, 16) && aligned(dst, 16);
  const int WU = vec ? W / 4 : W;
  const long nunits = rows * WU;
  const long trips = (nunits + UBT_TRIP - 1) / UBT_TRIP;
  const dim3 grid((unsigned)(trips > UBT_MAX_GRID ? UBT_MAX_GRID : trips)), block(UBT_BLOCK);
  if (vec)
    tta_kernel<FLIP, true, MERGE><<<grid, block, 0, stream>>>((const uint4*)src, (uint4*)dst, nunits, H, WU, last, log_k);
  else
    tta_kernel<FLIP, false, MERGE><<<grid, block, 0, stream>>>((const unsigned*)src, (unsigned*)dst, nunits, H, WU, last, log_k);
}

template <bool MERGE>
void launch_flip(const float* src, float* dst, long rows, int H, int W, int flip, int last, float log_k, hipStream_t stream) {
  switch (flip) {
    case 0: launch<0, MERGE>(src, dst, rows, H, W, last, log_k, stream); break;
    case 1: launch<1, MERGE>(src, dst, rows, H, W, last, log_k, stream); break;
    case 2: launch<2, MERGE>(src, dst, rows, H, W, last, log_k, stream); break;
    default: launch<3, MERGE>(src, dst, rows, H, W, last, log_k, stream); break;
  }
}

}  // namespace

// the checks the two calls share; `name` starts the message, a / b are the argument names of the two buffers
#define UBT_CHECK_PLANES(name, a, b, src, dst, nplanes, H, W, flip)                                                          \
  SAT_CHECK((src) && (dst), name ": null pointer (" a ", " b ")");                                                          \
  SAT_CHECK((nplanes) > 0 && (H) > 0 && (W) > 0, name ": nplanes=%lld, H=%d, W=%d must be positive", (long long)(nplanes), \
            (int)(H), (int)(W));                                                                                            \
  SAT_CHECK((nplanes) <= (int64_t)(1ll << 40) / (H) / (W), name ": nplanes=%lld x H=%d x W=%d exceeds 2^40 elements",       \
            (long long)(nplanes), (int)(H), (int)(W));                                                                      \
  SAT_CHECK((flip) >= 0 && (flip) <= 3, name ": flip=%d must be a mask of UBT_FLIP_ROWS | UBT_FLIP_COLS (0..3)", (int)(flip)); \
  SAT_CHECK(aligned((src), 4) && aligned((dst), 4), name ": " a " and " b " must be 4-byte aligned");                       \
  SAT_CHECK(!overlap((src), 4ull * (unsigned long long)((nplanes) * (H) * (W)), (dst),                                      \
                     4ull * (unsigned long long)((nplanes) * (H) * (W))), name ": " a " overlaps " b)

extern "C" int ubt_flip_planes(const float* src, float* dst, int64_t nplanes, int H, int W, int flip, void* stream) {
  UBT_CHECK_PLANES("ubt_flip_planes", "src", "dst", src, dst, nplanes, H, W, flip);
  launch_flip<false>(src, dst, (long)nplanes * H, H, W, flip, 0, 0.f, (hipStream_t)stream);
  SAT_LAUNCH_CHECK("ubt_flip_planes");
  return UBT_OK;
}

extern "C" int ubt_merge_view(const float* logp, float* acc, int64_t nplanes, int H, int W, int flip, int k, int K, float log_k,
                              void* stream) {
  UBT_CHECK_PLANES("ubt_merge_view", "logp", "acc", logp, acc, nplanes, H, W, flip);
  SAT_CHECK(K >= 1 && K <= UBT_MAX_VIEWS, "ubt_merge_view: K=%d must be in 1..%d (UBT_MAX_VIEWS)", K, UBT_MAX_VIEWS);
  SAT_CHECK(k >= 0 && k < K, "ubt_merge_view: k=%d must be in 0..K-1 (K=%d)", k, K);
  const int last = K > 1 && k == K - 1;
  SAT_CHECK(!last || (log_k == log_k && log_k > 0.f && log_k < INFINITY),
            "ubt_merge_view: log_k=%g must be finite and > 0 for the last of K=%d views", (double)log_k, K);
  if (k == 0)
    launch_flip<false>(logp, acc, (long)nplanes * H, H, W, flip, 0, 0.f, (hipStream_t)stream);
  else
    launch_flip<true>(logp, acc, (long)nplanes * H, H, W, flip, last, log_k, (hipStream_t)stream);
  SAT_LAUNCH_CHECK("ubt_merge_view");
  return UBT_OK;
}
