// libubresnet_accum.so: gradient accumulation over the flat gradient buffer (include/ubresnet_accum.h).  It links against none of
// the other libraries and shares ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/ubresnet_accum.h"
#include "ubr_sat.h"

#define UBC_VERSION 1
#define UBC_TRIP (UBC_BLOCK * UBC_UNROLL)

SAT_RETURN_CODES(UBC);
SAT_EXPORTS(ubc, UBC_VERSION)
using namespace sat;

namespace {

// The walk of all three kernels.  A workgroup's trip is UBC_TRIP CONSECUTIVE units: unit t * UBC_TRIP + u * UBC_BLOCK + lane for
// u < UBC_UNROLL, so a wave's load is 1 KiB in one piece, the workgroup's UBC_UNROLL loads of a buffer are 16 KiB in one piece,
// and the workgroups resident at one time read neighbouring pieces.  (update_kernel of ubr_ema.hip puts a lane's UBC_UNROLL units
// grid * UBC_BLOCK units apart -- 4 MiB at the grid cap, a power of two -- so that every workgroup has four streams that far
// apart open in each buffer.)  Workgroup g takes the trips g, g + grid, ..; the UBC_UNROLL units of a trip are loaded from both
// buffers before any is used, so a resident workgroup has 32 KiB of loads in flight.  Every index is checked against n4: the
// last trip may be partly filled.
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}

__device__ __forceinline__ float4 scale4(float4 a, float s) {
  return make_float4(__fmul_rn(a.x, s), __fmul_rn(a.y, s), __fmul_rn(a.z, s), __fmul_rn(a.w, s));
}

// integer units: nothing of a value is looked at, so every bit pattern survives
__global__ __launch_bounds__(UBC_BLOCK) void set_kernel(uint4* __restrict__ acc, const uint4* __restrict__ grad, long n4) {
  const long trips = (n4 + UBC_TRIP - 1) / UBC_TRIP;
  for (long t = blockIdx.x; t < trips; t += gridDim.x) {
    const long base = t * UBC_TRIP + threadIdx.x;
    uint4 G[UBC_UNROLL];
#pragma unroll
    for (int u = 0; u < UBC_UNROLL; ++u) {
      const long i = base + u * UBC_BLOCK;
      G[u] = i < n4 ? grad[i] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < UBC_UNROLL; ++u) {
      const long i = base + u * UBC_BLOCK;
      if (i < n4) acc[i] = G[u];
    }
  }
}

__global__ __launch_bounds__(UBC_BLOCK) void add_kernel(float4* __restrict__ acc, const float4* __restrict__ grad, long n4) {
  const long trips = (n4 + UBC_TRIP - 1) / UBC_TRIP;
  for (long t = blockIdx.x; t < trips; t += gridDim.x) {
    const long base = t * UBC_TRIP + threadIdx.x;
    float4 A[UBC_UNROLL], G[UBC_UNROLL];
#pragma unroll
    for (int u = 0; u < UBC_UNROLL; ++u) {
      const long i = base + u * UBC_BLOCK;
      G[u] = i < n4 ? grad[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      A[u] = i < n4 ? acc[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < UBC_UNROLL; ++u) {
      const long i = base + u * UBC_BLOCK;
      if (i < n4) acc[i] = add4(A[u], G[u]);
    }
  }
}

__global__ __launch_bounds__(UBC_BLOCK) void finish_kernel(float4* __restrict__ grad, const float4* __restrict__ acc, long n4, float scale) {
  const long trips = (n4 + UBC_TRIP - 1) / UBC_TRIP;
  for (long t = blockIdx.x; t < trips; t += gridDim.x) {
    const long base = t * UBC_TRIP + threadIdx.x;
    float4 A[UBC_UNROLL], G[UBC_UNROLL];
#pragma unroll
    for (int u = 0; u < UBC_UNROLL; ++u) {
      const long i = base + u * UBC_BLOCK;
      A[u] = i < n4 ? acc[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      G[u] = i < n4 ? grad[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < UBC_UNROLL; ++u) {
      const long i = base + u * UBC_BLOCK;
      if (i < n4) grad[i] = scale4(add4(A[u], G[u]), scale);
    }
  }
}

inline unsigned flat_grid(long n4) {
  long grid = (n4 + UBC_TRIP - 1) / UBC_TRIP;
  return (unsigned)(grid > UBC_MAX_GRID ? UBC_MAX_GRID : grid);
}

}  // namespace

// the checks the three calls share; `name` starts the message
#define UBC_CHECK_PAIR(name, acc, grad, n)                                                                                    \
  SAT_CHECK((acc) && (grad), name ": null pointer (acc, grad)");                                                             \
  SAT_CHECK((n) > 0 && (n) % 4 == 0, name ": n=%lld must be positive and a multiple of 4", (long long)(n));                  \
  SAT_CHECK(aligned((acc), 16) && aligned((grad), 16), name ": acc and grad must be 16-byte aligned");                       \
  SAT_CHECK(!overlap((acc), 4ull * (unsigned long long)(n), (grad), 4ull * (unsigned long long)(n)), name ": acc overlaps grad")

extern "C" int ubc_set(float* acc, const float* grad, int64_t n, void* stream) {
  UBC_CHECK_PAIR("ubc_set", acc, grad, n);
  const long n4 = (long)(n / 4);
  set_kernel<<<dim3(flat_grid(n4)), dim3(UBC_BLOCK), 0, (hipStream_t)stream>>>((uint4*)acc, (const uint4*)grad, n4);
  SAT_LAUNCH_CHECK("ubc_set");
  return UBC_OK;
}

extern "C" int ubc_add(float* acc, const float* grad, int64_t n, void* stream) {
  UBC_CHECK_PAIR("ubc_add", acc, grad, n);
  const long n4 = (long)(n / 4);
  add_kernel<<<dim3(flat_grid(n4)), dim3(UBC_BLOCK), 0, (hipStream_t)stream>>>((float4*)acc, (const float4*)grad, n4);
  SAT_LAUNCH_CHECK("ubc_add");
  return UBC_OK;
}

extern "C" int ubc_finish(float* grad, const float* acc, int64_t n, float scale, void* stream) {
  UBC_CHECK_PAIR("ubc_finish", acc, grad, n);
  SAT_CHECK(scale == scale, "ubc_finish: scale is NaN");
  SAT_CHECK(scale > 0.f && scale < INFINITY, "ubc_finish: scale=%g must be finite and > 0", (double)scale);
  const long n4 = (long)(n / 4);
  finish_kernel<<<dim3(flat_grid(n4)), dim3(UBC_BLOCK), 0, (hipStream_t)stream>>>((float4*)grad, (const float4*)acc, n4, scale);
  SAT_LAUNCH_CHECK("ubc_finish");
  return UBC_OK;
}
