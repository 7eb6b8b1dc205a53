// libubresnet_ema.so: the exponential moving average of the parameters (include/ubresnet_ema.h).  It links against none of the
// other libraries and shares ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/ubresnet_ema.h"
#include "ubr_ema_sched.h"
#include "ubr_sat.h"

#define UBE_VERSION 1

static_assert(sizeof(ube_ctl) == UBE_CTL_BYTES, "ube_ctl layout");
static_assert(offsetof(ube_ctl, apply) == 0 && offsetof(ube_ctl, w) == 4 && offsetof(ube_ctl, d) == 8 &&
                  offsetof(ube_ctl, updates) == 16 && offsetof(ube_ctl, held) == 24,
              "ube_ctl layout");
static_assert(sizeof(ube_seg) == 32 && offsetof(ube_seg, live) == 8 && offsetof(ube_seg, count) == 16, "ube_seg layout");

SAT_RETURN_CODES(UBE);
SAT_EXPORTS(ube, UBE_VERSION)
using namespace sat;

namespace {

__global__ __launch_bounds__(64) void ctl_init_kernel(ube_ctl* ctl, long long updates) {
  if (threadIdx.x != 0) return;
  ctl->apply = 0;
  ctl->w = 0.f;
  ctl->d = 0.f;
  ctl->reserved = 0;
  ctl->updates = updates;
  ctl->held = 0;
}

// One lane decides: whether the optimizer's step was applied is on the device only, and so is the count the schedule needs.
__global__ __launch_bounds__(64) void advance_kernel(ube_ctl* __restrict__ ctl, const int32_t* __restrict__ flag, float decay,
                                                     long long warmup) {
  if (threadIdx.x != 0) return;
  const int apply = flag == nullptr ? 1 : (*flag != 0);
  if (apply) {
    const long long u = ctl->updates;
    const ube::Weight s = ube::schedule(decay, warmup, u);
    ctl->w = s.w;
    ctl->d = s.d;
    ctl->updates = u + 1;
    ctl->apply = 1;
  } else {
    ctl->held += 1;
    ctl->apply = 0;
  }
}

// s + w * (p - s): the three operations are intrinsics with a rounding mode, which the compiler neither contracts nor reorders
__device__ __forceinline__ float lerp1(float s, float p, float w) { return __fadd_rn(s, __fmul_rn(w, __fsub_rn(p, s))); }

// Lane `l` of the grid (l = block * UBE_BLOCK + thread) takes the units l + k * lanes, k = 0, 1, ..: consecutive lanes read
// consecutive 16-byte units.  The UBE_UNROLL units of a trip are loaded from both buffers before any is used, so a trip of the
// grid has grid * UBE_BLOCK * UBE_UNROLL * 32 bytes of loads in flight.
__global__ __launch_bounds__(UBE_BLOCK) void update_kernel(float4* __restrict__ s, const float4* __restrict__ p, long n4,
                                                           const ube_ctl* __restrict__ ctl) {
  if (ctl->apply == 0) return;
  const float w = ctl->w;
  const long lanes = (long)gridDim.x * UBE_BLOCK;
  for (long base = (long)blockIdx.x * UBE_BLOCK + threadIdx.x; base < n4; base += lanes * UBE_UNROLL) {
    float4 S[UBE_UNROLL], P[UBE_UNROLL];
#pragma unroll
    for (int u = 0; u < UBE_UNROLL; ++u) {
      const long i = base + u * lanes;
      P[u] = i < n4 ? p[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      S[u] = i < n4 ? s[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < UBE_UNROLL; ++u) {
      const long i = base + u * lanes;
      if (i < n4) s[i] = make_float4(lerp1(S[u].x, P[u].x, w), lerp1(S[u].y, P[u].y, w), lerp1(S[u].z, P[u].z, w), lerp1(S[u].w, P[u].w, w));
    }
  }
}

// The same walk with integer units: nothing of a value is looked at, so every bit pattern survives.
__global__ __launch_bounds__(UBE_BLOCK) void swap_kernel(uint4* __restrict__ a, uint4* __restrict__ b, long n4) {
  const long lanes = (long)gridDim.x * UBE_BLOCK;
  for (long base = (long)blockIdx.x * UBE_BLOCK + threadIdx.x; base < n4; base += lanes * UBE_UNROLL) {
    uint4 A[UBE_UNROLL], B[UBE_UNROLL];
#pragma unroll
    for (int u = 0; u < UBE_UNROLL; ++u) {
      const long i = base + u * lanes;
      A[u] = i < n4 ? a[i] : make_uint4(0u, 0u, 0u, 0u);
      B[u] = i < n4 ? b[i] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < UBE_UNROLL; ++u) {
      const long i = base + u * lanes;
      if (i < n4) {
        a[i] = B[u];
        b[i] = A[u];
      }
    }
  }
}

// Small tensors that are in no flat buffer: a workgroup per row (striding over the rows), its lanes striding over the row's
// values with 4-byte loads.  No alignment beyond a float's is assumed.
__global__ __launch_bounds__(UBE_BLOCK) void update_segs_kernel(const ube_seg* __restrict__ table, long nseg, const ube_ctl* __restrict__ ctl) {
  if (ctl->apply == 0) return;
  const float w = ctl->w;
  for (long g = blockIdx.x; g < nseg; g += gridDim.x) {
    const ube_seg row = table[g];
    float* s = reinterpret_cast<float*>(row.shadow);
    const float* p = reinterpret_cast<const float*>(row.live);
    if (s == nullptr || p == nullptr) continue;
    for (long i = threadIdx.x; i < row.count; i += UBE_BLOCK) s[i] = lerp1(s[i], p[i], w);
  }
}

__global__ __launch_bounds__(UBE_BLOCK) void swap_segs_kernel(const ube_seg* __restrict__ table, long nseg) {
  for (long g = blockIdx.x; g < nseg; g += gridDim.x) {
    const ube_seg row = table[g];
    uint32_t* a = reinterpret_cast<uint32_t*>(row.shadow);
    uint32_t* b = reinterpret_cast<uint32_t*>(row.live);
    if (a == nullptr || b == nullptr) continue;
    for (long i = threadIdx.x; i < row.count; i += UBE_BLOCK) {
      const uint32_t x = a[i], y = b[i];
      a[i] = y;
      b[i] = x;
    }
  }
}

inline unsigned flat_grid(long n4) {
  long grid = (n4 + UBE_BLOCK * UBE_UNROLL - 1) / (UBE_BLOCK * UBE_UNROLL);
  return (unsigned)(grid > UBE_MAX_GRID ? UBE_MAX_GRID : grid);
}

inline unsigned seg_grid(int64_t nseg) { return (unsigned)(nseg > UBE_SEG_GRID ? UBE_SEG_GRID : nseg); }

}  // namespace

extern "C" int ube_ctl_init(void* ctl, int64_t updates, void* stream) {
  SAT_CHECK(ctl, "ube_ctl_init: null ctl");
  SAT_CHECK(aligned(ctl, 16), "ube_ctl_init: ctl must be 16-byte aligned");
  SAT_CHECK(updates >= 0, "ube_ctl_init: updates=%lld must be >= 0", (long long)updates);
  ctl_init_kernel<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>((ube_ctl*)ctl, (long long)updates);
  SAT_LAUNCH_CHECK("ube_ctl_init");
  return UBE_OK;
}

extern "C" int ube_advance(void* ctl, const int32_t* apply_flag, float decay, int64_t warmup, void* stream) {
  SAT_CHECK(ctl, "ube_advance: null ctl");
  SAT_CHECK(aligned(ctl, 16), "ube_advance: ctl must be 16-byte aligned");
  SAT_CHECK(aligned(apply_flag, 4), "ube_advance: apply_flag must be 4-byte aligned");
  SAT_CHECK(!overlap(ctl, UBE_CTL_BYTES, apply_flag, 4), "ube_advance: apply_flag lies inside ctl");
  SAT_CHECK(decay == decay, "ube_advance: decay is NaN");
  SAT_CHECK(decay >= 0.f && decay < 1.f, "ube_advance: decay=%g must lie in [0, 1)", (double)decay);
  SAT_CHECK(warmup >= 0 && warmup <= (INT64_MAX >> 2), "ube_advance: warmup=%lld must be >= 0", (long long)warmup);
  advance_kernel<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>((ube_ctl*)ctl, apply_flag, decay, (long long)warmup);
  SAT_LAUNCH_CHECK("ube_advance");
  return UBE_OK;
}

extern "C" int ube_update(float* shadow, const float* param, int64_t n, const void* ctl, void* stream) {
  SAT_CHECK(shadow && param && ctl, "ube_update: null pointer (shadow, param, ctl)");
  SAT_CHECK(n > 0 && n % 4 == 0, "ube_update: n=%lld must be positive and a multiple of 4", (long long)n);
  SAT_CHECK(aligned(shadow, 16) && aligned(param, 16) && aligned(ctl, 16), "ube_update: shadow, param and ctl must be 16-byte aligned");
  const unsigned long long bytes = 4ull * (unsigned long long)n;
  SAT_CHECK(!overlap(shadow, bytes, param, bytes), "ube_update: shadow overlaps param");
  SAT_CHECK(!overlap(ctl, UBE_CTL_BYTES, shadow, bytes), "ube_update: ctl overlaps shadow");
  SAT_CHECK(!overlap(ctl, UBE_CTL_BYTES, param, bytes), "ube_update: ctl overlaps param");
  const long n4 = (long)(n / 4);
  update_kernel<<<dim3(flat_grid(n4)), dim3(UBE_BLOCK), 0, (hipStream_t)stream>>>((float4*)shadow, (const float4*)param, n4,
                                                                                 (const ube_ctl*)ctl);
  SAT_LAUNCH_CHECK("ube_update");
  return UBE_OK;
}

extern "C" int ube_swap(float* a, float* b, int64_t n, void* stream) {
  SAT_CHECK(a && b, "ube_swap: null pointer (a, b)");
  SAT_CHECK(n > 0 && n % 4 == 0, "ube_swap: n=%lld must be positive and a multiple of 4", (long long)n);
  SAT_CHECK(aligned(a, 16) && aligned(b, 16), "ube_swap: a and b must be 16-byte aligned");
  const unsigned long long bytes = 4ull * (unsigned long long)n;
  SAT_CHECK(!overlap(a, bytes, b, bytes), "ube_swap: a overlaps b");
  const long n4 = (long)(n / 4);
  swap_kernel<<<dim3(flat_grid(n4)), dim3(UBE_BLOCK), 0, (hipStream_t)stream>>>((uint4*)a, (uint4*)b, n4);
  SAT_LAUNCH_CHECK("ube_swap");
  return UBE_OK;
}

extern "C" int ube_update_segs(const void* table, int64_t nseg, const void* ctl, void* stream) {
  SAT_CHECK(table && ctl, "ube_update_segs: null pointer (table, ctl)");
  SAT_CHECK(nseg >= 1 && nseg <= (INT64_MAX >> 6), "ube_update_segs: nseg=%lld must be >= 1", (long long)nseg);
  SAT_CHECK(aligned(table, 8) && aligned(ctl, 16), "ube_update_segs: table must be 8-byte and ctl 16-byte aligned");
  SAT_CHECK(!overlap(ctl, UBE_CTL_BYTES, table, 32ull * (unsigned long long)nseg), "ube_update_segs: ctl overlaps table");
  update_segs_kernel<<<dim3(seg_grid(nseg)), dim3(UBE_BLOCK), 0, (hipStream_t)stream>>>((const ube_seg*)table, (long)nseg,
                                                                                       (const ube_ctl*)ctl);
  SAT_LAUNCH_CHECK("ube_update_segs");
  return UBE_OK;
}

extern "C" int ube_swap_segs(const void* table, int64_t nseg, void* stream) {
  SAT_CHECK(table, "ube_swap_segs: null pointer (table)");
  SAT_CHECK(nseg >= 1 && nseg <= (INT64_MAX >> 6), "ube_swap_segs: nseg=%lld must be >= 1", (long long)nseg);
  SAT_CHECK(aligned(table, 8), "ube_swap_segs: table must be 8-byte aligned");
  swap_segs_kernel<<<dim3(seg_grid(nseg)), dim3(UBE_BLOCK), 0, (hipStream_t)stream>>>((const ube_seg*)table, (long)nseg);
  SAT_LAUNCH_CHECK("ube_swap_segs");
  return UBE_OK;
}
