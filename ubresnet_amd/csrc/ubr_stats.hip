// libubresnet_stats.so: the guard of the BatchNorm running statistics (include/ubresnet_stats.h).  It links against
// none of the other libraries and shares ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/ubresnet_stats.h"
#include "ubr_stats_decide.h"
#include "ubr_sat.h"

#define UBS_VERSION 1

static_assert(sizeof(ubs_ctl) == UBS_CTL_BYTES, "ubs_ctl layout");
static_assert(offsetof(ubs_ctl, keep) == 0 && offsetof(ubs_ctl, bad_rows) == 4 && offsetof(ubs_ctl, kept) == 8 &&
                  offsetof(ubs_ctl, restored) == 16 && offsetof(ubs_ctl, restored_for_stats) == 24,
              "ubs_ctl layout");
static_assert(sizeof(ubs_seg) == 32 && offsetof(ubs_seg, live) == 8 && offsetof(ubs_seg, count) == 16 && offsetof(ubs_seg, kind) == 24,
              "ubs_seg layout");
static_assert((UBS_BLOCK & (UBS_BLOCK - 1)) == 0, "the local-memory reduction halves UBS_BLOCK");

SAT_RETURN_CODES(UBS);
SAT_EXPORTS(ubs, UBS_VERSION)
using namespace sat;

namespace {

__global__ __launch_bounds__(64) void ctl_init_kernel(ubs_ctl* ctl) {
  if (threadIdx.x != 0) return;
  ctl->keep = 0;
  ctl->bad_rows = 0;
  ctl->kept = 0;
  ctl->restored = 0;
  ctl->restored_for_stats = 0;
}

// The sum of `mine` over the workgroup, in every lane.  Integer adds: any order gives the same sum.  Every lane of the
// workgroup calls it (the callers' loops are uniform over the workgroup).
__device__ __forceinline__ unsigned long long block_sum(unsigned long long mine, unsigned long long* part) {
  part[threadIdx.x] = mine;
  __syncthreads();
  for (int s = UBS_BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  const unsigned long long total = part[0];
  __syncthreads();                          // part is written again by the next row
  return total;
}

// A workgroup per row (striding over the rows), its lanes striding over the row's units with 4-byte loads.  The exponent field
// of an fp32 is bits 23..30: all ones is an infinity or a NaN.
__global__ __launch_bounds__(UBS_BLOCK) void scan_kernel(const ubs_seg* __restrict__ table, long nseg, int32_t* __restrict__ bad) {
  __shared__ unsigned long long part[UBS_BLOCK];
  for (long g = blockIdx.x; g < nseg; g += gridDim.x) {
    const ubs_seg row = table[g];
    const uint32_t* p = reinterpret_cast<const uint32_t*>(row.live);
    unsigned long long mine = 0;
    if (row.kind == UBS_KIND_F32 && p != nullptr)
      for (long i = threadIdx.x; i < row.count; i += UBS_BLOCK) mine += (p[i] & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    const unsigned long long total = block_sum(mine, part);
    if (threadIdx.x == 0) bad[g] = (int32_t)(total > 0x7fffffffull ? 0x7fffffffull : total);
  }
}

__global__ __launch_bounds__(UBS_BLOCK) void note_kernel(int32_t* __restrict__ seen, const int32_t* __restrict__ bad, long nseg) {
  for (long r = threadIdx.x; r < nseg; r += UBS_BLOCK) {
    const int32_t b = bad[r];
    if (b > 0) {
      const long long s = (long long)seen[r] + b;
      seen[r] = (int32_t)(s > 0x7fffffffll ? 0x7fffffffll : s);
    }
  }
}

// One workgroup counts the rows, one lane decides: whether the optimizer's step was applied is on the device only.
__global__ __launch_bounds__(UBS_BLOCK) void decide_kernel(ubs_ctl* __restrict__ ctl, const int32_t* __restrict__ bad, long nseg,
                                                           const int32_t* __restrict__ flag, int32_t check) {
  __shared__ unsigned long long part[UBS_BLOCK];
  unsigned long long mine = 0;
  for (long r = threadIdx.x; r < nseg; r += UBS_BLOCK) mine += bad[r] != 0 ? 1u : 0u;
  const unsigned long long total = block_sum(mine, part);
  if (threadIdx.x != 0) return;
  const int32_t bad_rows = (int32_t)(total > 0x7fffffffull ? 0x7fffffffull : total);
  const ubs::Verdict v = ubs::decide(flag != nullptr, flag != nullptr ? *flag : 1, check, bad_rows);
  ubs::record(ctl, v, bad_rows);
}

// Nothing of a value is looked at: 32-bit integer units in one direction or the other.
__global__ __launch_bounds__(UBS_BLOCK) void resolve_kernel(const ubs_seg* __restrict__ table, long nseg, const ubs_ctl* __restrict__ ctl) {
  const bool keep = ctl->keep != 0;
  for (long g = blockIdx.x; g < nseg; g += gridDim.x) {
    const ubs_seg row = table[g];
    uint32_t* s = reinterpret_cast<uint32_t*>(row.shadow);
    uint32_t* l = reinterpret_cast<uint32_t*>(row.live);
    if (s == nullptr || l == nullptr) continue;
    uint32_t* dst = keep ? s : l;
    const uint32_t* src = keep ? l : s;
    for (long i = threadIdx.x; i < row.count; i += UBS_BLOCK) dst[i] = src[i];
  }
}

inline unsigned seg_grid(int64_t nseg) { return (unsigned)(nseg > UBS_SEG_GRID ? UBS_SEG_GRID : nseg); }

}  // namespace

extern "C" int ubs_ctl_init(void* ctl, void* stream) {
  SAT_CHECK(ctl, "ubs_ctl_init: null ctl");
  SAT_CHECK(aligned(ctl, 16), "ubs_ctl_init: ctl must be 16-byte aligned");
  ctl_init_kernel<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>((ubs_ctl*)ctl);
  SAT_LAUNCH_CHECK("ubs_ctl_init");
  return UBS_OK;
}

extern "C" int ubs_scan(const void* table, int64_t nseg, int32_t* bad, void* stream) {
  SAT_CHECK(table && bad, "ubs_scan: null pointer (table, bad)");
  SAT_CHECK(nseg >= 1 && nseg <= (INT64_MAX >> 6), "ubs_scan: nseg=%lld must be >= 1", (long long)nseg);
  SAT_CHECK(aligned(table, 8) && aligned(bad, 4), "ubs_scan: table must be 8-byte and bad 4-byte aligned");
  SAT_CHECK(!overlap(bad, 4ull * (unsigned long long)nseg, table, 32ull * (unsigned long long)nseg), "ubs_scan: bad overlaps table");
  scan_kernel<<<dim3(seg_grid(nseg)), dim3(UBS_BLOCK), 0, (hipStream_t)stream>>>((const ubs_seg*)table, (long)nseg, bad);
  SAT_LAUNCH_CHECK("ubs_scan");
  return UBS_OK;
}

extern "C" int ubs_note(int32_t* seen, const int32_t* bad, int64_t nseg, void* stream) {
  SAT_CHECK(seen && bad, "ubs_note: null pointer (seen, bad)");
  SAT_CHECK(nseg >= 1 && nseg <= (INT64_MAX >> 6), "ubs_note: nseg=%lld must be >= 1", (long long)nseg);
  SAT_CHECK(aligned(seen, 4) && aligned(bad, 4), "ubs_note: seen and bad must be 4-byte aligned");
  SAT_CHECK(!overlap(seen, 4ull * (unsigned long long)nseg, bad, 4ull * (unsigned long long)nseg), "ubs_note: seen overlaps bad");
  note_kernel<<<dim3(1), dim3(UBS_BLOCK), 0, (hipStream_t)stream>>>(seen, bad, (long)nseg);
  SAT_LAUNCH_CHECK("ubs_note");
  return UBS_OK;
}

extern "C" int ubs_decide(void* ctl, const int32_t* bad, int64_t nseg, const int32_t* apply_flag, int32_t check, void* stream) {
  SAT_CHECK(ctl && bad, "ubs_decide: null pointer (ctl, bad)");
  SAT_CHECK(nseg >= 1 && nseg <= (INT64_MAX >> 6), "ubs_decide: nseg=%lld must be >= 1", (long long)nseg);
  SAT_CHECK(aligned(ctl, 16), "ubs_decide: ctl must be 16-byte aligned");
  SAT_CHECK(aligned(bad, 4) && aligned(apply_flag, 4), "ubs_decide: bad and apply_flag must be 4-byte aligned");
  SAT_CHECK(!overlap(ctl, UBS_CTL_BYTES, apply_flag, 4), "ubs_decide: apply_flag lies inside ctl");
  SAT_CHECK(!overlap(ctl, UBS_CTL_BYTES, bad, 4ull * (unsigned long long)nseg), "ubs_decide: ctl overlaps bad");
  SAT_CHECK(!overlap(apply_flag, 4, bad, 4ull * (unsigned long long)nseg), "ubs_decide: apply_flag lies inside bad");
  decide_kernel<<<dim3(1), dim3(UBS_BLOCK), 0, (hipStream_t)stream>>>((ubs_ctl*)ctl, bad, (long)nseg, apply_flag, check);
  SAT_LAUNCH_CHECK("ubs_decide");
  return UBS_OK;
}

extern "C" int ubs_resolve(const void* table, int64_t nseg, const void* ctl, void* stream) {
  SAT_CHECK(table && ctl, "ubs_resolve: null pointer (table, ctl)");
  SAT_CHECK(nseg >= 1 && nseg <= (INT64_MAX >> 6), "ubs_resolve: nseg=%lld must be >= 1", (long long)nseg);
  SAT_CHECK(aligned(table, 8) && aligned(ctl, 16), "ubs_resolve: table must be 8-byte and ctl 16-byte aligned");
  SAT_CHECK(!overlap(ctl, UBS_CTL_BYTES, table, 32ull * (unsigned long long)nseg), "ubs_resolve: ctl overlaps table");
  resolve_kernel<<<dim3(seg_grid(nseg)), dim3(UBS_BLOCK), 0, (hipStream_t)stream>>>((const ubs_seg*)table, (long)nseg, (const ubs_ctl*)ctl);
  SAT_LAUNCH_CHECK("ubs_resolve");
  return UBS_OK;
}
