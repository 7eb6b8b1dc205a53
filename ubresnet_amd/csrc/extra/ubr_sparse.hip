// libubresnet_sparse.so: sparse event I/O (include/ubresnet_sparse.h).  It links against none of the other libraries and shares
// ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream.  Block sizes, grids and the scratch layout come
// from ../ubr_sparse_plan.h, which tests/sparse_host.cpp runs on the host; the workgroup count, rank and scan from ../ubr_wave.h.
#include <hip/hip_runtime.h>
#include "../../../include/ubresnet_sparse.h"
#include "../ubr_sat.h"
#include "../ubr_sparse_plan.h"
#include "../ubr_wave.h"

#define UBZ_VERSION 1

SAT_RETURN_CODES(UBZ);
SAT_EXPORTS(ubz, UBZ_VERSION)
using namespace sat;

static_assert(ubz::LANES == UBZ_LANES && ubz::LANE_PIXELS == UBZ_LANE_PIXELS && ubz::PIXEL_BLOCK == UBZ_PIXEL_BLOCK &&
                  ubz::SCAN_WIDTH == UBZ_SCAN_WIDTH && ubz::MAX_GRID == UBZ_MAX_GRID,
              "the plan is the geometry of the public header");
static_assert(ubz::LANE_PIXELS == 4 && ubz::SCAN_LANE_COUNTS == 4 && ubz::WAVE == 64, "the kernels unroll four pixels / counts per lane");

namespace {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------------------------------
// fill: two byte ranges, each set to one byte value -- 16-byte stores over the aligned body, byte stores over the < 16 bytes
// before and after it
// ---------------------------------------------------------------------------------------------------------------------------
struct fill_t {
  uint8_t* p;
  long head, units, tail;      // bytes before the first 16-byte boundary, 16-byte units, bytes after the last unit
  unsigned word;               // the byte, four times
};

fill_t make_fill(void* p, long nbytes, int byte) {
  fill_t f;
  f.p = (uint8_t*)p;
  f.head = (long)((16 - ((uintptr_t)p & 15)) & 15);
  if (f.head > nbytes) f.head = nbytes;
  f.units = (nbytes - f.head) / 16;
  f.tail = nbytes - f.head - 16 * f.units;
  f.word = 0x01010101u * (unsigned)(byte & 255);
  return f;
}

__global__ __launch_bounds__(UBZ_LANES) void fill_kernel(const fill_t a, const fill_t b) {
  const long units = a.units + b.units;
  for (long u = (long)blockIdx.x * UBZ_LANES + threadIdx.x; u < units; u += (long)gridDim.x * UBZ_LANES) {
    const bool first = u < a.units;
    uint4* dst = first ? (uint4*)(a.p + a.head) + u : (uint4*)(b.p + b.head) + (u - a.units);
    const unsigned w = first ? a.word : b.word;
    *dst = make_uint4(w, w, w, w);
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {                 // lanes 0..31: the edges of a, 32..63: of b
    const fill_t& f = threadIdx.x < 32 ? a : b;
    const long e = threadIdx.x & 15;
    if ((threadIdx.x & 16) == 0) {
      if (e < f.head) f.p[e] = (uint8_t)f.word;
    } else {
      if (e < f.tail) f.p[f.head + 16 * f.units + e] = (uint8_t)f.word;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// scatter of the valid entries.  EXPAND false: in0 = value (32-bit words), out0 = view; true: in0 = label (bytes), in1 =
// confidence, out0 = out_label, out1 = out_confidence.  Every lane loads its predecessor's index.  The invalid entries are
// counted by wave ballots; one atomic add per workgroup, if it met any.
// ---------------------------------------------------------------------------------------------------------------------------
template <bool EXPAND>
__global__ __launch_bounds__(UBZ_LANES) void scatter_kernel(const int32_t* __restrict__ index, const void* __restrict__ in0,
                                                            const uint16_t* __restrict__ in1, long n, const u64* __restrict__ count,
                                                            void* __restrict__ out0, uint16_t* __restrict__ out1, int pixels,
                                                            u64* status) {
  __shared__ unsigned s_bad[ubz::WAVES];
  long m = n;
  if (count) {
    const u64 c = *count;
    if (c < (u64)m) m = (long)c;
  }
  unsigned bad = 0;                                           // wave-uniform
  for (long base = (long)blockIdx.x * UBZ_LANES; base < m; base += (long)gridDim.x * UBZ_LANES) {
    const long i = base + threadIdx.x;
    bool invalid = false;
    if (i < m) {
      const int32_t idx = index[i];
      const bool valid = idx >= 0 && idx < pixels && (i == 0 || idx > index[i - 1]);
      if (valid) {
        if (EXPAND) {
          ((uint8_t*)out0)[idx] = ((const uint8_t*)in0)[i];
          out1[idx] = in1[i];
        } else {
          ((uint32_t*)out0)[idx] = ((const uint32_t*)in0)[i];
        }
      }
      invalid = !valid;
    }
    bad += wv::mask_count<1>(invalid);
  }
  wv::block_total<ubz::WAVES>(bad, s_bad, [status](unsigned t) {
    if (t) atomicAdd(status, (u64)t);
  });
}

// ---------------------------------------------------------------------------------------------------------------------------
// compaction
// ---------------------------------------------------------------------------------------------------------------------------
// THE lit predicate, of the count pass and of the write pass alike: bit j is set iff pixel q + j exists and is lit.  A pixel is
// lit iff adc is null or any of its vplanes values is > thr (NaN > thr is false).  rc = rows * cols.  The four pixels of a lane
// are loaded as 16 bytes where they lie in one plane and the address is aligned, one by one otherwise.
__device__ __forceinline__ unsigned lit_mask(const float* __restrict__ adc, int vplanes, float thr, unsigned q, unsigned pixels,
                                             unsigned rc) {
  if (q >= pixels) return 0u;
  const unsigned left = pixels - q;
  const unsigned cnt = left < 4u ? left : 4u;
  if (!adc) return (1u << cnt) - 1u;
  const unsigned p = q / rc, o = q - p * rc;
  unsigned m = 0u;
  if (cnt == 4u && o + 3u < rc) {
    for (int v = 0; v < vplanes; ++v) {
      const float* a = adc + ((size_t)p * vplanes + v) * rc + o;
      if (((uintptr_t)a & 15) == 0) {
        const float4 x = *(const float4*)a;
        m |= (unsigned)(x.x > thr) | (unsigned)(x.y > thr) << 1 | (unsigned)(x.z > thr) << 2 | (unsigned)(x.w > thr) << 3;
      } else {
        for (int j = 0; j < 4; ++j) m |= (unsigned)(a[j] > thr) << j;
      }
    }
  } else {
    for (unsigned j = 0; j < cnt; ++j) {
      const unsigned qq = q + j, pp = qq / rc, oo = qq - pp * rc;
      for (int v = 0; v < vplanes; ++v) m |= (unsigned)(adc[((size_t)pp * vplanes + v) * rc + oo] > thr) << j;
    }
  }
  return m;
}

// launch 1: one workgroup per pixel block; four ballots per wave, their 64-bit popcounts, one count per block
__global__ __launch_bounds__(UBZ_LANES) void count_kernel(const float* __restrict__ adc, int vplanes, float thr, unsigned pixels,
                                                          unsigned rc, unsigned* __restrict__ scratch) {
  __shared__ unsigned s_wave[ubz::WAVES];
  const unsigned q = blockIdx.x * (unsigned)UBZ_PIXEL_BLOCK + threadIdx.x * 4u;
  const unsigned m = lit_mask(adc, vplanes, thr, q, pixels, rc);
  wv::block_total<ubz::WAVES>(wv::mask_count<4>(m), s_wave, [scratch](unsigned t) { scratch[blockIdx.x] = t; });
}

// launch 2: ONE workgroup; an exclusive scan of the block counts in place, UBZ_SCAN_WIDTH per trip, four per lane; count[0] = total
__global__ __launch_bounds__(UBZ_LANES) void scan_kernel(unsigned* __restrict__ scratch, long blocks, long trips, u64* __restrict__ count) {
  __shared__ unsigned s_wave[ubz::WAVES];
  wv::scan_block_counts<ubz::WAVES>(scratch, blocks, trips, count, s_wave);
}

// launch 3: the same predicate again; a lit pixel's place is its block's offset + the lit pixels of the waves before its own
// and of the lanes before its own (wv::block_rank) + those before it in its lane
__global__ __launch_bounds__(UBZ_LANES) void write_kernel(const uint8_t* __restrict__ label, const uint16_t* __restrict__ confidence,
                                                          const float* __restrict__ adc, int vplanes, float thr, unsigned pixels,
                                                          unsigned rc, const unsigned* __restrict__ scratch, u64 capacity,
                                                          int32_t* __restrict__ out_index, uint8_t* __restrict__ out_label,
                                                          uint16_t* __restrict__ out_confidence) {
  __shared__ unsigned s_wave[ubz::WAVES];
  const unsigned q = blockIdx.x * (unsigned)UBZ_PIXEL_BLOCK + threadIdx.x * 4u;
  const unsigned m = lit_mask(adc, vplanes, thr, q, pixels, rc);
  const unsigned before = wv::block_rank<ubz::WAVES, 4>(m, s_wave);
  u64 k = (u64)scratch[blockIdx.x] + before;
  for (unsigned j = 0; j < 4u; ++j) {
    if (!((m >> j) & 1u)) continue;
    if (k < capacity) {
      out_index[k] = (int32_t)(q + j);
      out_label[k] = label[q + j];
      out_confidence[k] = confidence[q + j];
    }
    ++k;
  }
}

// the checks the scatter and the expand share; -> 0 or -1 with the message set
int check_list(const char* who, const void* index, const void* in0, const void* in1, bool two, int64_t n, const void* count,
               int P, int rows, int cols, const void* status, ubz::Plan* plan) {
  SAT_CHECK(n >= 0 && n <= ubz::MAX_PIXELS, "%s: n=%lld must be in 0..2^31-1", who, (long long)n);
  SAT_CHECK(n == 0 || (index && in0 && (!two || in1)), "%s: null pointer (an entry array with n > 0)", who);
  SAT_CHECK(status, "%s: null pointer (status)", who);
  SAT_CHECK(P >= 1 && rows >= 1 && cols >= 1, "%s: P=%d, rows=%d, cols=%d must be positive", who, P, rows, cols);
  SAT_CHECK(ubz::make_plan(P, rows, cols, plan), "%s: P=%d x rows=%d x cols=%d must be below 2^31 pixels (int32 pixel index)", who, P,
            rows, cols);
  SAT_CHECK(aligned(index, 4) && aligned(count, 8) && aligned(status, 8),
            "%s: index must be 4-byte aligned, count and status 8-byte aligned", who);
  return 0;
}

}  // namespace

extern "C" int ubz_scatter_view(const int32_t* index, const float* value, int64_t n, const unsigned long long* count, float* view,
                                int P, int rows, int cols, unsigned long long* status, void* stream) {
  ubz::Plan plan;
  if (check_list("ubz_scatter_view", index, value, nullptr, false, n, count, P, rows, cols, status, &plan)) return UBZ_EINVAL;
  SAT_CHECK(view, "ubz_scatter_view: null pointer (view)");
  SAT_CHECK(aligned(value, 4) && aligned(view, 4), "ubz_scatter_view: value and view must be 4-byte aligned");
  const u64 vbytes = 4ull * (u64)plan.pixels;
  SAT_CHECK(!overlap(index, 4ull * (u64)n, view, vbytes) && !overlap(value, 4ull * (u64)n, view, vbytes) &&
                !overlap(count, 8, view, vbytes) && !overlap(status, 8, view, vbytes),
            "ubz_scatter_view: view overlaps an input or status");
  const fill_t f = make_fill(view, (long)vbytes, 0), none = make_fill(nullptr, 0, 0);
  const int64_t fgrid = ubz::stride_grid(f.units);
  fill_kernel<<<dim3((unsigned)(fgrid < 1 ? 1 : fgrid)), dim3(UBZ_LANES), 0, (hipStream_t)stream>>>(f, none);
  SAT_LAUNCH_CHECK("ubz_scatter_view (fill)");
  if (n > 0) {
    scatter_kernel<false><<<dim3((unsigned)ubz::stride_grid(n)), dim3(UBZ_LANES), 0, (hipStream_t)stream>>>(
        index, value, nullptr, (long)n, count, view, nullptr, (int)plan.pixels, status);
    SAT_LAUNCH_CHECK("ubz_scatter_view (scatter)");
  }
  return UBZ_OK;
}

extern "C" int64_t ubz_compact_scratch_bytes(int P, int rows, int cols) {
  ubz::Plan plan;
  if (!ubz::make_plan(P, rows, cols, &plan)) {
    set_error("ubz_compact_scratch_bytes: P=%d, rows=%d, cols=%d must be positive and below 2^31 pixels", P, rows, cols);
    return 0;
  }
  return plan.scratch_bytes;
}

extern "C" int ubz_compact(const uint8_t* label, const uint16_t* confidence, const float* adc, int vplanes, float adc_threshold,
                           int P, int rows, int cols, int64_t capacity, int32_t* out_index, uint8_t* out_label,
                           uint16_t* out_confidence, unsigned long long* count, void* scratch, int64_t scratch_bytes, void* stream) {
  SAT_CHECK(label && confidence, "ubz_compact: null pointer (label, confidence)");
  SAT_CHECK(out_index && out_label && out_confidence && count, "ubz_compact: null pointer (out_index, out_label, out_confidence, count)");
  SAT_CHECK(scratch, "ubz_compact: null pointer (scratch)");
  SAT_CHECK(P >= 1 && rows >= 1 && cols >= 1, "ubz_compact: P=%d, rows=%d, cols=%d must be positive", P, rows, cols);
  ubz::Plan plan;
  SAT_CHECK(ubz::make_plan(P, rows, cols, &plan), "ubz_compact: P=%d x rows=%d x cols=%d must be below 2^31 pixels (int32 pixel index)",
            P, rows, cols);
  SAT_CHECK(!adc || (vplanes >= 1 && vplanes <= UBZ_MAX_VPLANES), "ubz_compact: vplanes=%d must be 1..%d", vplanes, UBZ_MAX_VPLANES);
  SAT_CHECK(capacity >= 1, "ubz_compact: capacity=%lld must be >= 1", (long long)capacity);
  SAT_CHECK(scratch_bytes >= plan.scratch_bytes, "ubz_compact: scratch_bytes=%lld is short of the %lld that ubz_compact_scratch_bytes gives",
            (long long)scratch_bytes, (long long)plan.scratch_bytes);
  SAT_CHECK(aligned(confidence, 2) && aligned(adc, 4) && aligned(out_index, 4) && aligned(out_confidence, 2) && aligned(count, 8),
            "ubz_compact: confidence / out_confidence must be 2-byte, adc / out_index 4-byte and count 8-byte aligned");
  SAT_CHECK(aligned16(scratch), "ubz_compact: scratch must be 16-byte aligned");
  const u64 px = (u64)plan.pixels, cap = (u64)capacity < px ? (u64)capacity : px;        // entries that can be written
  const void* outs[5] = {out_index, out_label, out_confidence, count, scratch};
  const u64 obytes[5] = {4 * cap, cap, 2 * cap, 8, (u64)plan.scratch_bytes};
  for (int i = 0; i < 5; ++i) {
    SAT_CHECK(!overlap(outs[i], obytes[i], label, px) && !overlap(outs[i], obytes[i], confidence, 2 * px) &&
                  !overlap(outs[i], obytes[i], adc, 4 * px * (u64)(adc ? vplanes : 0)),
              "ubz_compact: an output or scratch overlaps an input");
    for (int j = i + 1; j < 5; ++j) SAT_CHECK(!overlap(outs[i], obytes[i], outs[j], obytes[j]), "ubz_compact: two outputs overlap");
  }
  const unsigned pixels = (unsigned)plan.pixels, rc = (unsigned)rows * (unsigned)cols;
  const dim3 grid((unsigned)plan.blocks), block(UBZ_LANES);
  hipStream_t st = (hipStream_t)stream;
  count_kernel<<<grid, block, 0, st>>>(adc, vplanes, adc_threshold, pixels, rc, (unsigned*)scratch);
  SAT_LAUNCH_CHECK("ubz_compact (count)");
  scan_kernel<<<dim3(1), block, 0, st>>>((unsigned*)scratch, (long)plan.blocks, (long)plan.scan_trips, count);
  SAT_LAUNCH_CHECK("ubz_compact (scan)");
  write_kernel<<<grid, block, 0, st>>>(label, confidence, adc, vplanes, adc_threshold, pixels, rc, (const unsigned*)scratch,
                                       (u64)capacity, out_index, out_label, out_confidence);
  SAT_LAUNCH_CHECK("ubz_compact (write)");
  return UBZ_OK;
}

extern "C" int ubz_expand(const int32_t* index, const uint8_t* label, const uint16_t* confidence, int64_t n,
                          const unsigned long long* count, int fill_label, uint8_t* out_label, uint16_t* out_confidence, int P,
                          int rows, int cols, unsigned long long* status, void* stream) {
  ubz::Plan plan;
  if (check_list("ubz_expand", index, label, confidence, true, n, count, P, rows, cols, status, &plan)) return UBZ_EINVAL;
  SAT_CHECK(out_label && out_confidence, "ubz_expand: null pointer (out_label, out_confidence)");
  SAT_CHECK(fill_label >= 0 && fill_label <= 255, "ubz_expand: fill_label=%d must be 0..255", fill_label);
  SAT_CHECK(aligned(confidence, 2) && aligned(out_confidence, 2), "ubz_expand: confidence and out_confidence must be 2-byte aligned");
  const u64 px = (u64)plan.pixels;
  const void* outs[2] = {out_label, out_confidence};
  const u64 obytes[2] = {px, 2 * px};
  for (int i = 0; i < 2; ++i)
    SAT_CHECK(!overlap(outs[i], obytes[i], index, 4ull * (u64)n) && !overlap(outs[i], obytes[i], label, (u64)n) &&
                  !overlap(outs[i], obytes[i], confidence, 2ull * (u64)n) && !overlap(outs[i], obytes[i], count, 8) &&
                  !overlap(outs[i], obytes[i], status, 8),
              "ubz_expand: an output overlaps an input or status");
  SAT_CHECK(!overlap(out_label, px, out_confidence, 2 * px), "ubz_expand: out_label overlaps out_confidence");
  const fill_t fl = make_fill(out_label, (long)px, fill_label), fc = make_fill(out_confidence, (long)(2 * px), 0);
  const int64_t fgrid = ubz::stride_grid(fl.units + fc.units);
  fill_kernel<<<dim3((unsigned)(fgrid < 1 ? 1 : fgrid)), dim3(UBZ_LANES), 0, (hipStream_t)stream>>>(fl, fc);
  SAT_LAUNCH_CHECK("ubz_expand (fill)");
  if (n > 0) {
    scatter_kernel<true><<<dim3((unsigned)ubz::stride_grid(n)), dim3(UBZ_LANES), 0, (hipStream_t)stream>>>(
        index, label, confidence, (long)n, count, out_label, out_confidence, (int)plan.pixels, status);
    SAT_LAUNCH_CHECK("ubz_expand (scatter)");
  }
  return UBZ_OK;
}
