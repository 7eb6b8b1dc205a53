// libubresnet_data.so: device-side batch preparation of the training loader (include/ubresnet_data.h).  It links against none of
// the other libraries and shares ubr_sat.h with them; launches are plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "../../include/ubresnet_data.h"
#include "ubr_sat.h"

#define UBD_VERSION 1

SAT_RETURN_CODES(UBD);
SAT_EXPORTS(ubd, UBD_VERSION)
using namespace sat;

namespace {

typedef long long ll2 __attribute__((ext_vector_type(2)));

struct PrepK {
  const float* lab;      // [n] wire labels
  long long* out;        // [n]
  float* img;            // [B][planes][hw], touched only by the THR instantiation
  float* wgt;            // [n] or null
  int n, nvec;           // pixels; full groups of UBD_LANE_PIXELS
  int off, planes, hw;
  float thr;
  int vlab, vout, vwgt, vimg;   // the region is 16-byte aligned (vimg: and hw % 4 == 0): vector accesses
};

// |v| < 2^31 -> trunc(v) + off (v_cvt_i32_f32 truncates toward zero; the value is in range); NaN fails the compare
__device__ __forceinline__ long long to_label(float v, int off) {
  return fabsf(v) < 2147483648.0f ? (long long)(int)v + (long long)off : LLONG_MIN;
}

// zero what is below the threshold in the `planes` values of the pixel at a[0], a[hw], ...; -> all of them were below
__device__ __forceinline__ bool threshold_pixel(float* a, int planes, int hw, float thr) {
  bool dark = true;
  for (int p = 0; p < planes; ++p) {
    float* q = a + (long)p * hw;
    if (*q < thr) *q = 0.0f; else dark = false;          // NaN < thr is false
  }
  return dark;
}

// One pass over the batch, UBD_LANE_PIXELS = 4 consecutive pixels per lane and trip, grid-strided: consecutive lanes take
// consecutive 16 bytes of the wire labels and of the weights and consecutive 32 bytes of the int64 labels.  Which regions are
// accessed as vectors is the same for every lane (k.v*): no branch diverges.  The last n % 4 pixels go to the first lanes of the
// grid, one each, with element accesses, so nothing past n is touched.
template <bool THR>
__global__ __launch_bounds__(UBD_BLOCK) void prep_batch_kernel(const PrepK k) {
  const long stride = (long)gridDim.x * UBD_BLOCK;
  const long t = (long)blockIdx.x * UBD_BLOCK + threadIdx.x;
  for (long g = t; g < k.nvec; g += stride) {
    const long i = g * 4;                                   // i + 3 < n < 2^31
    float v[4];
    if (k.vlab) {
      const float4 q = *reinterpret_cast<const float4*>(k.lab + i);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = k.lab[i + j];
    }
    bool dark[4] = {false, false, false, false};
    if (THR) {
      unsigned b = (unsigned)i / (unsigned)k.hw, r = (unsigned)i - b * (unsigned)k.hw;     // image and offset of pixel i
      if (k.vimg) {                                         // hw % 4 == 0: the four pixels share an image, every plane row is aligned
        float* a = k.img + (long)b * k.planes * k.hw + r;
#pragma unroll
        for (int j = 0; j < 4; ++j) dark[j] = true;
        for (int p = 0; p < k.planes; ++p) {
          float4* q = reinterpret_cast<float4*>(a + (long)p * k.hw);
          const float4 x = *q;
          const bool lo[4] = {x.x < k.thr, x.y < k.thr, x.z < k.thr, x.w < k.thr};
#pragma unroll
          for (int j = 0; j < 4; ++j) dark[j] = dark[j] && lo[j];
          if (lo[0] || lo[1] || lo[2] || lo[3])
            *q = make_float4(lo[0] ? 0.0f : x.x, lo[1] ? 0.0f : x.y, lo[2] ? 0.0f : x.z, lo[3] ? 0.0f : x.w);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dark[j] = threshold_pixel(k.img + (long)b * k.planes * k.hw + r, k.planes, k.hw, k.thr);
          if (++r == (unsigned)k.hw) { r = 0; ++b; }
        }
      }
    }
    long long o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (THR && dark[j]) ? 0ll : to_label(v[j], k.off);
    if (k.vout) {
      ll2* q = reinterpret_cast<ll2*>(k.out + i);
      ll2 lo2, hi2;
      lo2.x = o[0]; lo2.y = o[1]; hi2.x = o[2]; hi2.y = o[3];
      q[0] = lo2;
      q[1] = hi2;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) k.out[i + j] = o[j];
    }
    if (k.wgt != nullptr) {
      if (k.vwgt) {
        *reinterpret_cast<float4*>(k.wgt + i) = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) k.wgt[i + j] = 1.0f;
      }
    }
  }
  if (t < (long)(k.n & 3)) {
    const long i = (long)k.nvec * 4 + t;                    // < n
    bool dark = false;
    if (THR) {
      const unsigned b = (unsigned)i / (unsigned)k.hw, r = (unsigned)i - b * (unsigned)k.hw;
      dark = threshold_pixel(k.img + (long)b * k.planes * k.hw + r, k.planes, k.hw, k.thr);
    }
    k.out[i] = dark ? 0ll : to_label(k.lab[i], k.off);
    if (k.wgt != nullptr) k.wgt[i] = 1.0f;
  }
}

}  // namespace

extern "C" int ubd_prep_batch(const float* label_wire, int64_t* label, int64_t n, int32_t label_offset,
                              float* image, int planes, int64_t hw, int use_threshold, float threshold,
                              float* weight_fill, void* stream) {
  SAT_CHECK(label_wire && label, "ubd_prep_batch: null label pointer");
  SAT_CHECK(n >= 1 && n < (1ll << 31), "ubd_prep_batch: n=%lld must be 1..2^31-1", (long long)n);
  SAT_CHECK(planes >= 1, "ubd_prep_batch: planes=%d must be >= 1", planes);
  SAT_CHECK(aligned(label_wire, 4) && aligned(label, 8) && aligned(image, 4) && aligned(weight_fill, 4),
            "ubd_prep_batch: a pointer lacks its natural alignment (4 bytes for float, 8 for int64_t)");
  if (use_threshold) {
    SAT_CHECK(image, "ubd_prep_batch: the threshold is on and image is null");
    SAT_CHECK(hw >= 1 && hw <= n && n % hw == 0, "ubd_prep_batch: hw=%lld must be >= 1 and divide n=%lld", (long long)hw, (long long)n);
  }
  PrepK k{};
  k.lab = label_wire; k.out = (long long*)label; k.img = use_threshold ? image : nullptr; k.wgt = weight_fill;
  k.n = (int)n; k.nvec = (int)(n / UBD_LANE_PIXELS);
  k.off = label_offset; k.planes = planes; k.hw = use_threshold ? (int)hw : 1; k.thr = threshold;
  k.vlab = aligned(label_wire, 16); k.vout = aligned(label, 16); k.vwgt = aligned(weight_fill, 16);
  k.vimg = aligned(image, 16) && hw % 4 == 0;
  const long span = (long)UBD_BLOCK * UBD_LANE_PIXELS;
  long blocks = (n + span - 1) / span;
  if (blocks > UBD_MAX_GRID) blocks = UBD_MAX_GRID;
  if (use_threshold)
    prep_batch_kernel<true><<<dim3((unsigned)blocks), dim3(UBD_BLOCK), 0, (hipStream_t)stream>>>(k);
  else
    prep_batch_kernel<false><<<dim3((unsigned)blocks), dim3(UBD_BLOCK), 0, (hipStream_t)stream>>>(k);
  SAT_LAUNCH_CHECK("ubd_prep_batch");
  return UBD_OK;
}
