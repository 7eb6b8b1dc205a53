// libubresnet_post.so: event products of whole-view inference (include/ubresnet_post.h).  It links against none of
// the other libraries and shares ubr_sat.h with them; launches are plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/ubresnet_post.h"
#include "ubr_sat.h"

#define UBP_VERSION 1

SAT_RETURN_CODES(UBP);
SAT_EXPORTS(ubp, UBP_VERSION)
using namespace sat;

namespace {

struct PostK {
  int th, tw, rows, cols, C, vplanes, fill;
  float thr;
  // keep windows in tile coordinates, already clipped to the view on the host: every pixel of [kr0,kr1) x [kc0,kc1) is written
  int plane[UBP_MAX_TILES], r0[UBP_MAX_TILES], c0[UBP_MAX_TILES];
  int kr0[UBP_MAX_TILES], kr1[UBP_MAX_TILES], kc0[UBP_MAX_TILES], kc1[UBP_MAX_TILES];
};

// grid (x: 256-pixel chunks of the keep window, strided; y: tile).  Consecutive lanes take consecutive columns of a keep-window
// row: the ADC reads, the C score-plane reads and both stores coalesce.  The scores of an unlit pixel are never loaded.  Classes
// are counted per wave by ballot into a per-workgroup LDS histogram (all blocks of a tile share one plane); one 64-bit global
// atomic per non-empty bin at the end, as confusion_kernel flushes.
__global__ __launch_bounds__(256) void stitch_products_kernel(const float* __restrict__ logp, const float* __restrict__ adc,
                                                              uint8_t* __restrict__ label, uint16_t* __restrict__ conf,
                                                              unsigned long long* counts, const PostK k) {
  __shared__ unsigned int hist[UBP_MAX_CLASSES];
  if (threadIdx.x < UBP_MAX_CLASSES) hist[threadIdx.x] = 0u;
  __syncthreads();
  const int t = blockIdx.y;
  const int kh = k.kr1[t] - k.kr0[t], kw = k.kc1[t] - k.kc0[t];
  const int n = (kh > 0 && kw > 0) ? kh * kw : 0;            // th * tw fits an int (checked on the host)
  const long vpx = (long)k.rows * k.cols, tpx = (long)k.th * k.tw;
  const int plane = k.plane[t];
  const bool count = counts != nullptr;
  for (long base = (long)blockIdx.x * 256; base < n; base += (long)gridDim.x * 256) {   // wave-uniform trip count (ballot below)
    const long i = base + threadIdx.x;                     // < n + 256: the quotient below is a 32-bit division
    const bool valid = i < n;
    bool lit = false;
    int best = 0;
    if (valid) {
      const int y = (int)((unsigned)i / (unsigned)kw), x = (int)i - y * kw;
      const int ty = k.kr0[t] + y, tx = k.kc0[t] + x;
      const long opx = (long)(k.r0[t] + ty) * k.cols + (k.c0[t] + tx);
      const long o = (long)plane * vpx + opx;
      if (adc != nullptr) {
        const float* a = adc + (long)plane * k.vplanes * vpx + opx;
        for (int v = 0; v < k.vplanes; ++v) lit |= a[(long)v * vpx] > k.thr;       // NaN > thr is false
      } else {
        lit = true;
      }
      if (lit) {
        const float* s = logp + (long)t * k.C * tpx + (long)ty * k.tw + tx;
        float bv = s[0];
        for (int c = 1; c < k.C; c += 4) {             // four independent loads in flight; -inf never wins a strict compare
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = (c + j < k.C) ? s[(long)(c + j) * tpx] : -INFINITY;
#pragma unroll
          for (int j = 0; j < 4; ++j) if (v[j] > bv) { bv = v[j]; best = c + j; }
        }
        label[o] = (uint8_t)best;
        const _Float16 h = (_Float16)expf(bv);         // v_cvt_f16_f32: round to nearest even, subnormals kept
        conf[o] = __builtin_bit_cast(uint16_t, h);
      } else {
        label[o] = (uint8_t)k.fill;
        conf[o] = (uint16_t)0;
      }
    }
    if (count && __ballot(lit) != 0ull) {                 // wave-uniform: a wave without a lit pixel counts nothing
      for (int c = 0; c < k.C; ++c) {
        const unsigned long long m = __ballot(lit && best == c);
        if ((threadIdx.x & 63) == 0 && m != 0ull) atomicAdd(&hist[c], (unsigned int)__popcll(m));
      }
    }
  }
  __syncthreads();
  if (count && (int)threadIdx.x < k.C && hist[threadIdx.x] != 0u)
    atomicAdd(&counts[(long)plane * k.C + threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

}  // namespace

extern "C" int ubp_stitch_products(const float* logp, int C, int th, int tw, const int32_t* tile_desc_host, int ntiles,
                                   const float* adc, int vplanes, float adc_threshold,
                                   uint8_t* label, uint16_t* confidence, unsigned long long* counts,
                                   int fill_label, int P, int rows, int cols, void* stream) {
  SAT_CHECK(logp && label && confidence, "ubp_stitch_products: null pointer");
  SAT_CHECK(tile_desc_host && ntiles >= 1 && ntiles <= UBP_MAX_TILES && th > 0 && tw > 0 && rows > 0 && cols > 0 && P >= 1 &&
            (long)th * tw < (1l << 30),
            "ubp_stitch_products: bad arguments (ntiles=%d must be 1..%d; th, tw, rows, cols, P positive, th * tw < 2^30)", ntiles, UBP_MAX_TILES);
  SAT_CHECK(C >= 1 && C <= UBP_MAX_CLASSES, "ubp_stitch_products: C=%d must be 1..%d", C, UBP_MAX_CLASSES);
  SAT_CHECK(vplanes >= 1, "ubp_stitch_products: vplanes=%d must be >= 1", vplanes);
  SAT_CHECK(fill_label >= 0 && fill_label <= 255, "ubp_stitch_products: fill_label=%d must be 0..255", fill_label);
  PostK k{};
  k.th = th; k.tw = tw; k.rows = rows; k.cols = cols; k.C = C; k.vplanes = vplanes; k.fill = fill_label; k.thr = adc_threshold;
  for (int t = 0; t < ntiles; ++t) {
    const int32_t* d = tile_desc_host + 7 * t;
    SAT_CHECK(d[0] >= 0 && d[0] < P && d[1] >= 0 && d[2] >= 0 && d[1] < rows && d[2] < cols,
              "ubp_stitch_products: tile %d origin out of range", t);
    SAT_CHECK(d[3] >= 0 && d[3] <= d[4] && d[4] <= th && d[5] >= 0 && d[5] <= d[6] && d[6] <= tw,
              "ubp_stitch_products: tile %d keep window out of range", t);
    k.plane[t] = d[0]; k.r0[t] = d[1]; k.c0[t] = d[2];
    k.kr0[t] = d[3]; k.kr1[t] = d[4] < rows - d[1] ? d[4] : rows - d[1];
    k.kc0[t] = d[5]; k.kc1[t] = d[6] < cols - d[2] ? d[6] : cols - d[2];
  }
  const unsigned gx = (unsigned)(((long)th * tw + 256 * 8 - 1) / (256 * 8));
  stitch_products_kernel<<<dim3(gx, (unsigned)ntiles), dim3(256), 0, (hipStream_t)stream>>>(logp, adc, label, confidence, counts, k);
  SAT_LAUNCH_CHECK("ubp_stitch_products");
  return UBP_OK;
}
