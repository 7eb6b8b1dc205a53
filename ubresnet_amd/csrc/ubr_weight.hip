// libubresnet_weight.so: device-side pixel weights for PixelWiseNLLLoss (include/ubresnet_weight.h).  It links against
// none of the other libraries and shares ubr_sat.h with them; launches are plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include "ubr_weight_tile.h"
#include "ubr_sat.h"

#define UBW_VERSION 1

SAT_RETURN_CODES(UBW);
SAT_EXPORTS(ubw, UBW_VERSION)
using namespace sat;

namespace {

using namespace ubw;

struct CountK {
  const long long* lab;          // [B][n]
  unsigned long long* counts;    // [B][UBW_MAX_CLASSES], zero
  int n, C, gx;                  // pixels of an image; classes; workgroups per image
};

// the wave's pixels of class c, for every class, out of one class id per lane (NONE: no class)
__device__ __forceinline__ void tally(unsigned (&cnt)[UBW_MAX_CLASSES], unsigned id, int C) {
#pragma unroll
  for (int c = 0; c < UBW_MAX_CLASSES; ++c)
    if (c < C) cnt[c] += (unsigned)__popcll(__ballot(id == (unsigned)c));
}

// Count pass: gx workgroups per image stride over its groups of UBW_LANE_PIXELS pixels; an image whose first label is 16-byte
// aligned is read with two 16-byte loads per lane and trip, any other with element loads (the same for every lane of the
// workgroup).  A wave counts with one ballot per class and pixel slot into wave-uniform counters, lane 0 of each wave adds
// them into the workgroup's LDS row, and the workgroup issues one 64-bit integer atomic per class it met.  The last n % 4
// pixels of an image go to the first lanes of its first workgroup.
__global__ __launch_bounds__(UBW_BLOCK) void count_kernel(const CountK k) {
  __shared__ unsigned s_cnt[UBW_MAX_CLASSES];
  const int t = threadIdx.x;
  const unsigned b = blockIdx.x / (unsigned)k.gx, chunk = blockIdx.x - b * (unsigned)k.gx;
  const long long* lab = k.lab + (long)b * k.n;
  if (t < UBW_MAX_CLASSES) s_cnt[t] = 0;
  __syncthreads();
  const bool vec = ((uintptr_t)lab & 15) == 0;
  const int nvec = k.n / LP, stride = k.gx * UBW_BLOCK;
  unsigned cnt[UBW_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < UBW_MAX_CLASSES; ++c) cnt[c] = 0;
  for (int g0 = (int)chunk * UBW_BLOCK; g0 < nvec; g0 += stride) {      // the same trips for every lane: ballots see whole waves
    const int g = g0 + t;
    unsigned id[LP] = {NONE, NONE, NONE, NONE};
    if (g < nvec) {
      const long long* p = lab + (long)g * LP;                           // g * 4 + 3 < n
      long long v[LP];
      if (vec) {
        const LL2 a = reinterpret_cast<const LL2*>(p)[0], c = reinterpret_cast<const LL2*>(p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = c.x; v[3] = c.y;
      } else {
#pragma unroll
        for (int j = 0; j < LP; ++j) v[j] = p[j];
      }
#pragma unroll
      for (int j = 0; j < LP; ++j) id[j] = class_of(v[j], k.C);
    }
#pragma unroll
    for (int j = 0; j < LP; ++j) tally(cnt, id[j], k.C);
  }
  if (chunk == 0 && (k.n & (LP - 1)) != 0 && t < 64) {
    const int i = nvec * LP + t;
    tally(cnt, t < (k.n & (LP - 1)) ? class_of(lab[i], k.C) : NONE, k.C);
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int c = 0; c < UBW_MAX_CLASSES; ++c)
      if (cnt[c] != 0) atomicAdd(&s_cnt[c], cnt[c]);
  }
  __syncthreads();
  if (t < UBW_MAX_CLASSES && s_cnt[t] != 0)
    atomicAdd(&k.counts[(long)b * UBW_MAX_CLASSES + t], (unsigned long long)s_cnt[t]);
}

// Apply pass: one workgroup per UBW_TILE_H x UBW_TILE_W tile of an image, a lane per UBW_LANE_PIXELS pixels of a tile row.
// The first 16 lanes turn the image's row of counts into its 16 class weights; every lane classifies its pixels and the
// workgroup stages the tile's class ids, a byte per pixel, with an R-wide halo in LDS (ubr_weight_tile.h, phase 1); the window
// test is separable: the set of classes in columns x-R..x+R per staged row (phase 2), then the union of 2R+1 rows (phase 3),
// which also stores the weights, 16 bytes per lane on the fast path.  R = 0 stages nothing.
template <int R>
__global__ __launch_bounds__(UBW_BLOCK) void apply_kernel(const ApplyK k) {
  __shared__ float wc[UBW_MAX_CLASSES];
  __shared__ __attribute__((aligned(16))) unsigned char ids[ids_bytes(R)];
  __shared__ __attribute__((aligned(16))) unsigned short rm[rm_words(R)];
  const int t = threadIdx.x;
  const unsigned b = blockIdx.x / (unsigned)k.tiles, tile = blockIdx.x - b * (unsigned)k.tiles;
  const int y0 = (int)(tile / (unsigned)k.tiles_x) * TH, x0 = (int)(tile % (unsigned)k.tiles_x) * TW;
  const long n = (long)k.H * k.W;
  const long long* lab = k.lab + (long)b * n;
  if (t < UBW_MAX_CLASSES) wc[t] = class_weight(k.counts + (long)b * UBW_MAX_CLASSES, t, k.max_weight);
  const unsigned own = stage<R>(k, lab, x0, y0, t, ids);
  __syncthreads();
  if (R > 0) {
    row_sets<R>(t, ids, rm);
    __syncthreads();
  }
  finish<R>(k, k.wgt + (long)b * n, x0, y0, t, own, rm, wc);
}

}  // namespace

extern "C" int ubw_pixel_weights(const int64_t* label, float* weight, int64_t* counts,
                                 int B, int H, int W, int C,
                                 float max_weight, int radius, float gain, int lo, void* stream) {
  SAT_CHECK(label && weight && counts, "ubw_pixel_weights: null pointer (label %p, weight %p, counts %p)", (const void*)label,
            (void*)weight, (void*)counts);
  SAT_CHECK(B >= 1 && H >= 1 && W >= 1, "ubw_pixel_weights: B=%d, H=%d, W=%d must be >= 1", B, H, W);
  const long long hw = (long long)H * W;
  SAT_CHECK(hw < (1ll << 31) && (long long)B * hw < (1ll << 31), "ubw_pixel_weights: B*H*W = %d*%d*%d must be below 2^31", B, H, W);
  SAT_CHECK(C >= 1 && C <= UBW_MAX_CLASSES, "ubw_pixel_weights: C=%d must be 1..%d", C, UBW_MAX_CLASSES);
  SAT_CHECK(radius >= 0 && radius <= UBW_MAX_RADIUS, "ubw_pixel_weights: radius=%d must be 0..%d", radius, UBW_MAX_RADIUS);
  SAT_CHECK(lo >= 0 && lo <= C, "ubw_pixel_weights: lo=%d must be 0..C=%d", lo, C);
  SAT_CHECK(max_weight > 0.0f, "ubw_pixel_weights: max_weight=%g must be > 0 (+inf: no cap)", (double)max_weight);
  SAT_CHECK(gain >= 0.0f && gain < INFINITY, "ubw_pixel_weights: gain=%g must be finite and >= 0", (double)gain);
  SAT_CHECK(aligned(label, 8) && aligned(counts, 8) && aligned(weight, 4),
            "ubw_pixel_weights: a pointer lacks its natural alignment (4 bytes for float, 8 for int64_t)");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, sizeof(int64_t) * UBW_MAX_CLASSES * (size_t)B, s);
  if (e != hipSuccess) {
    set_error("ubw_pixel_weights: memset of counts failed: %s", hipGetErrorString(e));
    return UBW_ELAUNCH;
  }
  CountK ck{};
  ck.lab = (const long long*)label; ck.counts = (unsigned long long*)counts; ck.n = (int)hw; ck.C = C;
  const long long span = (long long)UBW_BLOCK * UBW_LANE_PIXELS;
  long long gx = (hw + span - 1) / span, cap = UBW_MAX_GRID / B;
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  ck.gx = (int)gx;
  count_kernel<<<dim3((unsigned)(gx * B)), dim3(UBW_BLOCK), 0, s>>>(ck);
  e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("ubw_pixel_weights: launch of the count pass failed: %s", hipGetErrorString(e));
    return UBW_ELAUNCH;
  }
  ApplyK k{};
  k.lab = (const long long*)label; k.wgt = weight; k.counts = (const long long*)counts;
  k.H = H; k.W = W; k.C = C; k.lo = lo;
  k.tiles_x = (W + UBW_TILE_W - 1) / UBW_TILE_W;
  k.tiles = k.tiles_x * ((H + UBW_TILE_H - 1) / UBW_TILE_H);
  k.max_weight = max_weight; k.gain = gain;
  k.vlab = W % 4 == 0 && aligned(label, 16);
  k.vwgt = W % 4 == 0 && aligned(weight, 16);
  const dim3 grid((unsigned)((long long)k.tiles * B)), block(UBW_BLOCK);            // tiles * B <= B*H*W < 2^31
  switch (radius) {
    case 0: apply_kernel<0><<<grid, block, 0, s>>>(k); break;
    case 1: apply_kernel<1><<<grid, block, 0, s>>>(k); break;
    case 2: apply_kernel<2><<<grid, block, 0, s>>>(k); break;
    case 3: apply_kernel<3><<<grid, block, 0, s>>>(k); break;
    default: apply_kernel<4><<<grid, block, 0, s>>>(k); break;
  }
  e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("ubw_pixel_weights: launch of the apply pass failed: %s", hipGetErrorString(e));
    return UBW_ELAUNCH;
  }
  return UBW_OK;
}
