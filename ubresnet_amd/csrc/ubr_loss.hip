// libubresnet_loss.so: the pixel-wise focal loss and its normalised means (include/ubresnet_loss.h).  It links against none of
// the other libraries and shares ubr_sat.h with them, and ubr_rows.h with ubr_dice.hip; the launches are plain <<<>>> on the
// caller's stream, and there is no atomic operation: the forward's streaming pass leaves one row of partials per workgroup, one
// workgroup adds the rows in a fixed order.
#include <hip/hip_runtime.h>
#include <math.h>
#include "ubr_loss_term.h"
#include "ubr_rows.h"
#include "ubr_sat.h"

#define UBL_VERSION 1
#define UBL_TRIP_UNITS (UBL_BLOCK * UBL_UNROLL)
#define UBL_TRIP_PIXELS (UBL_TRIP_UNITS * 4)
#define UBL_FINISH_SUB 16                                  /* the finish adds UBL_FINISH_SUB interleaved row sequences, then those */
#define UBL_FINISH_BLOCK (UBL_FINISH_SUB * UBL_ROW_WORDS)  /* 576 lanes: one per (sequence, word) */

SAT_RETURN_CODES(UBL);
SAT_EXPORTS(ubl, UBL_VERSION)
using namespace sat;
using namespace rowsum;

namespace {

// what a lane keeps over its trips: the totals in registers, the per-class sums in a column of LDS that is the lane's own (so
// neither a barrier nor an atomic is needed until the end)
struct Lane {
  double s, ws;
  unsigned n, bad;
};

__device__ __forceinline__ void take(Lane& a, double* cls_sum, unsigned* cls_n, long long t, bool ok, float lp, float pw, const float* cw,
                                     float gamma) {
  if (!ok) return;
  const float w = cw ? cw[t] : 1.f;
  const float v = ubl::term(lp, gamma, w, pw);
  const float wp = w * pw;
  a.s += (double)v;
  a.ws += (double)wp;
  a.n += 1u;
  cls_sum[(int)t * UBL_BLOCK] += (double)v;
  cls_n[(int)t * UBL_BLOCK] += 1u;
}

__device__ __forceinline__ bool integer_word(int word) {
  return word == UBL_ROW_VALID || word == UBL_ROW_BAD || word >= UBL_ROW_CLASS_PIXELS;
}

// The forward's streaming pass.  VEC: a unit is 4 pixels of one image (hw % 4 == 0): the target as two 16-byte loads, the weight
// as one, predict gathered at the target channel only; all loads of a trip are issued before any is used.  Otherwise one pixel at
// a time with the same walk over the same trips.  Every index is checked against the number of units / pixels.
template <bool VEC>
__global__ __launch_bounds__(UBL_BLOCK) void focal_fwd_kernel(const float* __restrict__ pred, const long long* __restrict__ target,
                                                              const float* __restrict__ pw, const float* __restrict__ cw, int C, long hw,
                                                              long total, long long ignore_index, float gamma, u64* __restrict__ rows) {
  __shared__ double cls_sum[UBL_MAX_CLASSES * UBL_BLOCK];
  __shared__ unsigned cls_n[UBL_MAX_CLASSES * UBL_BLOCK];
  __shared__ u64 wave_row[UBL_BLOCK / 64][UBL_ROW_WORDS];
  const int lane = threadIdx.x;
  for (int c = 0; c < C; ++c) {
    cls_sum[c * UBL_BLOCK + lane] = 0.0;
    cls_n[c * UBL_BLOCK + lane] = 0u;
  }
  Lane a = {0.0, 0.0, 0u, 0u};
  const long trips = (total + UBL_TRIP_PIXELS - 1) / UBL_TRIP_PIXELS;
  for (long trip = blockIdx.x; trip < trips; trip += gridDim.x) {
    if (VEC) {
      const long units = total / 4;
      const long base = trip * UBL_TRIP_UNITS + lane;
      ll2 T[UBL_UNROLL][2];
      float4 P[UBL_UNROLL];
      float LP[UBL_UNROLL][4];
      bool OK[UBL_UNROLL][4];
#pragma unroll
      for (int u = 0; u < UBL_UNROLL; ++u) {
        const long i = base + u * UBL_BLOCK;
        const bool in = i < units;
        T[u][0] = in ? *(const ll2*)(target + 4 * i) : (ll2){ignore_index, ignore_index};
        T[u][1] = in ? *(const ll2*)(target + 4 * i + 2) : (ll2){ignore_index, ignore_index};
        P[u] = in ? *(const float4*)(pw + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < UBL_UNROLL; ++u) {
        const long i = base + u * UBL_BLOCK;
        const bool in = i < units;
        const long p0 = 4 * i, n = p0 / hw, r = p0 - n * hw;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const long long t = T[u][k >> 1][k & 1];
          OK[u][k] = in && contributes(t, C, ignore_index);
          if (in && t != ignore_index && !OK[u][k]) a.bad += 1u;
          LP[u][k] = OK[u][k] ? pred[(n * C + t) * hw + r + k] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < UBL_UNROLL; ++u) {
        const float pv[4] = {P[u].x, P[u].y, P[u].z, P[u].w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          take(a, cls_sum + lane, cls_n + lane, T[u][k >> 1][k & 1], OK[u][k], LP[u][k], pv[k], cw, gamma);
      }
    } else {
      const long base = trip * UBL_TRIP_PIXELS + lane;
      long long T[4 * UBL_UNROLL];
      float P[4 * UBL_UNROLL], LP[4 * UBL_UNROLL];
      bool OK[4 * UBL_UNROLL];
#pragma unroll
      for (int j = 0; j < 4 * UBL_UNROLL; ++j) {
        const long p = base + j * UBL_BLOCK;
        T[j] = p < total ? target[p] : ignore_index;
        P[j] = p < total ? pw[p] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4 * UBL_UNROLL; ++j) {
        const long p = base + j * UBL_BLOCK;
        const bool in = p < total;
        const long n = p / hw, r = p - n * hw;
        OK[j] = in && contributes(T[j], C, ignore_index);
        if (in && T[j] != ignore_index && !OK[j]) a.bad += 1u;
        LP[j] = OK[j] ? pred[(n * C + T[j]) * hw + r] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4 * UBL_UNROLL; ++j) take(a, cls_sum + lane, cls_n + lane, T[j], OK[j], LP[j], P[j], cw, gamma);
    }
  }
  // the lanes of a wave in the fixed order of the shuffle tree, then the four waves in order
  const int wave = lane >> 6;
  const double s = wave_sum(a.s), ws = wave_sum(a.ws);
  const u64 n = wave_sum((u64)a.n), bad = wave_sum((u64)a.bad);
  if ((lane & 63) == 0) {
    wave_row[wave][UBL_ROW_LOSS_SUM] = (u64)__double_as_longlong(s);
    wave_row[wave][UBL_ROW_WEIGHT_SUM] = (u64)__double_as_longlong(ws);
    wave_row[wave][UBL_ROW_VALID] = n;
    wave_row[wave][UBL_ROW_BAD] = bad;
  }
  for (int c = 0; c < UBL_MAX_CLASSES; ++c) {
    const double cs = c < C ? wave_sum(cls_sum[c * UBL_BLOCK + lane]) : 0.0;
    const u64 cn = c < C ? wave_sum((u64)cls_n[c * UBL_BLOCK + lane]) : 0ull;
    if ((lane & 63) == 0) {
      wave_row[wave][UBL_ROW_CLASS_LOSS + c] = (u64)__double_as_longlong(cs);
      wave_row[wave][UBL_ROW_CLASS_PIXELS + c] = cn;
    }
  }
  __syncthreads();
  if (lane < UBL_ROW_WORDS)
    rows[(long)blockIdx.x * UBL_ROW_WORDS + lane] = add_wave_rows(wave_row, lane, integer_word(lane));
}

// One workgroup: lane (q, word) adds word `word` of the rows q, q + 16, q + 32, .. in that order; then lane `word` adds the 16
// sequences in order.  The same rows give the same bits.
__global__ __launch_bounds__(UBL_FINISH_BLOCK) void focal_finish_kernel(const u64* __restrict__ rows, int nrows, int mode, u64 total,
                                                                        u64* __restrict__ ctl, float* __restrict__ loss) {
  __shared__ u64 sub[UBL_FINISH_SUB][UBL_ROW_WORDS];
  __shared__ u64 tot[UBL_ROW_WORDS];
  const int word = threadIdx.x % UBL_ROW_WORDS, q = threadIdx.x / UBL_ROW_WORDS;
  const bool integer = integer_word(word);
  sub[q][word] = sequence_sum<UBL_FINISH_SUB, UBL_ROW_WORDS>(rows, nrows, q, word, integer);
  __syncthreads();
  if (threadIdx.x < UBL_ROW_WORDS) {
    const u64 out = sequences_sum(sub, word, integer);
    tot[word] = out;
    // row words 0..3 are ctl words 0..3; the per-class words move up behind the four words of the mean
    ctl[word < UBL_ROW_CLASS_LOSS ? word : word + (UBL_CTL_CLASS_LOSS - UBL_ROW_CLASS_LOSS)] = out;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const ubl::Mean r = ubl::mean(mode, __longlong_as_double((long long)tot[UBL_ROW_LOSS_SUM]),
                                  __longlong_as_double((long long)tot[UBL_ROW_WEIGHT_SUM]), tot[UBL_ROW_VALID], total);
    ctl[UBL_CTL_DENOM] = (u64)__double_as_longlong(r.denom);
    ctl[UBL_CTL_INV_DENOM] = (u64)__float_as_uint(r.inv_denom);
    ctl[UBL_CTL_LOSS] = (u64)__float_as_uint(r.loss);
    ctl[UBL_CTL_MODE] = (u64)mode;
    *loss = r.loss;
  }
}

__device__ __forceinline__ float grad_of(bool ok, long long t, float lp, float pw, const float* cw, float gamma, float s) {
  if (!ok) return 0.f;
  const float w = cw ? cw[t] : 1.f;
  return ubl::grad(s, pw, w, ubl::deriv(lp, gamma));
}

// The backward: the walk of the forward.  Every channel of every pixel is written: VEC as one 16-byte store per channel and
// unit, otherwise one float per channel and pixel.
template <bool VEC>
__global__ __launch_bounds__(UBL_BLOCK) void focal_bwd_kernel(const float* __restrict__ gloss, const u64* __restrict__ ctl,
                                                              const float* __restrict__ pred, const long long* __restrict__ target,
                                                              const float* __restrict__ pw, const float* __restrict__ cw, int C, long hw,
                                                              long total, long long ignore_index, float gamma, float* __restrict__ gpred) {
  const int lane = threadIdx.x;
  const float s = *gloss * __uint_as_float((unsigned)ctl[UBL_CTL_INV_DENOM]);
  const long trips = (total + UBL_TRIP_PIXELS - 1) / UBL_TRIP_PIXELS;
  for (long trip = blockIdx.x; trip < trips; trip += gridDim.x) {
    if (VEC) {
      const long units = total / 4;
      const long base = trip * UBL_TRIP_UNITS + lane;
      ll2 T[UBL_UNROLL][2];
      float4 P[UBL_UNROLL];
      float LP[UBL_UNROLL][4];
      bool OK[UBL_UNROLL][4];
#pragma unroll
      for (int u = 0; u < UBL_UNROLL; ++u) {
        const long i = base + u * UBL_BLOCK;
        const bool in = i < units;
        T[u][0] = in ? *(const ll2*)(target + 4 * i) : (ll2){ignore_index, ignore_index};
        T[u][1] = in ? *(const ll2*)(target + 4 * i + 2) : (ll2){ignore_index, ignore_index};
        P[u] = in ? *(const float4*)(pw + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < UBL_UNROLL; ++u) {
        const long i = base + u * UBL_BLOCK;
        const bool in = i < units;
        const long p0 = 4 * i, n = p0 / hw, r = p0 - n * hw;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const long long t = T[u][k >> 1][k & 1];
          OK[u][k] = in && contributes(t, C, ignore_index);
          LP[u][k] = OK[u][k] ? pred[(n * C + t) * hw + r + k] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < UBL_UNROLL; ++u) {
        const long i = base + u * UBL_BLOCK;
        if (i >= units) continue;
        const long p0 = 4 * i, n = p0 / hw, r = p0 - n * hw;
        const float pv[4] = {P[u].x, P[u].y, P[u].z, P[u].w};
        float g[4];
        int tc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const long long t = T[u][k >> 1][k & 1];
          g[k] = grad_of(OK[u][k], t, LP[u][k], pv[k], cw, gamma, s);
          tc[k] = OK[u][k] ? (int)t : -1;
        }
        float* dst = gpred + n * C * hw + r;
        for (int c = 0; c < C; ++c)
          *(float4*)(dst + c * hw) = make_float4(tc[0] == c ? g[0] : 0.f, tc[1] == c ? g[1] : 0.f, tc[2] == c ? g[2] : 0.f, tc[3] == c ? g[3] : 0.f);
      }
    } else {
      const long base = trip * UBL_TRIP_PIXELS + lane;
      long long T[4 * UBL_UNROLL];
      float P[4 * UBL_UNROLL], LP[4 * UBL_UNROLL];
      bool OK[4 * UBL_UNROLL];
#pragma unroll
      for (int j = 0; j < 4 * UBL_UNROLL; ++j) {
        const long p = base + j * UBL_BLOCK;
        T[j] = p < total ? target[p] : ignore_index;
        P[j] = p < total ? pw[p] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4 * UBL_UNROLL; ++j) {
        const long p = base + j * UBL_BLOCK;
        const long n = p / hw, r = p - n * hw;
        OK[j] = p < total && contributes(T[j], C, ignore_index);
        LP[j] = OK[j] ? pred[(n * C + T[j]) * hw + r] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4 * UBL_UNROLL; ++j) {
        const long p = base + j * UBL_BLOCK;
        if (p >= total) continue;
        const long n = p / hw, r = p - n * hw;
        const float g = grad_of(OK[j], T[j], LP[j], P[j], cw, gamma, s);
        const int tc = OK[j] ? (int)T[j] : -1;
        float* dst = gpred + n * C * hw + r;
        for (int c = 0; c < C; ++c) dst[c * hw] = tc == c ? g : 0.f;
      }
    }
  }
}

inline unsigned grid_of(long total) {
  long grid = (total + UBL_TRIP_PIXELS - 1) / UBL_TRIP_PIXELS;
  return (unsigned)(grid > UBL_MAX_GRID ? UBL_MAX_GRID : grid);
}

}  // namespace

// the checks the two calls share; `name` starts the message
#define UBL_CHECK_OPERANDS(name, predict, target, pixelweights, classw, N, C, H, W, gamma)                                       \
  SAT_CHECK((predict) && (target) && (pixelweights), name ": null pointer (predict, target, pixelweights)");                     \
  SAT_CHECK((N) > 0 && (H) > 0 && (W) > 0, name ": bad extents N=%d H=%d W=%d", (N), (H), (W));                                   \
  SAT_CHECK((C) >= 1 && (C) <= UBL_MAX_CLASSES, name ": C=%d must be in [1, %d]", (C), UBL_MAX_CLASSES);                          \
  SAT_CHECK((gamma) == (gamma), name ": gamma is NaN");                                                                           \
  SAT_CHECK((gamma) >= 0.f && (gamma) < INFINITY, name ": gamma=%g must be finite and >= 0", (double)(gamma));                    \
  SAT_CHECK(aligned((predict), 4) && aligned((pixelweights), 4) && aligned((classw), 4) && aligned((target), 8),                 \
            name ": predict, pixelweights and classw must be 4-byte aligned, target 8-byte aligned")

extern "C" int ubl_focal_fwd(const float* predict, const int64_t* target, const float* pixelweights, const float* classw,
                             int N, int C, int H, int W, int64_t ignore_index, float gamma, int mode,
                             void* workspace, void* ctl, float* loss, void* stream) {
  UBL_CHECK_OPERANDS("ubl_focal_fwd", predict, target, pixelweights, classw, N, C, H, W, gamma);
  SAT_CHECK(workspace && ctl && loss, "ubl_focal_fwd: null pointer (workspace, ctl, loss)");
  SAT_CHECK(mode == UBL_MEAN_PIXELS || mode == UBL_MEAN_VALID || mode == UBL_MEAN_WEIGHTS, "ubl_focal_fwd: unknown mode %d", mode);
  SAT_CHECK(aligned(workspace, 16), "ubl_focal_fwd: workspace must be 16-byte aligned");
  SAT_CHECK(aligned(ctl, 8) && aligned(loss, 4), "ubl_focal_fwd: ctl must be 8-byte aligned, loss 4-byte aligned");
  SAT_CHECK(!overlap(workspace, UBL_WORKSPACE_BYTES, ctl, UBL_CTL_BYTES), "ubl_focal_fwd: ctl overlaps workspace");
  SAT_CHECK(!overlap(workspace, UBL_WORKSPACE_BYTES, loss, 4), "ubl_focal_fwd: loss inside workspace");
  SAT_CHECK(!overlap(ctl, UBL_CTL_BYTES, loss, 4), "ubl_focal_fwd: loss inside ctl");
  const long hw = (long)H * W, total = (long)N * hw;
  const unsigned grid = grid_of(total);
  const bool vec = hw % 4 == 0 && aligned(predict, 16) && aligned(target, 16) && aligned(pixelweights, 16);
  if (vec)
    focal_fwd_kernel<true><<<dim3(grid), dim3(UBL_BLOCK), 0, (hipStream_t)stream>>>(predict, (const long long*)target, pixelweights, classw,
                                                                                   C, hw, total, (long long)ignore_index, gamma, (u64*)workspace);
  else
    focal_fwd_kernel<false><<<dim3(grid), dim3(UBL_BLOCK), 0, (hipStream_t)stream>>>(predict, (const long long*)target, pixelweights, classw,
                                                                                    C, hw, total, (long long)ignore_index, gamma, (u64*)workspace);
  SAT_LAUNCH_CHECK("ubl_focal_fwd");
  focal_finish_kernel<<<dim3(1), dim3(UBL_FINISH_BLOCK), 0, (hipStream_t)stream>>>((const u64*)workspace, (int)grid, mode, (u64)total,
                                                                                  (u64*)ctl, loss);
  SAT_LAUNCH_CHECK("ubl_focal_fwd (finish)");
  return UBL_OK;
}

extern "C" int ubl_focal_bwd(const float* g_loss, const void* ctl, const float* predict, const int64_t* target, const float* pixelweights,
                             const float* classw, int N, int C, int H, int W, int64_t ignore_index, float gamma,
                             float* g_predict, void* stream) {
  UBL_CHECK_OPERANDS("ubl_focal_bwd", predict, target, pixelweights, classw, N, C, H, W, gamma);
  SAT_CHECK(g_loss && ctl && g_predict, "ubl_focal_bwd: null pointer (g_loss, ctl, g_predict)");
  SAT_CHECK(aligned(ctl, 8) && aligned(g_loss, 4) && aligned(g_predict, 4),
            "ubl_focal_bwd: ctl must be 8-byte aligned, g_loss and g_predict 4-byte aligned");
  const long hw = (long)H * W, total = (long)N * hw;
  const unsigned long long gbytes = 4ull * (unsigned long long)total * (unsigned long long)C;
  SAT_CHECK(!overlap(g_predict, gbytes, predict, gbytes), "ubl_focal_bwd: g_predict overlaps predict");
  SAT_CHECK(!overlap(g_predict, gbytes, target, 8ull * (unsigned long long)total), "ubl_focal_bwd: g_predict overlaps target");
  SAT_CHECK(!overlap(g_predict, gbytes, pixelweights, 4ull * (unsigned long long)total), "ubl_focal_bwd: g_predict overlaps pixelweights");
  SAT_CHECK(!overlap(g_predict, gbytes, ctl, UBL_CTL_BYTES), "ubl_focal_bwd: g_predict overlaps ctl");
  SAT_CHECK(!overlap(g_predict, gbytes, g_loss, 4), "ubl_focal_bwd: g_predict overlaps g_loss");
  const unsigned grid = grid_of(total);
  const bool vec = hw % 4 == 0 && aligned(predict, 16) && aligned(target, 16) && aligned(pixelweights, 16) && aligned(g_predict, 16);
  if (vec)
    focal_bwd_kernel<true><<<dim3(grid), dim3(UBL_BLOCK), 0, (hipStream_t)stream>>>(g_loss, (const u64*)ctl, predict, (const long long*)target,
                                                                                   pixelweights, classw, C, hw, total, (long long)ignore_index,
                                                                                   gamma, g_predict);
  else
    focal_bwd_kernel<false><<<dim3(grid), dim3(UBL_BLOCK), 0, (hipStream_t)stream>>>(g_loss, (const u64*)ctl, predict, (const long long*)target,
                                                                                    pixelweights, classw, C, hw, total, (long long)ignore_index,
                                                                                    gamma, g_predict);
  SAT_LAUNCH_CHECK("ubl_focal_bwd");
  return UBL_OK;
}
