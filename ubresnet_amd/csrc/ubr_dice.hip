// libubresnet_dice.so: the soft Dice / Tversky region loss (include/ubresnet_dice.h).  It links against none of the other
// libraries and shares ubr_sat.h with them, and ubr_rows.h with ubr_loss.hip; the launches are plain <<<>>> on the caller's
// stream, and there is no atomic operation: the forward's streaming pass leaves one row of partials per workgroup, one workgroup
// adds the rows in a fixed order and derives the two coefficients per class that the backward multiplies with.
//
// The class of every addend is a channel index, not the data-dependent target: FP_c always, TP_c and FN_c by a select on t == c.
// So a lane keeps its 3 C fp64 sums and C counts in registers; the forward is instantiated for C = 1 .. UBK_REG_CLASSES, and once
// with the class loop bounded by the runtime C for the rest (up to 16: the same code, more registers, fewer waves).
#include <hip/hip_runtime.h>
#include <math.h>
#include "ubr_dice_term.h"
#include "ubr_rows.h"
#include "ubr_sat.h"

#define UBK_VERSION 1
#define UBK_TRIP_UNITS (UBK_BLOCK * UBK_UNROLL)
#define UBK_TRIP_PIXELS (UBK_TRIP_UNITS * 4)
#define UBK_FINISH_SUB 8                                   /* the finish adds UBK_FINISH_SUB interleaved row sequences, then those */
#define UBK_FINISH_LANES (UBK_FINISH_SUB * UBK_ROW_WORDS)  /* 528: one per (sequence, word) */
#define UBK_FINISH_BLOCK 576                               /* the next multiple of the wave */

SAT_RETURN_CODES(UBK);
SAT_EXPORTS(ubk, UBK_VERSION)
using namespace sat;
using namespace rowsum;

namespace {

// what a lane keeps over its trips; CM is the bound of the unrolled class loops, so every index is a constant
template <int CM>
struct Lane {
  double tp[CM], fp[CM], fn[CM];
  unsigned n[CM], bad;
};

// one pixel: lp[c] are its log-probabilities (c < C), ok says whether it contributes.  Selects, not products by zero: what a
// pixel that does not contribute holds is never added.
template <int CT, int CM>
__device__ __forceinline__ void take(Lane<CM>& a, int C, long long t, bool ok, float pw, const float (&lp)[CM]) {
  float lpt = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (CT || c < C) lpt = t == c ? lp[c] : lpt;
  const float fnv = ubk::lost(lpt, pw);
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (CT || c < C) {
      const float v = ubk::hit(lp[c], pw);
      const bool is = ok && t == c, other = ok && t != c;
      a.tp[c] += is ? (double)v : 0.0;
      a.fp[c] += other ? (double)v : 0.0;
      a.fn[c] += is ? (double)fnv : 0.0;
      a.n[c] += is ? 1u : 0u;
    }
}

// The forward's streaming pass.  CT: the number of classes, or 0 for the runtime C.  VEC: a unit is 4 pixels of one image
// (hw % 4 == 0): the target as two 16-byte loads, the weight as one, predict as one per channel; all loads of a trip are issued
// before any is used.  Otherwise one pixel at a time with the same walk over the same trips.  Every index is checked against the
// number of units / pixels.
template <int CT, bool VEC>
__global__ __launch_bounds__(UBK_BLOCK) void dice_fwd_kernel(const float* __restrict__ pred, const long long* __restrict__ target,
                                                             const float* __restrict__ pw, int C, long hw, long total,
                                                             long long ignore_index, u64* __restrict__ rows) {
  constexpr int CM = CT ? CT : UBK_MAX_CLASSES;
  __shared__ u64 wave_row[UBK_BLOCK / 64][UBK_ROW_WORDS];
  const int lane = threadIdx.x;
  if (CT) C = CT;
  Lane<CM> a;
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    a.tp[c] = 0.0;
    a.fp[c] = 0.0;
    a.fn[c] = 0.0;
    a.n[c] = 0u;
  }
  a.bad = 0u;
  const long trips = (total + UBK_TRIP_PIXELS - 1) / UBK_TRIP_PIXELS;
  for (long trip = blockIdx.x; trip < trips; trip += gridDim.x) {
    if (VEC) {
      const long units = total / 4;
      const long base = trip * UBK_TRIP_UNITS + lane;
      ll2 T[UBK_UNROLL][2];
      float4 P[UBK_UNROLL];
      float4 X[UBK_UNROLL][CM];
#pragma unroll
      for (int u = 0; u < UBK_UNROLL; ++u) {
        const long i = base + u * UBK_BLOCK;
        const bool in = i < units;
        T[u][0] = in ? *(const ll2*)(target + 4 * i) : (ll2){ignore_index, ignore_index};
        T[u][1] = in ? *(const ll2*)(target + 4 * i + 2) : (ll2){ignore_index, ignore_index};
        P[u] = in ? *(const float4*)(pw + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
        const long p0 = 4 * i, n = p0 / hw, r = p0 - n * hw;
        const float* src = pred + n * C * hw + r;
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (CT || c < C) X[u][c] = in ? *(const float4*)(src + c * hw) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < UBK_UNROLL; ++u) {
        const bool in = base + u * UBK_BLOCK < units;
        const float pv[4] = {P[u].x, P[u].y, P[u].z, P[u].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const long long t = T[u][k >> 1][k & 1];
          const bool ok = in && contributes(t, C, ignore_index);
          if (in && t != ignore_index && !ok) a.bad += 1u;
          float lp[CM];
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (CT || c < C) lp[c] = k == 0 ? X[u][c].x : (k == 1 ? X[u][c].y : (k == 2 ? X[u][c].z : X[u][c].w));
          take<CT, CM>(a, C, t, ok, pv[k], lp);
        }
      }
    } else {
      const long base = trip * UBK_TRIP_PIXELS + lane;
      long long T[4 * UBK_UNROLL];
      float P[4 * UBK_UNROLL];
      float X[4 * UBK_UNROLL][CM];
#pragma unroll
      for (int j = 0; j < 4 * UBK_UNROLL; ++j) {
        const long p = base + j * UBK_BLOCK;
        const bool in = p < total;
        T[j] = in ? target[p] : ignore_index;
        P[j] = in ? pw[p] : 0.f;
        const long n = p / hw, r = p - n * hw;
        const float* src = pred + n * C * hw + r;
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (CT || c < C) X[j][c] = in ? src[c * hw] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4 * UBK_UNROLL; ++j) {
        const bool in = base + j * UBK_BLOCK < total;
        const bool ok = in && contributes(T[j], C, ignore_index);
        if (in && T[j] != ignore_index && !ok) a.bad += 1u;
        take<CT, CM>(a, C, T[j], ok, P[j], X[j]);
      }
    }
  }
  // the lanes of a wave in the fixed order of the shuffle tree, then the four waves in order; classes >= C stay 0
  const int wave = lane >> 6;
  for (int i = lane; i < (UBK_BLOCK / 64) * UBK_ROW_WORDS; i += UBK_BLOCK) (&wave_row[0][0])[i] = 0ull;
  __syncthreads();
  u64 valid = 0ull;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (CT || c < C) {
      const double tp = wave_sum(a.tp[c]), fp = wave_sum(a.fp[c]), fn = wave_sum(a.fn[c]);
      const u64 n = wave_sum((u64)a.n[c]);
      valid += n;
      if ((lane & 63) == 0) {
        wave_row[wave][UBK_ROW_TP + c] = (u64)__double_as_longlong(tp);
        wave_row[wave][UBK_ROW_FP + c] = (u64)__double_as_longlong(fp);
        wave_row[wave][UBK_ROW_FN + c] = (u64)__double_as_longlong(fn);
        wave_row[wave][UBK_ROW_PIXELS + c] = n;
      }
    }
  const u64 bad = wave_sum((u64)a.bad);
  if ((lane & 63) == 0) {
    wave_row[wave][UBK_ROW_VALID] = valid;
    wave_row[wave][UBK_ROW_BAD] = bad;
  }
  __syncthreads();
  if (lane < UBK_ROW_WORDS)
    rows[(long)blockIdx.x * UBK_ROW_WORDS + lane] = add_wave_rows(wave_row, lane, lane >= UBK_ROW_PIXELS);
}

// One workgroup: lane (q, word) adds word `word` of the rows q, q + 8, q + 16, .. in that order; then lane `word` adds the 8
// sequences in order.  The same rows give the same bits.  Then S in class order, the classes side by side, the loss in class order.
__global__ __launch_bounds__(UBK_FINISH_BLOCK) void dice_finish_kernel(const u64* __restrict__ rows, int nrows, const float* __restrict__ cw,
                                                                       int C, float alpha, float beta, float eps, int present_only,
                                                                       u64* __restrict__ ctl, float* __restrict__ loss) {
  __shared__ u64 sub[UBK_FINISH_SUB][UBK_ROW_WORDS];
  __shared__ u64 tot[UBK_ROW_WORDS];
  __shared__ double term[UBK_MAX_CLASSES];
  __shared__ double S_all;
  const int tid = threadIdx.x;
  const int word = tid % UBK_ROW_WORDS, q = tid / UBK_ROW_WORDS;
  const bool integer = word >= UBK_ROW_PIXELS;
  if (tid < UBK_FINISH_LANES) sub[q][word] = sequence_sum<UBK_FINISH_SUB, UBK_ROW_WORDS>(rows, nrows, q, word, integer);
  __syncthreads();
  if (tid < UBK_ROW_WORDS) {
    const u64 out = sequences_sum(sub, word, integer);
    tot[word] = out;
    ctl[word] = out;          // ctl words 0 .. 65 are the row words
  }
  __syncthreads();
  if (tid == 0) {
    double S = 0.0;
    for (int c = 0; c < C; ++c) {
      const bool present = !present_only || tot[UBK_ROW_PIXELS + c] > 0ull;
      S += present ? (double)(cw ? cw[c] : 1.f) : 0.0;
    }
    S_all = S;
    ctl[UBK_CTL_S] = (u64)__double_as_longlong(S);
  }
  __syncthreads();
  if (tid < UBK_MAX_CLASSES) {
    const int c = tid;
    ubk::Class r = {0.0, 0.0, 0.f, 0.f};
    if (c < C) {
      const double S = S_all;
      const bool present = !present_only || tot[UBK_ROW_PIXELS + c] > 0ull;
      const double a = (present && S != 0.0) ? (double)(cw ? cw[c] : 1.f) / S : 0.0;
      r = ubk::finish_class(S != 0.0, a, __longlong_as_double((long long)tot[UBK_ROW_TP + c]),
                            __longlong_as_double((long long)tot[UBK_ROW_FP + c]), __longlong_as_double((long long)tot[UBK_ROW_FN + c]),
                            (double)alpha, (double)beta, (double)eps);
    }
    term[c] = r.term;
    ctl[UBK_CTL_T + c] = (u64)__double_as_longlong(r.T);
    ctl[UBK_CTL_K1 + c] = (u64)__float_as_uint(r.k1);
    ctl[UBK_CTL_K0 + c] = (u64)__float_as_uint(r.k0);
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += term[c];
    const float l = (float)s;
    ctl[UBK_CTL_LOSS] = (u64)__float_as_uint(l);
    *loss = l;
  }
}

// The backward: the walk of the forward.  Every channel of every pixel is written: VEC as one 16-byte load and one 16-byte store
// per channel and unit, otherwise one float per channel and pixel.  K1 and K0 are read from the control block at addresses that
// are the same for every lane.
template <bool VEC>
__global__ __launch_bounds__(UBK_BLOCK) void dice_bwd_kernel(const float* __restrict__ gloss, const float* __restrict__ ctlf,
                                                             const float* __restrict__ pred, const long long* __restrict__ target,
                                                             const float* __restrict__ pw, int C, long hw, long total,
                                                             long long ignore_index, float* __restrict__ gpred) {
  const int lane = threadIdx.x;
  const float gl = *gloss;
  const float* __restrict__ K1 = ctlf + 2 * UBK_CTL_K1;      // (the low 4 bytes of 8-byte words)
  const float* __restrict__ K0 = ctlf + 2 * UBK_CTL_K0;
  const long trips = (total + UBK_TRIP_PIXELS - 1) / UBK_TRIP_PIXELS;
  for (long trip = blockIdx.x; trip < trips; trip += gridDim.x) {
    if (VEC) {
      const long units = total / 4;
      const long base = trip * UBK_TRIP_UNITS + lane;
      ll2 T[UBK_UNROLL][2];
      float4 P[UBK_UNROLL];
#pragma unroll
      for (int u = 0; u < UBK_UNROLL; ++u) {
        const long i = base + u * UBK_BLOCK;
        const bool in = i < units;
        T[u][0] = in ? *(const ll2*)(target + 4 * i) : (ll2){ignore_index, ignore_index};
        T[u][1] = in ? *(const ll2*)(target + 4 * i + 2) : (ll2){ignore_index, ignore_index};
        P[u] = in ? *(const float4*)(pw + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < UBK_UNROLL; ++u) {
        const long i = base + u * UBK_BLOCK;
        if (i >= units) continue;
        const long p0 = 4 * i, n = p0 / hw, r = p0 - n * hw;
        const float pv[4] = {P[u].x, P[u].y, P[u].z, P[u].w};
        float s[4];
        int tc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const long long t = T[u][k >> 1][k & 1];
          tc[k] = contributes(t, C, ignore_index) ? (int)t : -1;
          s[k] = gl * pv[k];
        }
        const float* src = pred + n * C * hw + r;
        float* dst = gpred + n * C * hw + r;
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
          const float4 x = *(const float4*)(src + c * hw);
          const float k1 = K1[2 * c], k0 = K0[2 * c];
          float4 g;
          g.x = tc[0] < 0 ? 0.f : ubk::grad(s[0], x.x, tc[0] == c ? k1 : k0);
          g.y = tc[1] < 0 ? 0.f : ubk::grad(s[1], x.y, tc[1] == c ? k1 : k0);
          g.z = tc[2] < 0 ? 0.f : ubk::grad(s[2], x.z, tc[2] == c ? k1 : k0);
          g.w = tc[3] < 0 ? 0.f : ubk::grad(s[3], x.w, tc[3] == c ? k1 : k0);
          *(float4*)(dst + c * hw) = g;
        }
      }
    } else {
      const long base = trip * UBK_TRIP_PIXELS + lane;
      long long T[4 * UBK_UNROLL];
      float P[4 * UBK_UNROLL];
#pragma unroll
      for (int j = 0; j < 4 * UBK_UNROLL; ++j) {
        const long p = base + j * UBK_BLOCK;
        T[j] = p < total ? target[p] : ignore_index;
        P[j] = p < total ? pw[p] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4 * UBK_UNROLL; ++j) {
        const long p = base + j * UBK_BLOCK;
        if (p >= total) continue;
        const long n = p / hw, r = p - n * hw;
        const int tc = contributes(T[j], C, ignore_index) ? (int)T[j] : -1;
        const float s = gl * P[j];
        const float* src = pred + n * C * hw + r;
        float* dst = gpred + n * C * hw + r;
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
          const float x = src[c * hw];
          dst[c * hw] = tc < 0 ? 0.f : ubk::grad(s, x, tc == c ? K1[2 * c] : K0[2 * c]);
        }
      }
    }
  }
}

inline unsigned grid_of(long total) {
  long grid = (total + UBK_TRIP_PIXELS - 1) / UBK_TRIP_PIXELS;
  return (unsigned)(grid > UBK_MAX_GRID ? UBK_MAX_GRID : grid);
}

inline bool finite_nonneg(float v) { return v >= 0.f && v < INFINITY; }     // false for a NaN

template <int CT>
void launch_fwd(bool vec, unsigned grid, hipStream_t stream, const float* predict, const long long* target, const float* pixelweights, int C,
                long hw, long total, long long ignore_index, u64* rows) {
  if (vec)
    dice_fwd_kernel<CT, true><<<dim3(grid), dim3(UBK_BLOCK), 0, stream>>>(predict, target, pixelweights, C, hw, total, ignore_index, rows);
  else
    dice_fwd_kernel<CT, false><<<dim3(grid), dim3(UBK_BLOCK), 0, stream>>>(predict, target, pixelweights, C, hw, total, ignore_index, rows);
}

}  // namespace

// the checks the two calls share; `name` starts the message
#define UBK_CHECK_OPERANDS(name, predict, target, pixelweights, N, C, H, W)                                                      \
  SAT_CHECK((predict) && (target) && (pixelweights), name ": null pointer (predict, target, pixelweights)");                     \
  SAT_CHECK((N) > 0 && (H) > 0 && (W) > 0, name ": bad extents N=%d H=%d W=%d", (N), (H), (W));                                   \
  SAT_CHECK((C) >= 1 && (C) <= UBK_MAX_CLASSES, name ": C=%d must be in [1, %d]", (C), UBK_MAX_CLASSES);                          \
  SAT_CHECK(aligned((predict), 4) && aligned((pixelweights), 4) && aligned((target), 8),                                         \
            name ": predict and pixelweights must be 4-byte aligned, target 8-byte aligned")

extern "C" int ubk_dice_fwd(const float* predict, const int64_t* target, const float* pixelweights, const float* classw,
                            int N, int C, int H, int W, int64_t ignore_index, float alpha, float beta, float eps, int present_only,
                            void* workspace, void* ctl, float* loss, void* stream) {
  UBK_CHECK_OPERANDS("ubk_dice_fwd", predict, target, pixelweights, N, C, H, W);
  SAT_CHECK(workspace && ctl && loss, "ubk_dice_fwd: null pointer (workspace, ctl, loss)");
  SAT_CHECK(finite_nonneg(alpha), "ubk_dice_fwd: alpha=%g must be finite and >= 0", (double)alpha);
  SAT_CHECK(finite_nonneg(beta), "ubk_dice_fwd: beta=%g must be finite and >= 0", (double)beta);
  SAT_CHECK(finite_nonneg(eps), "ubk_dice_fwd: eps=%g must be finite and >= 0", (double)eps);
  SAT_CHECK(present_only == 0 || present_only == 1, "ubk_dice_fwd: present_only=%d must be 0 or 1", present_only);
  SAT_CHECK(aligned(classw, 4), "ubk_dice_fwd: classw must be 4-byte aligned");
  SAT_CHECK(aligned(workspace, 16), "ubk_dice_fwd: workspace must be 16-byte aligned");
  SAT_CHECK(aligned(ctl, 8) && aligned(loss, 4), "ubk_dice_fwd: ctl must be 8-byte aligned, loss 4-byte aligned");
  SAT_CHECK(!overlap(workspace, UBK_WORKSPACE_BYTES, ctl, UBK_CTL_BYTES), "ubk_dice_fwd: ctl overlaps workspace");
  SAT_CHECK(!overlap(workspace, UBK_WORKSPACE_BYTES, loss, 4), "ubk_dice_fwd: loss inside workspace");
  SAT_CHECK(!overlap(ctl, UBK_CTL_BYTES, loss, 4), "ubk_dice_fwd: loss inside ctl");
  const long hw = (long)H * W, total = (long)N * hw;
  const unsigned grid = grid_of(total);
  const bool vec = hw % 4 == 0 && aligned(predict, 16) && aligned(target, 16) && aligned(pixelweights, 16);
  const long long* t = (const long long*)target;
  const hipStream_t s = (hipStream_t)stream;
  switch (C <= UBK_REG_CLASSES ? C : 0) {
    case 1: launch_fwd<1>(vec, grid, s, predict, t, pixelweights, C, hw, total, (long long)ignore_index, (u64*)workspace); break;
    case 2: launch_fwd<2>(vec, grid, s, predict, t, pixelweights, C, hw, total, (long long)ignore_index, (u64*)workspace); break;
    case 3: launch_fwd<3>(vec, grid, s, predict, t, pixelweights, C, hw, total, (long long)ignore_index, (u64*)workspace); break;
    case 4: launch_fwd<4>(vec, grid, s, predict, t, pixelweights, C, hw, total, (long long)ignore_index, (u64*)workspace); break;
    default: launch_fwd<0>(vec, grid, s, predict, t, pixelweights, C, hw, total, (long long)ignore_index, (u64*)workspace); break;
  }
  SAT_LAUNCH_CHECK("ubk_dice_fwd");
  dice_finish_kernel<<<dim3(1), dim3(UBK_FINISH_BLOCK), 0, s>>>((const u64*)workspace, (int)grid, classw, C, alpha, beta, eps, present_only,
                                                               (u64*)ctl, loss);
  SAT_LAUNCH_CHECK("ubk_dice_fwd (finish)");
  return UBK_OK;
}

extern "C" int ubk_dice_bwd(const float* g_loss, const void* ctl, const float* predict, const int64_t* target, const float* pixelweights,
                            int N, int C, int H, int W, int64_t ignore_index, float* g_predict, void* stream) {
  UBK_CHECK_OPERANDS("ubk_dice_bwd", predict, target, pixelweights, N, C, H, W);
  SAT_CHECK(g_loss && ctl && g_predict, "ubk_dice_bwd: null pointer (g_loss, ctl, g_predict)");
  SAT_CHECK(aligned(ctl, 8) && aligned(g_loss, 4) && aligned(g_predict, 4),
            "ubk_dice_bwd: ctl must be 8-byte aligned, g_loss and g_predict 4-byte aligned");
  const long hw = (long)H * W, total = (long)N * hw;
  const unsigned long long gbytes = 4ull * (unsigned long long)total * (unsigned long long)C;
  SAT_CHECK(!overlap(g_predict, gbytes, predict, gbytes), "ubk_dice_bwd: g_predict overlaps predict");
  SAT_CHECK(!overlap(g_predict, gbytes, target, 8ull * (unsigned long long)total), "ubk_dice_bwd: g_predict overlaps target");
  SAT_CHECK(!overlap(g_predict, gbytes, pixelweights, 4ull * (unsigned long long)total), "ubk_dice_bwd: g_predict overlaps pixelweights");
  SAT_CHECK(!overlap(g_predict, gbytes, ctl, UBK_CTL_BYTES), "ubk_dice_bwd: g_predict overlaps ctl");
  SAT_CHECK(!overlap(g_predict, gbytes, g_loss, 4), "ubk_dice_bwd: g_predict overlaps g_loss");
  const unsigned grid = grid_of(total);
  const bool vec = hw % 4 == 0 && aligned(predict, 16) && aligned(target, 16) && aligned(pixelweights, 16) && aligned(g_predict, 16);
  if (vec)
    dice_bwd_kernel<true><<<dim3(grid), dim3(UBK_BLOCK), 0, (hipStream_t)stream>>>(g_loss, (const float*)ctl, predict, (const long long*)target,
                                                                                  pixelweights, C, hw, total, (long long)ignore_index, g_predict);
  else
    dice_bwd_kernel<false><<<dim3(grid), dim3(UBK_BLOCK), 0, (hipStream_t)stream>>>(g_loss, (const float*)ctl, predict, (const long long*)target,
                                                                                   pixelweights, C, hw, total, (long long)ignore_index, g_predict);
  SAT_LAUNCH_CHECK("ubk_dice_bwd");
  return UBK_OK;
}
