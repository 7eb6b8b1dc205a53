// libubresnet_calib.so: temperature calibration of the class scores (include/ubresnet_calib.h).  It links against none of the
// other libraries and shares ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream, there is no atomic
// operation and no workgroup waits for another.  The geometry is that of ../ubr_calib_plan.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>
#include "../../../include/ubresnet_calib.h"
#include "../ubr_calib_plan.h"
#include "../ubr_sat.h"

#define UBF_VERSION 1

SAT_RETURN_CODES(UBF);
SAT_EXPORTS(ubf, UBF_VERSION)
using namespace sat;

namespace {

using ubf::BLOCK;
using ubf::LANE_PIXELS;
using ubf::TRIP_UNITS;
using ubf::UNROLL;
using ubf::WAVES;
typedef unsigned long long u64;
typedef long long ll2 __attribute__((ext_vector_type(2)));

static_assert(ubf::MAX_TEMPS == UBF_MAX_TEMPS && ubf::MAX_GROUPS == UBF_MAX_GROUPS && ubf::MAX_CLASSES == UBF_MAX_CLASSES &&
              ubf::REG_CLASSES == UBF_REG_CLASSES && ubf::MAX_IMAGES == UBF_MAX_IMAGES, "the plan and the public header agree");
static_assert(ubf::MAX_TEMPS <= ubf::WAVE && 3 * ubf::MAX_TEMPS + 3 <= ubf::FINISH_WORDS && LANE_PIXELS == 4, "a lane per temperature");

constexpr int ROW_MAX = 3 * ubf::MAX_TEMPS + 3;
constexpr int NONE = 255;                                     // a truth that is not a class

__device__ __forceinline__ int class_of(uint8_t v, int C) { return (int)v < C ? (int)v : NONE; }
__device__ __forceinline__ int class_of(long long v, int C) { return (v >= 0ll && v < (long long)C) ? (int)v : NONE; }

__device__ __forceinline__ float comp(const float4& v, int q) { return q == 0 ? v.x : (q == 1 ? v.y : (q == 2 ? v.z : v.w)); }
__device__ __forceinline__ bool finite(float v) { return fabsf(v) < INFINITY; }     // false for a NaN

// the four truth values of a unit that starts at pixel p0 of the image; NONE-valued (255 is no class) past the image's end
__device__ __forceinline__ void load_truth(const uint8_t* t, long p0, long hw, bool vec, uint8_t (&out)[4]) {
  if (vec) {
    const unsigned w = p0 < hw ? *reinterpret_cast<const unsigned*>(t + p0) : 0xFFFFFFFFu;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = (uint8_t)((w >> (8 * q)) & 255u);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = p0 + q < hw ? t[p0 + q] : (uint8_t)NONE;
  }
}
__device__ __forceinline__ void load_truth(const long long* t, long p0, long hw, bool vec, long long (&out)[4]) {
  if (vec) {
    const ll2 a = p0 < hw ? *reinterpret_cast<const ll2*>(t + p0) : (ll2){-1ll, -1ll};
    const ll2 b = p0 < hw ? *reinterpret_cast<const ll2*>(t + p0 + 2) : (ll2){-1ll, -1ll};
    out[0] = a[0]; out[1] = a[1]; out[2] = b[0]; out[3] = b[1];
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = p0 + q < hw ? t[p0 + q] : -1ll;
  }
}

struct AccK {
  const float* scores;
  const void* truth;
  const float* lit;        // or null
  const float* betas;
  u64* rows;
  float thr;
  int C, K, vec;
  long hw, trips;
};

// The streaming pass of ubf_accumulate.  CT: the number of classes, or 0 for the runtime C (bounded by UBF_MAX_CLASSES).  Grid
// (gx, N); workgroup (x, n) walks trips x, x + gx, .. of image n.  A lane takes UNROLL units of four consecutive pixels per
// trip: the truth and lit loads of the trip are issued first, the scores of a unit are loaded only if one of its pixels counts
// and has a class for a truth (with CT, for all the trip's units before any is used; without, unit by unit).  Then, slot by
// slot, the wave visits its counted pixels in lane order: the pixel's d_c and d_t are broadcast from its lane and lane k adds
// the three terms at betas[k] to its fp64 sums.  Every index is checked against hw.
template <int CT, typename T>
__global__ __launch_bounds__(BLOCK) void accum_kernel(const AccK k) {
  constexpr int CM = CT ? CT : UBF_MAX_CLASSES;
  constexpr int UB = CT ? UNROLL : 1;
  __shared__ u64 wave_row[WAVES][ROW_MAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = CT ? CT : k.C, K = k.K;
  const long hw = k.hw, n = blockIdx.y;
  const bool vec = k.vec != 0;
  const float* scores = k.scores + n * C * hw;
  const T* truth = reinterpret_cast<const T*>(k.truth) + n * hw;
  const float* lit = k.lit ? k.lit + n * hw : nullptr;
  const float beta = lane < K ? k.betas[lane] : 1.f;
  double a_nll = 0.0, a_g = 0.0, a_h = 0.0;
  u64 n_cnt = 0ull, n_ign = 0ull, n_nf = 0ull;                // wave-uniform
  for (long trip = blockIdx.x; trip < k.trips; trip += gridDim.x) {
    T traw[UNROLL][4];
    float4 lv[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long p0 = (trip * TRIP_UNITS + u * BLOCK + tid) * LANE_PIXELS;
      load_truth(truth, p0, hw, vec, traw[u]);
      lv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lit) {
        if (vec) {
          if (p0 < hw) lv[u] = *reinterpret_cast<const float4*>(lit + p0);
        } else {
          if (p0 < hw) lv[u].x = lit[p0];
          if (p0 + 1 < hw) lv[u].y = lit[p0 + 1];
          if (p0 + 2 < hw) lv[u].z = lit[p0 + 2];
          if (p0 + 3 < hw) lv[u].w = lit[p0 + 3];
        }
      }
    }
    int cls[UNROLL][4];
    bool cnt[UNROLL][4], need[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long p0 = (trip * TRIP_UNITS + u * BLOCK + tid) * LANE_PIXELS;
      need[u] = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        cls[u][q] = class_of(traw[u][q], C);
        cnt[u][q] = p0 + q < hw && (!lit || comp(lv[u], q) > k.thr);
        need[u] = need[u] || (cnt[u][q] && cls[u][q] != NONE);
      }
    }
#pragma unroll
    for (int u0 = 0; u0 < UNROLL; u0 += UB) {
      float4 X[UB][CM];
#pragma unroll
      for (int b = 0; b < UB; ++b) {
        const int u = u0 + b;
        const long p0 = (trip * TRIP_UNITS + u * BLOCK + tid) * LANE_PIXELS;
#pragma unroll
        for (int c = 0; c < CM; ++c) {
          X[b][c] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (CT || c < C) {
            const float* src = scores + c * hw + p0;
            if (vec) {
              if (need[u]) X[b][c] = *reinterpret_cast<const float4*>(src);       // need: p0 < hw, and hw % 4 == 0
            } else {
              if (cnt[u][0] && cls[u][0] != NONE) X[b][c].x = src[0];
              if (cnt[u][1] && cls[u][1] != NONE) X[b][c].y = src[1];
              if (cnt[u][2] && cls[u][2] != NONE) X[b][c].z = src[2];
              if (cnt[u][3] && cls[u][3] != NONE) X[b][c].w = src[3];
            }
          }
        }
      }
#pragma unroll
      for (int b = 0; b < UB; ++b) {
        const int u = u0 + b;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool valid = cls[u][q] != NONE;
          if (__ballot(cnt[u][q]) == 0ull) continue;           // wave-uniform
          n_ign += (unsigned)__popcll(__ballot(cnt[u][q] && !valid));
          const bool ok = cnt[u][q] && valid;
          float d[CM];
          bool fin = true;
          float ml = comp(X[b][0], q);
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (CT || c < C) {
              d[c] = comp(X[b][c], q);
              fin = fin && finite(d[c]);
              ml = fmaxf(ml, d[c]);
            }
          float dt = 0.f;
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (CT || c < C) {
              d[c] = __fsub_rn(d[c], ml);
              dt = cls[u][q] == c ? d[c] : dt;
            }
          n_nf += (unsigned)__popcll(__ballot(ok && !fin));
          u64 rem = __ballot(ok && fin);
          n_cnt += (unsigned)__popcll(rem);
          while (rem != 0ull) {                                // wave-uniform: one trip per counted pixel of the slot, in lane order
            const int j = __ffsll((long long)rem) - 1;
            rem &= rem - 1ull;
            float dj[CM], e[CM];
            const float dtj = __shfl(dt, j);
            float S = 0.f, A = 0.f;
#pragma unroll
            for (int c = 0; c < CM; ++c)
              if (CT || c < C) {
                dj[c] = __shfl(d[c], j);
                e[c] = expf(__fmul_rn(beta, dj[c]));
                S = __fadd_rn(S, e[c]);
                A = __fadd_rn(A, __fmul_rn(e[c], dj[c]));
              }
            const float mean = __fdiv_rn(A, S);
            float V = 0.f;
#pragma unroll
            for (int c = 0; c < CM; ++c)
              if (CT || c < C) {
                const float r = __fsub_rn(dj[c], mean);
                V = __fadd_rn(V, __fmul_rn(e[c], __fmul_rn(r, r)));
              }
            a_nll += (double)__fsub_rn(logf(S), __fmul_rn(beta, dtj));
            a_g += (double)__fsub_rn(mean, dtj);
            a_h += (double)__fdiv_rn(V, S);
          }
        }
      }
    }
  }
  // lane k < K of every wave holds the sums of betas[k]; the four waves in order
  if (lane < K) {
    wave_row[wave][3 * lane + 0] = (u64)__double_as_longlong(a_nll);
    wave_row[wave][3 * lane + 1] = (u64)__double_as_longlong(a_g);
    wave_row[wave][3 * lane + 2] = (u64)__double_as_longlong(a_h);
  }
  if (lane == 0) {
    wave_row[wave][3 * K + 0] = n_cnt;
    wave_row[wave][3 * K + 1] = n_ign;
    wave_row[wave][3 * K + 2] = n_nf;
  }
  __syncthreads();
  const int words = 3 * K + 3;
  if (tid < words) {
    u64 out;
    if (tid >= 3 * K) {
      out = 0ull;
      for (int w = 0; w < WAVES; ++w) out += wave_row[w][tid];
    } else {
      double s = 0.0;
      for (int w = 0; w < WAVES; ++w) s += __longlong_as_double((long long)wave_row[w][tid]);
      out = (u64)__double_as_longlong(s);
    }
    k.rows[((long)blockIdx.y * gridDim.x + blockIdx.x) * words + tid] = out;
  }
}

// One workgroup.  Image by image in ascending n: lane (s, w) adds word w of the image's rows s, s + FINISH_SUB, .. in that
// order; after a barrier lane (0, w) adds the FINISH_SUB sequences in order and adds the sum onto the word of the image's group
// (ubf::host_finish of the plan is this loop on the host).  The same rows give the same bits.
__global__ __launch_bounds__(ubf::FINISH_BLOCK) void finish_kernel(const u64* __restrict__ rows, int N, int gx, int K, int G,
                                                                   const uint8_t* __restrict__ group, double* table, u64* counters) {
  __shared__ u64 sub[ubf::FINISH_SUB][ubf::FINISH_WORDS];
  const int w = threadIdx.x % ubf::FINISH_WORDS, s = threadIdx.x / ubf::FINISH_WORDS;
  const int words = 3 * K + 3;
  const bool integer = w >= 3 * K;
  for (int n = 0; n < N; ++n) {
    const int g = group[n];                                    // the same for every lane
    if (g >= G) continue;
    if (w < words) {
      u64 ai = 0ull;
      double ad = 0.0;
#pragma unroll 8
      for (int r = s; r < gx; r += ubf::FINISH_SUB) {
        const u64 v = rows[((long)n * gx + r) * words + w];
        ai += integer ? v : 0ull;
        ad += integer ? 0.0 : __longlong_as_double((long long)v);
      }
      sub[s][w] = integer ? ai : (u64)__double_as_longlong(ad);
    }
    __syncthreads();
    if (s == 0 && w < words) {
      if (integer) {
        u64 t = 0ull;
        for (int q = 0; q < ubf::FINISH_SUB; ++q) t += sub[q][w];
        counters[g * 3 + (w - 3 * K)] += t;
      } else {
        double t = 0.0;
        for (int q = 0; q < ubf::FINISH_SUB; ++q) t += __longlong_as_double((long long)sub[q][w]);
        table[(long)g * 3 * K + w] += t;
      }
    }
    __syncthreads();                                           // sub is free for the next image
  }
}

// one pixel of ubf_apply, in place in x[]: the rules of the header
template <int CT, int CM>
__device__ __forceinline__ void rescale(float (&x)[CM], int C, float beta) {
  bool bad = false;
  float m = x[0];
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (CT || c < C) {
      bad = bad || x[c] != x[c] || x[c] == INFINITY;
      m = fmaxf(m, x[c]);
    }
  if (bad) {
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (CT || c < C) x[c] = __uint_as_float(0x7FC00000u);
    return;
  }
  if (m == -INFINITY) return;                                  // all C are -inf: they stay
  float S = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (CT || c < C) {
      x[c] = __fmul_rn(beta, __fsub_rn(x[c], m));
      S = __fadd_rn(S, expf(x[c]));
    }
  const float L = logf(S);
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (CT || c < C) x[c] = __fsub_rn(x[c], L);
}

// ubf_apply.  The walk of ubr_tta.hip: a workgroup's trip is TRIP_UNITS consecutive units, workgroup g takes trips g,
// g + grid, ..  VEC: a unit is four consecutive pixels of one tile (th * tw % 4 == 0), C loads and C stores of 16 bytes; with
// CT the loads of both units of a lane are issued before any is used (2 CT loads of 16 bytes in flight per lane).  Otherwise a
// unit is one pixel.  A lane reads all C values of a pixel before it writes any, and no other lane touches them: out == in is safe.
template <int CT, bool VEC>
__global__ __launch_bounds__(BLOCK) void apply_kernel(const float* in, float* out, const float* __restrict__ betas, int C, long hw,
                                                      long nunits) {
  constexpr int CM = CT ? CT : UBF_MAX_CLASSES;
  constexpr int UB = CT ? UNROLL : 1;
  typedef typename std::conditional<VEC, float4, float>::type U;
  constexpr int UP = VEC ? LANE_PIXELS : 1;
  if (CT) C = CT;
  const long trips = (nunits + TRIP_UNITS - 1) / TRIP_UNITS;
  for (long trip = blockIdx.x; trip < trips; trip += gridDim.x) {
#pragma unroll
    for (int u0 = 0; u0 < UNROLL; u0 += UB) {
      U X[UB][CM];
      float beta[UB];
      long at[UB];
#pragma unroll
      for (int b = 0; b < UB; ++b) {
        const long i = trip * TRIP_UNITS + (long)(u0 + b) * BLOCK + threadIdx.x;
        const bool in_range = i < nunits;
        const long p0 = i * UP, tile = in_range ? p0 / hw : 0, r = p0 - tile * hw;
        at[b] = tile * C * hw + r;
        beta[b] = in_range ? betas[tile] : 1.f;
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (CT || c < C) {
            if (in_range) X[b][c] = *reinterpret_cast<const U*>(in + at[b] + c * hw);
          }
      }
#pragma unroll
      for (int b = 0; b < UB; ++b) {
        const long i = trip * TRIP_UNITS + (long)(u0 + b) * BLOCK + threadIdx.x;
        if (i >= nunits) continue;
        if constexpr (VEC) {
          float px[4][CM];
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (CT || c < C) { px[0][c] = X[b][c].x; px[1][c] = X[b][c].y; px[2][c] = X[b][c].z; px[3][c] = X[b][c].w; }
#pragma unroll
          for (int q = 0; q < 4; ++q) rescale<CT, CM>(px[q], C, beta[b]);
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (CT || c < C) *reinterpret_cast<float4*>(out + at[b] + c * hw) = make_float4(px[0][c], px[1][c], px[2][c], px[3][c]);
        } else {
          float px[CM];
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (CT || c < C) px[c] = X[b][c];
          rescale<CT, CM>(px, C, beta[b]);
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (CT || c < C) out[at[b] + c * hw] = px[c];
        }
      }
    }
  }
}

template <int CT>
void launch_accum(int truth_kind, dim3 grid, hipStream_t stream, const AccK& k) {
  if (truth_kind == UBF_TRUTH_U8)
    accum_kernel<CT, uint8_t><<<grid, dim3(BLOCK), 0, stream>>>(k);
  else
    accum_kernel<CT, long long><<<grid, dim3(BLOCK), 0, stream>>>(k);
}

template <int CT>
void launch_apply(bool vec, unsigned grid, hipStream_t stream, const float* in, float* out, const float* betas, int C, long hw, long nunits) {
  if (vec)
    apply_kernel<CT, true><<<dim3(grid), dim3(BLOCK), 0, stream>>>(in, out, betas, C, hw, nunits);
  else
    apply_kernel<CT, false><<<dim3(grid), dim3(BLOCK), 0, stream>>>(in, out, betas, C, hw, nunits);
}

}  // namespace

extern "C" int64_t ubf_scratch_bytes(int N, int H, int W, int K) {
  ubf::Plan p;
  if (!ubf::make_plan(N, H, W, K, &p)) {
    set_error("ubf_scratch_bytes: N=%d must be 1..%d, H=%d and W=%d >= 1, N * H * W at most 2^40, K=%d must be 1..%d", N, UBF_MAX_IMAGES,
              H, W, K, UBF_MAX_TEMPS);
    return 0;
  }
  return p.scratch_bytes;
}

extern "C" int ubf_accumulate(const float* scores, const void* truth, int truth_kind, const float* lit, float lit_threshold,
                              const uint8_t* group, const float* betas, int K, int N, int C, int H, int W, int G,
                              double* table, unsigned long long* counters, void* scratch, int64_t scratch_bytes, void* stream) {
  // the scalar arguments first, the pointers last: a refusal names the first thing that is wrong with the call
  SAT_CHECK(truth_kind == UBF_TRUTH_U8 || truth_kind == UBF_TRUTH_I64, "ubf_accumulate: truth_kind=%d must be %d (uint8) or %d (int64)",
            truth_kind, UBF_TRUTH_U8, UBF_TRUTH_I64);
  SAT_CHECK(K >= 1 && K <= UBF_MAX_TEMPS, "ubf_accumulate: K=%d must be 1..%d", K, UBF_MAX_TEMPS);
  SAT_CHECK(C >= 1 && C <= UBF_MAX_CLASSES, "ubf_accumulate: C=%d must be 1..%d", C, UBF_MAX_CLASSES);
  SAT_CHECK(G >= 1 && G <= UBF_MAX_GROUPS, "ubf_accumulate: G=%d must be 1..%d", G, UBF_MAX_GROUPS);
  SAT_CHECK(lit_threshold == lit_threshold, "ubf_accumulate: lit_threshold is NaN");
  ubf::Plan p;
  SAT_CHECK(ubf::make_plan(N, H, W, K, &p), "ubf_accumulate: N=%d must be 1..%d, H=%d and W=%d >= 1, N * H * W at most 2^40", N,
            UBF_MAX_IMAGES, H, W);
  SAT_CHECK(scores && truth && group && betas, "ubf_accumulate: null pointer (scores %p, truth %p, group %p, betas %p)", (const void*)scores,
            truth, (const void*)group, (const void*)betas);
  SAT_CHECK(table && counters && scratch, "ubf_accumulate: null pointer (table %p, counters %p, scratch %p)", (void*)table, (void*)counters,
            scratch);
  SAT_CHECK(scratch_bytes >= p.scratch_bytes, "ubf_accumulate: scratch_bytes=%lld is short of the %lld that ubf_scratch_bytes counts",
            (long long)scratch_bytes, (long long)p.scratch_bytes);
  SAT_CHECK(aligned(scores, 4) && aligned(lit, 4) && aligned(betas, 4), "ubf_accumulate: scores, lit and betas must be 4-byte aligned");
  SAT_CHECK(truth_kind == UBF_TRUTH_U8 || aligned(truth, 8), "ubf_accumulate: an int64 truth must be 8-byte aligned");
  SAT_CHECK(aligned(table, 8) && aligned(counters, 8) && aligned(scratch, 8), "ubf_accumulate: table, counters and scratch must be 8-byte aligned");
  const unsigned long long pixels = (unsigned long long)N * (unsigned long long)p.hw;
  const unsigned long long tbytes = 8ull * 3ull * (unsigned long long)K * (unsigned long long)G, cbytes = 24ull * (unsigned long long)G;
  const unsigned long long sbytes = (unsigned long long)p.scratch_bytes;
  SAT_CHECK(!overlap(table, tbytes, counters, cbytes) && !overlap(table, tbytes, scratch, sbytes) && !overlap(counters, cbytes, scratch, sbytes),
            "ubf_accumulate: two of table, counters and scratch overlap");
  const void* outs[3] = {table, counters, scratch};
  const unsigned long long obytes[3] = {tbytes, cbytes, sbytes};
  for (int o = 0; o < 3; ++o)
    SAT_CHECK(!overlap(outs[o], obytes[o], scores, 4ull * pixels * (unsigned long long)C) &&
                  !overlap(outs[o], obytes[o], truth, (truth_kind == UBF_TRUTH_U8 ? 1ull : 8ull) * pixels) &&
                  !overlap(outs[o], obytes[o], lit, 4ull * pixels) && !overlap(outs[o], obytes[o], group, (unsigned long long)N) &&
                  !overlap(outs[o], obytes[o], betas, 4ull * (unsigned long long)K),
              "ubf_accumulate: %s overlaps an input", o == 0 ? "table" : (o == 1 ? "counters" : "scratch"));
  AccK k{};
  k.scores = scores; k.truth = truth; k.lit = lit; k.betas = betas; k.rows = (u64*)scratch;
  k.thr = lit_threshold; k.C = C; k.K = K; k.hw = (long)p.hw; k.trips = (long)p.trips;
  k.vec = p.hw % LANE_PIXELS == 0 && aligned(scores, 16) && aligned(lit, 16) && aligned(truth, truth_kind == UBF_TRUTH_U8 ? 4 : 16);
  const dim3 grid((unsigned)p.gx, (unsigned)N);
  const hipStream_t s = (hipStream_t)stream;
  switch (C <= UBF_REG_CLASSES ? C : 0) {
    case 1: launch_accum<1>(truth_kind, grid, s, k); break;
    case 2: launch_accum<2>(truth_kind, grid, s, k); break;
    case 3: launch_accum<3>(truth_kind, grid, s, k); break;
    case 4: launch_accum<4>(truth_kind, grid, s, k); break;
    default: launch_accum<0>(truth_kind, grid, s, k); break;
  }
  SAT_LAUNCH_CHECK("ubf_accumulate");
  finish_kernel<<<dim3(1), dim3(ubf::FINISH_BLOCK), 0, s>>>((const u64*)scratch, N, (int)p.gx, K, G, group, table, (u64*)counters);
  SAT_LAUNCH_CHECK("ubf_accumulate (finish)");
  return UBF_OK;
}

extern "C" int ubf_apply(const float* in, float* out, const float* betas, int n, int C, int th, int tw, void* stream) {
  SAT_CHECK(C >= 1 && C <= UBF_MAX_CLASSES, "ubf_apply: C=%d must be 1..%d", C, UBF_MAX_CLASSES);
  ubf::ApplyPlan p;
  SAT_CHECK(ubf::make_apply_plan(n, th, tw, false, &p) && p.units <= ubf::MAX_PIXELS / C,
            "ubf_apply: n=%d, th=%d and tw=%d must be >= 1 and n * C * th * tw at most 2^40", n, th, tw);
  SAT_CHECK(in && out && betas, "ubf_apply: null pointer (in %p, out %p, betas %p)", (const void*)in, (void*)out, (const void*)betas);
  SAT_CHECK(aligned(in, 4) && aligned(out, 4) && aligned(betas, 4), "ubf_apply: in, out and betas must be 4-byte aligned");
  const unsigned long long bytes = 4ull * (unsigned long long)p.units * (unsigned long long)C;
  SAT_CHECK((const float*)out == in || !overlap(in, bytes, out, bytes), "ubf_apply: out overlaps in without being in");
  SAT_CHECK(!overlap(out, bytes, betas, 4ull * (unsigned long long)n), "ubf_apply: out overlaps betas");
  const long hw = (long)th * tw;
  const bool vec = hw % LANE_PIXELS == 0 && aligned(in, 16) && aligned(out, 16);
  ubf::make_apply_plan(n, th, tw, vec, &p);
  const hipStream_t s = (hipStream_t)stream;
  switch (C <= UBF_REG_CLASSES ? C : 0) {
    case 1: launch_apply<1>(vec, (unsigned)p.grid, s, in, out, betas, C, hw, (long)p.units); break;
    case 2: launch_apply<2>(vec, (unsigned)p.grid, s, in, out, betas, C, hw, (long)p.units); break;
    case 3: launch_apply<3>(vec, (unsigned)p.grid, s, in, out, betas, C, hw, (long)p.units); break;
    case 4: launch_apply<4>(vec, (unsigned)p.grid, s, in, out, betas, C, hw, (long)p.units); break;
    default: launch_apply<0>(vec, (unsigned)p.grid, s, in, out, betas, C, hw, (long)p.units); break;
  }
  SAT_LAUNCH_CHECK("ubf_apply");
  return UBF_OK;
}
