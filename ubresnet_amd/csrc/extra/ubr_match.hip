// libubresnet_match.so: clusters of different wire planes matched by their time profiles (include/ubresnet_match.h).  It links
// against none of the other libraries and shares ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream.
// Limits, time bins, chunks, the tile enumeration, the scratch layout and the bounds come from ../ubr_match_plan.h, which
// tests/match_host.cpp runs on the host; trip, grid and span of the profile launch from ../ubr_walk_plan.h; the id load, the wave
// round and the trip loop from ../ubr_walk.h, the weight of a pixel from ../ubr_adc_rule.h, the wave sums and the workgroup scan
// from ../ubr_wave.h.
//
// Loops and their bounds ("PlaneMatch"):
//   the clear strides over lengths the host computed; the select makes at most select_trips trips and ends where the clusters do
//   the trip loop of the profile (walk::trip_loop) runs over the host-computed span; it has no LDS table, so its flush is empty
//   a wave round (walk::wave_round) ends after one trip per distinct (candidate, bin) among its lanes
//   the summary and the match make `chunks` trips over the bins; the match passes over the chunks outside both hulls
//   tile_of makes at most `tiles` trips
// No loop reads a word to wait for another workgroup's store.
#include <hip/hip_runtime.h>
#include "../../../include/ubresnet_match.h"
#include "../ubr_match_plan.h"
#include "../ubr_adc_rule.h"
#include "../ubr_sat.h"
#include "../ubr_walk.h"

#define UBU_VERSION 1

SAT_RETURN_CODES(UBU);
SAT_EXPORTS(ubu, UBU_VERSION)
using namespace sat;

static_assert(ubu::LANES == UBU_LANES && ubu::TRIP_PIXELS == UBU_TRIP_PIXELS && ubu::MAX_GRID == UBU_MAX_GRID && ubu::TILE == UBU_TILE &&
                  ubu::CHUNK_BINS == UBU_CHUNK_BINS && ubu::MIN_PLANES == UBU_MIN_PLANES && ubu::MAX_PLANES == UBU_MAX_PLANES &&
                  ubu::MIN_SLOTS == UBU_MIN_SLOTS && ubu::MAX_SLOTS == UBU_MAX_SLOTS && ubu::MAX_TIME_BIN == UBU_MAX_TIME_BIN &&
                  ubu::MAX_SHIFT == UBU_MAX_SHIFT && ubu::MAX_ROWS == UBU_MAX_ROWS && ubu::MAX_COLS == UBU_MAX_COLS &&
                  ubu::MAX_PLANE_PIXELS == UBU_MAX_PLANE_PIXELS && ubu::MAX_BIN_PIXELS == UBU_MAX_BIN_PIXELS &&
                  ubu::MAX_CLASSES == UBU_MAX_CLASSES && ubu::CLUSTER_FIXED == UBU_CLUSTER_FIXED && ubu::CAND_COLUMNS == UBU_CAND_COLUMNS &&
                  ubu::PAIR_COLUMNS == UBU_PAIR_COLUMNS && ubu::MAX_WEIGHT == UBU_MAX_WEIGHT && ubu::MAX_SCALE == UBU_MAX_SCALE,
              "the plan is the geometry of the public header");
static_assert(ubu::LANE_PIXELS == 4 && ubu::WAVE == 64 && ubu::WAVES == 4 && ubu::LANE_TILE == 4 && ubu::CAND_COLUMNS == 6 && ubu::PAIR_COLUMNS == 4,
              "the kernels unroll four pixels per lane, a 4 x 4 block of pairs per lane, six and four columns");

namespace {

typedef unsigned long long u64;
constexpr int TILE = ubu::TILE;
constexpr int STRIDE = ubu::STRIP_STRIDE;

struct MatK {
  const int32_t* ids;
  const long long* clusters;
  const u64* count;
  const float* view;
  unsigned* profile;     // [S][T]
  unsigned* occ;         // [S][T] in scratch: pixels per bin
  u64* mask;             // [S][chunks] in scratch: bit b of word c is set where bin 64 c + b holds a pixel
  int* slot_of;          // [rows_max] in scratch
  long long* cand;       // [S][6]
  long long* pairs;      // [S][S][4]
  u64* ncand;
  u64* status;
  u64 rows_max;
  long long min_pixels;
  float scale;
  int width, log2_bin, tiles;
  int shift[ubu::MAX_PLANES];
  unsigned pixels, rc, rows, cols, T, chunks, S;
  unsigned trips, span, select_trips;
};

// ---- launch 1 ----
__global__ __launch_bounds__(UBU_LANES) void clear_kernel(const MatK a) {
  const u64 bins = (u64)a.S * a.T, cells = (u64)a.S * UBU_CAND_COLUMNS, step = (u64)gridDim.x * UBU_LANES;
  for (u64 i = (u64)blockIdx.x * UBU_LANES + threadIdx.x; i < bins; i += step) {
    a.profile[i] = 0u;
    a.occ[i] = 0u;
  }
  for (u64 i = (u64)blockIdx.x * UBU_LANES + threadIdx.x; i < cells; i += step) a.cand[i] = 0ll;
}

// ---- launch 2: one workgroup ----
__global__ __launch_bounds__(UBU_LANES) void select_kernel(const MatK a) {
  __shared__ unsigned s_wave[ubu::WAVES];
  u64 n = *a.count;
  if (n > a.rows_max) n = a.rows_max;
  unsigned carry = 0u;                                            // candidates before this trip: at most rows_max < 2^31
  for (unsigned t = 0; t < a.select_trips; ++t) {                 // workgroup-uniform
    if ((u64)t * UBU_LANES >= n) break;                           // the clusters end here: slot_of at or past n is never read
    const u64 k = (u64)t * UBU_LANES + threadIdx.x;
    bool cand = false;
    long long root = 0;
    if (k < n) {
      const long long* row = a.clusters + k * (u64)a.width;
      cand = row[1] >= a.min_pixels;
      root = row[0];
    }
    unsigned total;
    const unsigned slot = carry + wv::block_scan<ubu::WAVES>(cand ? 1u : 0u, s_wave, &total) - 1u;
    const bool kept = cand && slot < a.S;
    if (k < n) a.slot_of[k] = kept ? (int)slot : -1;
    if (kept) {
      a.cand[(u64)slot * UBU_CAND_COLUMNS + 0] = (long long)k;
      a.cand[(u64)slot * UBU_CAND_COLUMNS + 1] = root / (long long)a.rc;
    }
    carry += total;
    __syncthreads();                                              // s_wave is written again in the next trip
  }
  if (threadIdx.x == 0) {
    *a.ncand = (u64)carry;
    if (carry > a.S) atomicAdd(a.status, (u64)(carry - a.S));
  }
}

// ---- launch 3 ----
// One wave round: every lane brings the weight `w` and the pixel count `cnt` of its pixels of bin `key` = slot * T + t (-1: none)
__device__ __forceinline__ void bin_round(const MatK& a, int key, unsigned w, unsigned cnt) {
  walk::wave_round(key, key >= 0, [&](const wv::KeyGroup<int>& g, int lane) {
    const unsigned tw = wv::sum_all(g.member ? w : 0u), tc = wv::sum_all(g.member ? cnt : 0u);
    if (lane == g.leader) {
      if (tw != 0u) atomicAdd(a.profile + g.key, tw);
      atomicAdd(a.occ + g.key, tc);
    }
  }, [&] {
    if (w != 0u) atomicAdd(a.profile + key, w);
    atomicAdd(a.occ + key, cnt);
  });
}

// the four pixels q .. q + 3 of a lane, whose cluster numbers are k4; `dropped` counts the lane's pixels that row_shift pushed out
__device__ __forceinline__ void lane_pixels(const MatK& a, unsigned q, const int4 k4, u64 nrows, unsigned& dropped) {
  const int k[4] = {k4.x, k4.y, k4.z, k4.w};
  int slot[4];
  unsigned lit = 0u;                                              // bit j: pixel q + j belongs to a candidate
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    slot[j] = (k[j] >= 0 && (u64)k[j] < nrows) ? a.slot_of[k[j]] : -1;
    lit |= (unsigned)(slot[j] >= 0) << j;
  }
  if (__ballot(lit != 0u) == 0ull) return;                        // wave-uniform
  int key[4] = {-1, -1, -1, -1};
  unsigned w[4] = {0u, 0u, 0u, 0u};
  int first = -1;
  bool mixed = false;
  if (lit != 0u) {
    float v[4];
    if (q + 3u < a.pixels) {                                      // q is a multiple of four: the load is aligned
      const float4 v4 = *(const float4*)(a.view + q);
      v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = q + (unsigned)j < a.pixels ? a.view[q + j] : 0.0f;
    }
    unsigned plane = q / a.rc;
    const unsigned o = q - plane * a.rc;
    unsigned yy = o / a.cols, xx = o - yy * a.cols;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned y = yy, pl = plane;
      if (++xx == a.cols) {                                       // the next pixel starts a row, or a plane
        xx = 0u;
        if (++yy == a.rows) {
          yy = 0u;
          ++plane;
        }
      }
      if (!((lit >> j) & 1u)) continue;                           // a pixel past the end of the image is not lit: pl < P below
      const int shifted = (int)y + a.shift[pl];
      if (shifted < 0 || shifted >= (int)a.rows) {
        ++dropped;
        continue;
      }
      key[j] = slot[j] * (int)a.T + (shifted >> a.log2_bin);      // t < T: shifted < rows
      w[j] = adc::weight_of(v[j], a.scale).w;
      if (first < 0) first = key[j];
      else mixed = mixed || key[j] != first;
    }
  }
  if (__ballot(mixed) == 0ull) {                                  // wave-uniform: every lane's pixels are of one bin
    unsigned cnt = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt += key[j] >= 0 ? 1u : 0u;
    bin_round(a, first, w[0] + w[1] + w[2] + w[3], cnt);          // w is 0 where the pixel takes no part
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) bin_round(a, key[j], w[j], 1u);
  }
}

__global__ __launch_bounds__(UBU_LANES) void profile_kernel(const MatK a) {
  __shared__ unsigned s_none;                                     // the walk's count of taken LDS slots: there is no LDS table here
  if (threadIdx.x == 0) s_none = 0u;
  __syncthreads();
  u64 nrows = *a.count;
  if (nrows > a.rows_max) nrows = a.rows_max;
  unsigned dropped = 0u;
  walk::trip_loop(a.trips, a.span, &s_none, 0u, [&](unsigned q) { return walk::load_ids(a.ids, q, a.pixels); },
                  [&](unsigned q, const int4& k4) { lane_pixels(a, q, k4, nrows, dropped); }, [] {});
  const unsigned d = wv::sum_all(dropped);                        // a lane walks fewer than 2^31 / 64 pixels
  if ((threadIdx.x & 63) == 0 && d != 0u) atomicAdd(a.status + 1, (u64)d);
}

// ---- launch 4: a wave per candidate ----
__global__ __launch_bounds__(UBU_LANES) void summary_kernel(const MatK a) {
  u64 n = *a.ncand;
  if (n > a.S) n = a.S;
  const unsigned lane = threadIdx.x & 63u, c = blockIdx.x * ubu::WAVES + (threadIdx.x >> 6);
  if (c >= n) return;                                             // wave-uniform; the kernel holds no barrier
  u64 q = 0ull;
  int bins = 0, t_min = (int)a.T, t_max = -1;
  for (unsigned ch = 0; ch < a.chunks; ++ch) {
    const unsigned t = ch * UBU_CHUNK_BINS + lane;
    unsigned p = 0u, o = 0u;
    if (t < a.T) {
      p = a.profile[(u64)c * a.T + t];
      o = a.occ[(u64)c * a.T + t];
    }
    q += p;
    const u64 m = __ballot(o != 0u);
    if (m != 0ull) {
      bins += __popcll(m);
      const int lo = (int)(ch * UBU_CHUNK_BINS) + __ffsll((long long)m) - 1, hi = (int)(ch * UBU_CHUNK_BINS) + 63 - __clzll((long long)m);
      t_min = lo < t_min ? lo : t_min;
      t_max = hi;                                                 // the chunks ascend
    }
    if (lane == 0u) a.mask[(u64)c * a.chunks + ch] = m;
  }
  q = wv::sum_all(q);
  if (lane == 0u) {
    long long* row = a.cand + (u64)c * UBU_CAND_COLUMNS;
    row[2] = (long long)q; row[3] = bins; row[4] = t_min; row[5] = t_max;
  }
}

// ---- launch 5: a workgroup per tile of the upper triangle ----
__global__ __launch_bounds__(UBU_LANES) void match_kernel(const MatK a) {
  __shared__ unsigned s_pi[TILE * STRIDE], s_pj[TILE * STRIDE];   // [candidate of the tile][bin of the chunk]
  __shared__ u64 s_mi[TILE], s_mj[TILE];
  __shared__ int s_plane[2 * TILE];
  __shared__ int s_hull[4];                                       // t_min, t_max of the i side, then of the j side
  u64 n = *a.ncand;
  if (n > a.S) n = a.S;
  int ti, tj;
  ubu::tile_of((int)blockIdx.x, a.tiles, &ti, &tj);
  const unsigned i0 = (unsigned)ti * TILE, j0 = (unsigned)tj * TILE;
  if (j0 >= n) return;                                            // workgroup-uniform; i0 <= j0
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (wave < 2u) {                                                // wave 0 reads the candidates of the i side, wave 1 those of the j side
    const unsigned c = (wave == 0u ? i0 : j0) + lane;
    int plane = -1, lo = 0x7FFFFFFF, hi = -1;
    if (c < n) {
      const long long* row = a.cand + (u64)c * UBU_CAND_COLUMNS;
      plane = (int)row[1]; lo = (int)row[4]; hi = (int)row[5];
    }
    s_plane[wave * TILE + lane] = plane;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0u) {
      s_hull[wave * 2u] = lo;
      s_hull[wave * 2u + 1u] = hi;
    }
  }
  __syncthreads();
  // the candidates ascend in plane: the tile lies in one plane where its first and its last candidate do
  const unsigned j_last = (unsigned)(n - 1ull - j0) < (unsigned)(TILE - 1) ? (unsigned)(n - 1ull - j0) : (unsigned)(TILE - 1);
  const bool one_plane = s_plane[0] == s_plane[TILE + j_last];
  const int lo = s_hull[0] > s_hull[2] ? s_hull[0] : s_hull[2], hi = s_hull[1] < s_hull[3] ? s_hull[1] : s_hull[3];
  const bool skip = one_plane || lo > hi;                         // workgroup-uniform
  const unsigned li = tid >> 4, lj = tid & 15u;                   // the lane's pairs: i0 + 4 li + x against j0 + 4 lj + y
  u64 sum_i[4][4], in_i[4][4], in_j[4][4];
  unsigned both[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      sum_i[x][y] = 0ull; in_i[x][y] = 0ull; in_j[x][y] = 0ull; both[x][y] = 0u;
    }
  if (!skip) {
    const unsigned c_lo = (unsigned)lo / UBU_CHUNK_BINS, c_hi = (unsigned)hi / UBU_CHUNK_BINS;   // 0 <= lo <= hi < T
    for (unsigned ch = 0; ch < a.chunks; ++ch) {                  // workgroup-uniform
      if (ch < c_lo || ch > c_hi) continue;
      const unsigned t = ch * UBU_CHUNK_BINS + lane;
#pragma unroll
      for (int r = 0; r < TILE / ubu::WAVES; ++r) {               // a wave stages one candidate's chunk per trip: i0 + c, j0 + c < S
        const unsigned c = wave + (unsigned)r * ubu::WAVES;
        s_pi[c * STRIDE + lane] = t < a.T ? a.profile[(u64)(i0 + c) * a.T + t] : 0u;
        s_pj[c * STRIDE + lane] = t < a.T ? a.profile[(u64)(j0 + c) * a.T + t] : 0u;
      }
      if (wave == 0u) s_mi[lane] = i0 + lane < n ? a.mask[(u64)(i0 + lane) * a.chunks + ch] : 0ull;
      if (wave == 1u) s_mj[lane] = j0 + lane < n ? a.mask[(u64)(j0 + lane) * a.chunks + ch] : 0ull;
      __syncthreads();
      u64 mi[4], mj[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        mi[x] = s_mi[li * 4u + x];
        mj[x] = s_mj[lj * 4u + x];
      }
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) both[x][y] += (unsigned)__popcll(mi[x] & mj[y]);
#pragma unroll 2
      for (int b = 0; b < UBU_CHUNK_BINS; ++b) {
        unsigned pi[4], pj[4], oi[4], oj[4];                      // oi, oj: all ones where the candidate occupies the bin
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          pi[x] = s_pi[(li * 4u + x) * STRIDE + b];
          pj[x] = s_pj[(lj * 4u + x) * STRIDE + b];
          oi[x] = 0u - (unsigned)((mi[x] >> b) & 1ull);
          oj[x] = 0u - (unsigned)((mj[x] >> b) & 1ull);
        }
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y) {
            sum_i[x][y] += pi[x] < pj[y] ? pi[x] : pj[y];
            in_i[x][y] += pi[x] & oj[y];
            in_j[x][y] += pj[y] & oi[x];
          }
      }
      __syncthreads();                                            // the strips are staged again in the next trip
    }
  }
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const unsigned i = i0 + li * 4u + x, j = j0 + lj * 4u + y;
      if (i >= j || j >= n) continue;                             // i < j < min(ncand, S): inside the table
      const bool zero = skip || s_plane[li * 4u + x] == s_plane[TILE + lj * 4u + y];
      ulonglong2* out = (ulonglong2*)(a.pairs + ((u64)i * a.S + j) * UBU_PAIR_COLUMNS);
      out[0] = zero ? make_ulonglong2(0ull, 0ull) : make_ulonglong2((u64)both[x][y], sum_i[x][y]);
      out[1] = zero ? make_ulonglong2(0ull, 0ull) : make_ulonglong2(in_i[x][y], in_j[x][y]);
    }
}

// the arguments both entry points check; the plan in *p
int check_geometry(const char* who, int P, int rows, int cols, int time_bin, int64_t slots, int64_t capacity, ubu::Plan* p) {
  const char* why;
  SAT_CHECK(ubu::make_plan(P, rows, cols, time_bin, slots, capacity, p, &why),
            "%s: P=%d, rows=%d, cols=%d, time_bin=%d, slots=%lld, capacity=%lld: %s", who, P, rows, cols, time_bin, (long long)slots,
            (long long)capacity, why);
  return 0;
}

}  // namespace

extern "C" int64_t ubu_scratch_bytes(int P, int rows, int cols, int time_bin, int64_t slots, int64_t capacity) {
  ubu::Plan p;
  if (check_geometry("ubu_scratch_bytes", P, rows, cols, time_bin, slots, capacity, &p) != 0) return 0;
  return p.scratch_bytes;
}

extern "C" int ubu_match(const int32_t* ids, const long long* clusters, int cluster_width, const unsigned long long* count, int64_t capacity,
                         const float* view, float adc_scale, int P, int rows, int cols, int64_t min_pixels, int time_bin,
                         const int* row_shift, int64_t slots, uint32_t* profile, long long* candidates, long long* pairs,
                         unsigned long long* ncand, unsigned long long* status, void* scratch, void* stream) {
  SAT_CHECK(cluster_width > UBU_CLUSTER_FIXED && cluster_width <= UBU_CLUSTER_FIXED + UBU_MAX_CLASSES,
            "ubu_match: cluster_width=%d must be %d + C for 1..%d classes", cluster_width, UBU_CLUSTER_FIXED, UBU_MAX_CLASSES);
  SAT_CHECK(ubu::valid_scale(adc_scale), "ubu_match: adc_scale=%g must be a power of two in 1..%d", (double)adc_scale, UBU_MAX_SCALE);
  SAT_CHECK(min_pixels >= 1, "ubu_match: min_pixels=%lld must be >= 1", (long long)min_pixels);
  ubu::Plan plan;
  if (check_geometry("ubu_match", P, rows, cols, time_bin, slots, capacity, &plan) != 0) return UBU_EINVAL;
  SAT_CHECK(row_shift, "ubu_match: null pointer (row_shift)");
  for (int p = 0; p < P; ++p)
    SAT_CHECK(row_shift[p] >= -UBU_MAX_SHIFT && row_shift[p] <= UBU_MAX_SHIFT, "ubu_match: row_shift[%d]=%d must be in -%d..%d", p, row_shift[p],
              UBU_MAX_SHIFT, UBU_MAX_SHIFT);
  SAT_CHECK(ids && clusters && count && view, "ubu_match: null pointer (ids, clusters, count, view)");
  SAT_CHECK(profile && candidates && pairs && ncand && status && scratch, "ubu_match: null pointer (profile, candidates, pairs, ncand, status, scratch)");
  SAT_CHECK(aligned16(ids) && aligned16(view), "ubu_match: ids and view must be 16-byte aligned");
  SAT_CHECK(aligned(clusters, 8) && aligned(count, 8) && aligned(candidates, 8) && aligned(ncand, 8) && aligned(status, 8),
            "ubu_match: clusters, count, candidates, ncand and status must be 8-byte aligned");
  SAT_CHECK(aligned(profile, 4) && aligned16(pairs) && aligned16(scratch), "ubu_match: profile must be 4-byte, pairs and scratch 16-byte aligned");
  const u64 px = (u64)plan.pixels, S = (u64)slots;
  struct Range { const void* p; u64 bytes; };
  const Range in[4] = {{ids, 4 * px}, {clusters, 8 * (u64)plan.rows_max * (u64)cluster_width}, {count, 8}, {view, 4 * px}};
  const Range out[6] = {{profile, 4 * S * (u64)plan.T}, {candidates, 8 * S * UBU_CAND_COLUMNS}, {pairs, 8 * S * S * UBU_PAIR_COLUMNS}, {ncand, 8},
                        {status, 16}, {scratch, (u64)plan.scratch_bytes}};
  for (int o = 0; o < 6; ++o) {
    for (int i = 0; i < 4; ++i) SAT_CHECK(!overlap(out[o].p, out[o].bytes, in[i].p, in[i].bytes), "ubu_match: an output or scratch overlaps an input");
    for (int o2 = o + 1; o2 < 6; ++o2)
      SAT_CHECK(!overlap(out[o].p, out[o].bytes, out[o2].p, out[o2].bytes), "ubu_match: outputs and scratch overlap one another");
  }
  MatK a;
  a.ids = ids; a.clusters = clusters; a.count = count; a.view = view;
  a.profile = profile;
  a.mask = (u64*)scratch;
  a.occ = (unsigned*)((char*)scratch + plan.occ_offset);
  a.slot_of = (int*)((char*)scratch + plan.slot_offset);
  a.cand = candidates; a.pairs = pairs; a.ncand = ncand; a.status = status;
  a.rows_max = (u64)plan.rows_max; a.min_pixels = (long long)min_pixels; a.scale = adc_scale;
  a.width = cluster_width; a.log2_bin = plan.log2_bin; a.tiles = (int)plan.tiles;
  for (int p = 0; p < ubu::MAX_PLANES; ++p) a.shift[p] = p < P ? row_shift[p] : 0;
  a.pixels = (unsigned)plan.pixels; a.rc = (unsigned)rows * (unsigned)cols; a.rows = (unsigned)rows; a.cols = (unsigned)cols;
  a.T = (unsigned)plan.T; a.chunks = (unsigned)plan.chunks; a.S = (unsigned)slots;
  a.trips = (unsigned)plan.trips; a.span = (unsigned)plan.span; a.select_trips = (unsigned)plan.select_trips;
  hipStream_t st = (hipStream_t)stream;
  clear_kernel<<<dim3((unsigned)plan.clear_grid), dim3(UBU_LANES), 0, st>>>(a);
  SAT_LAUNCH_CHECK("ubu_match (clear)");
  select_kernel<<<dim3(1), dim3(UBU_LANES), 0, st>>>(a);
  SAT_LAUNCH_CHECK("ubu_match (select)");
  profile_kernel<<<dim3((unsigned)plan.grid), dim3(UBU_LANES), 0, st>>>(a);
  SAT_LAUNCH_CHECK("ubu_match (profile)");
  summary_kernel<<<dim3((unsigned)plan.summary_grid), dim3(UBU_LANES), 0, st>>>(a);
  SAT_LAUNCH_CHECK("ubu_match (summarise)");
  match_kernel<<<dim3((unsigned)plan.match_grid), dim3(UBU_LANES), 0, st>>>(a);
  SAT_LAUNCH_CHECK("ubu_match (match)");
  return UBU_OK;
}
