// libubresnet_moment.so: per-cluster charge and shape (include/ubresnet_moment.h).  It links against none of the other libraries
// and shares ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream.  Limits, the clear grid and the overflow
// bound come from ../ubr_moment_plan.h, which tests/moment_host.cpp runs on the host; trip, grid and span from ../ubr_walk_plan.h
// (tests/walk_host.cpp); the loads, the wave round and the trip loop from ../ubr_walk.h, the weight of a pixel from
// ../ubr_adc_rule.h, the wave sums from ../ubr_wave.h.  libubresnet_overlap.so walks the pixels with the same three headers.
//
// Loops and their bounds ("ClusterMoments"):
//   the trip loop of a workgroup (walk::trip_loop, ubr_walk.h) runs over the host-computed span; the clear strides over a length
//     read from the device
//   a wave round (walk::wave_round, ubr_walk.h) ends after one trip per distinct cluster among its lanes: each trip clears at
//     least one bit of `rem`
//   find_slot makes at most PROBES probes
// No loop reads a word to wait for another workgroup's store.
#include <hip/hip_runtime.h>
#include "../../../include/ubresnet_moment.h"
#include "../ubr_moment_plan.h"
#include "../ubr_adc_rule.h"
#include "../ubr_sat.h"
#include "../ubr_walk.h"

#define UBM_VERSION 1

SAT_RETURN_CODES(UBM);
SAT_EXPORTS(ubm, UBM_VERSION)
using namespace sat;

static_assert(ubm::LANES == UBM_LANES && ubm::TRIP_PIXELS == UBM_TRIP_PIXELS && ubm::MAX_GRID == UBM_MAX_GRID && ubm::SLOTS == UBM_SLOTS &&
                  ubm::MAX_CLASSES == UBM_MAX_CLASSES && ubm::TABLE_FIXED == UBM_TABLE_FIXED && ubm::MAX_ROWS == UBM_MAX_ROWS &&
                  ubm::MAX_COLS == UBM_MAX_COLS && ubm::MAX_PLANE_PIXELS == UBM_MAX_PLANE_PIXELS && ubm::MAX_WEIGHT == UBM_MAX_WEIGHT &&
                  ubm::MAX_SCALE == UBM_MAX_SCALE,
              "the plan is the geometry of the public header");
static_assert(ubm::LANE_PIXELS == 4 && ubm::WAVE == 64 && ubm::TABLE_FIXED == 9, "the kernel unrolls four pixels per lane and nine fixed columns");

namespace {

typedef unsigned long long u64;
constexpr int SLOT_WORDS = ubm::SLOT_WORDS;

struct MomK {
  const int32_t* ids;
  const uint8_t* label;
  const float* view;
  u64* table;
  const u64* count;
  u64 capacity;
  float scale;
  int C, width;
  unsigned pixels, rc, rows, cols;
  unsigned trips, span;
};

// the rows below min(*count, capacity), zeroed
__global__ __launch_bounds__(UBM_LANES) void clear_kernel(u64* __restrict__ table, const u64* __restrict__ count, u64 capacity, u64 width) {
  u64 n = *count;
  if (n > capacity) n = capacity;
  n *= width;
  for (u64 i = (u64)blockIdx.x * UBM_LANES + threadIdx.x; i < n; i += (u64)gridDim.x * UBM_LANES) table[i] = 0ull;
}

// the count word of a weighed pixel: weighted | clipped << COUNT_BITS | odd << 2 COUNT_BITS
__device__ __forceinline__ unsigned count_word(const adc::Weight& r) {
  if (r.cls == adc::PLAIN) return r.w != 0u ? 1u : 0u;
  return r.cls == adc::ODD ? 1u << (2 * ubm::COUNT_BITS) : 1u | (1u << ubm::COUNT_BITS);
}

// The LDS table of a workgroup: SLOTS slots of SLOT_WORDS sums, keyed by the cluster number (-1: free).  A free slot holds zeros.
struct Lds {
  u64* val;
  int* key;
  unsigned* used;
};

// the slot of cluster k, claimed if need be; -1 if the PROBES slots from k % SLOTS on belong to other clusters
__device__ __forceinline__ int find_slot(const Lds& s, int k) {
  for (int p = 0; p < ubm::PROBES; ++p) {
    const int slot = (k + p) & (ubm::SLOTS - 1);
    const int old = atomicCAS(s.key + slot, -1, k);
    if (old == -1) {
      atomicAdd(s.used, 1u);
      return slot;
    }
    if (old == k) return slot;
  }
  return -1;
}

// one column of cluster k: into its slot, or into memory directly where it has none (row < capacity: the caller's lit test)
__device__ __forceinline__ void push(const Lds& s, const MomK& a, int slot, int k, int col, u64 v) {
  if (v == 0ull) return;
  if (slot >= 0) atomicAdd(s.val + slot * SLOT_WORDS + col, v);
  else atomicAdd(a.table + (u64)k * (u64)a.width + (u64)col, v);
}

struct Sums {
  unsigned cnt, q;
  u64 qr, qc, qrr, qrc, qcc;
};

__device__ __forceinline__ void push_sums(const Lds& s, const MomK& a, int slot, int k, const Sums& m) {
  push(s, a, slot, k, 0, (u64)(m.cnt & ((1u << ubm::COUNT_BITS) - 1u)));
  push(s, a, slot, k, 1, (u64)((m.cnt >> ubm::COUNT_BITS) & ((1u << ubm::COUNT_BITS) - 1u)));
  push(s, a, slot, k, 2, (u64)(m.cnt >> (2 * ubm::COUNT_BITS)));
  push(s, a, slot, k, 3, (u64)m.q);
  push(s, a, slot, k, 4, m.qr);
  push(s, a, slot, k, 5, m.qc);
  push(s, a, slot, k, 6, m.qrr);
  push(s, a, slot, k, 7, m.qrc);
  push(s, a, slot, k, 8, m.qcc);
}

// One wave round: every lane brings the sums `m` of those of its four pixels that `pm` names, all of cluster `key` (-1: none).
// The lanes that share a cluster are summed across the wave, and the first of them sends the sums on; a lane alone with its
// cluster sends its own (walk::wave_round).  w[j] is 0 for a pixel that adds no charge, and lab[j] < C wherever w[j] != 0.
__device__ __forceinline__ void wave_round(const Lds& s, const MomK& a, int key, unsigned pm, const Sums& m, const unsigned (&w)[4],
                                           const unsigned (&lab)[4]) {
  const bool active = key >= 0 && (m.cnt | m.q) != 0u;            // a pixel of weight 0 that is neither clipped nor odd adds nothing
  walk::wave_round(key, active, [&](const wv::KeyGroup<int>& g, int lane) {
    Sums t;
    t.cnt = wv::sum_all(g.member ? m.cnt : 0u);
    t.q = wv::sum_all(g.member ? m.q : 0u);
    t.qr = wv::sum_all(g.member ? m.qr : 0ull);
    t.qc = wv::sum_all(g.member ? m.qc : 0ull);
    t.qrr = wv::sum_all(g.member ? m.qrr : 0ull);
    t.qrc = wv::sum_all(g.member ? m.qrc : 0ull);
    t.qcc = wv::sum_all(g.member ? m.qcc : 0ull);
    int slot = -1;
    if (lane == g.leader) {
      slot = find_slot(s, g.key);
      push_sums(s, a, slot, g.key, t);
    }
    if (t.q != 0u) {
      for (int c = 0; c < a.C; ++c) {
        unsigned mine = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) mine += (g.member && ((pm >> j) & 1u) && lab[j] == (unsigned)c) ? w[j] : 0u;
        const unsigned qc = wv::sum_all(mine);
        if (lane == g.leader) push(s, a, slot, g.key, UBM_TABLE_FIXED + c, (u64)qc);
      }
    }
  }, [&] {
    const int slot = find_slot(s, key);
    push_sums(s, a, slot, key, m);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (((pm >> j) & 1u) && w[j] != 0u) push(s, a, slot, key, UBM_TABLE_FIXED + (int)lab[j], (u64)w[j]);
  });
}

// the four pixels q .. q + 3 of a lane, whose cluster numbers are k4
__device__ __forceinline__ void lane_pixels(const Lds& s, const MomK& a, unsigned q, const int4 k4, u64 nrows) {
  const int k[4] = {k4.x, k4.y, k4.z, k4.w};
  unsigned lit = 0u;                                              // bit j: pixel q + j belongs to a cluster whose row is written
#pragma unroll
  for (int j = 0; j < 4; ++j) lit |= (unsigned)(k[j] >= 0 && (u64)k[j] < nrows) << j;
  if (__ballot(lit != 0u) == 0ull) return;                        // wave-uniform
  unsigned w[4] = {0u, 0u, 0u, 0u}, lab[4] = {0u, 0u, 0u, 0u}, cnt[4] = {0u, 0u, 0u, 0u};
  unsigned y[4] = {0u, 0u, 0u, 0u}, x[4] = {0u, 0u, 0u, 0u};
  int first = -1;
  bool mixed = false;
  if (lit != 0u) {
    float v[4];
    if (q + 3u < a.pixels) {                                      // q is a multiple of four: both loads are aligned
      const float4 v4 = *(const float4*)(a.view + q);
      const uchar4 l4 = *(const uchar4*)(a.label + q);
      v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
      lab[0] = l4.x; lab[1] = l4.y; lab[2] = l4.z; lab[3] = l4.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = q + (unsigned)j < a.pixels;               // a pixel past the end is not lit
        v[j] = in ? a.view[q + j] : 0.0f;
        lab[j] = in ? (unsigned)a.label[q + j] : 0u;
      }
    }
    const unsigned o = q % a.rc;
    unsigned yy = o / a.cols, xx = o - yy * a.cols;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      y[j] = yy; x[j] = xx;
      if (++xx == a.cols) {                                       // the next pixel starts a row, or a plane
        xx = 0u;
        if (++yy == a.rows) yy = 0u;
      }
      if (!((lit >> j) & 1u)) continue;
      if (lab[j] >= (unsigned)a.C) {                              // no class of the table: odd, and nothing else
        cnt[j] = 1u << (2 * ubm::COUNT_BITS);
      } else {
        const adc::Weight r = adc::weight_of(v[j], a.scale);
        w[j] = r.w;
        cnt[j] = count_word(r);
      }
      if (first < 0) first = k[j];
      else mixed = mixed || k[j] != first;
    }
  }
  if (__ballot(mixed) == 0ull) {                                  // wave-uniform: every lane's lit pixels are of one cluster
    Sums m = {0u, 0u, 0ull, 0ull, 0ull, 0ull, 0ull};
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                 // w and cnt are 0 where the pixel is not lit
      const u64 wy = (u64)w[j] * y[j], wx = (u64)w[j] * x[j];
      m.cnt += cnt[j]; m.q += w[j];
      m.qr += wy; m.qc += wx;
      m.qrr += wy * y[j]; m.qrc += wy * x[j]; m.qcc += wx * x[j];
    }
    wave_round(s, a, first, lit, m, w, lab);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u64 wy = (u64)w[j] * y[j], wx = (u64)w[j] * x[j];
      const Sums m = {cnt[j], w[j], wy, wx, wy * y[j], wy * x[j], wx * x[j]};
      wave_round(s, a, ((lit >> j) & 1u) ? k[j] : -1, 1u << j, m, w, lab);
    }
  }
}

// the occupied slots to memory, zero columns left out; the table is empty afterwards.  Every lane of the workgroup calls it.
__device__ __forceinline__ void flush(const Lds& s, const MomK& a) {
  __syncthreads();                                                // every add of the trips before has landed
  for (int i = threadIdx.x; i < ubm::SLOTS * SLOT_WORDS; i += UBM_LANES) {
    const int slot = i / SLOT_WORDS, col = i - slot * SLOT_WORDS;
    const int k = s.key[slot];
    if (k < 0) continue;
    const u64 v = s.val[i];
    if (v == 0ull) continue;
    atomicAdd(a.table + (u64)k * (u64)a.width + (u64)col, v);     // col < width: a class column at or past C is never added to
    s.val[i] = 0ull;
  }
  __syncthreads();
  if (threadIdx.x < ubm::SLOTS) s.key[threadIdx.x] = -1;
  if (threadIdx.x == 0) *s.used = 0u;
  __syncthreads();
}

__global__ __launch_bounds__(UBM_LANES) void moment_kernel(const MomK a) {
  __shared__ u64 s_val[ubm::SLOTS * SLOT_WORDS];
  __shared__ int s_key[ubm::SLOTS];
  __shared__ unsigned s_used;
  const Lds s = {s_val, s_key, &s_used};
  for (int i = threadIdx.x; i < ubm::SLOTS * SLOT_WORDS; i += UBM_LANES) s_val[i] = 0ull;
  if (threadIdx.x < ubm::SLOTS) s_key[threadIdx.x] = -1;
  if (threadIdx.x == 0) s_used = 0u;
  __syncthreads();
  u64 nrows = *a.count;
  if (nrows > a.capacity) nrows = a.capacity;
  walk::trip_loop(a.trips, a.span, &s_used, (unsigned)ubm::FLUSH_ABOVE, [&](unsigned q) { return walk::load_ids(a.ids, q, a.pixels); },
                  [&](unsigned q, const int4& k4) { lane_pixels(s, a, q, k4, nrows); }, [&] { flush(s, a); });
}

}  // namespace

extern "C" int ubm_moments(const int32_t* ids, const uint8_t* label, const float* view, int C, float adc_scale, long long* table,
                           int64_t capacity, const unsigned long long* count, int P, int rows, int cols, void* stream) {
  SAT_CHECK(C >= 1 && C <= UBM_MAX_CLASSES, "ubm_moments: C=%d must be 1..%d", C, UBM_MAX_CLASSES);
  SAT_CHECK(ubm::valid_scale(adc_scale), "ubm_moments: adc_scale=%g must be a power of two in 1..%d", (double)adc_scale, UBM_MAX_SCALE);
  SAT_CHECK(capacity >= 1, "ubm_moments: capacity=%lld must be >= 1", (long long)capacity);
  const char* why;
  SAT_CHECK(ubm::valid_image(P, rows, cols, &why), "ubm_moments: P=%d, rows=%d, cols=%d: %s", P, rows, cols, why);
  ubm::Plan plan;
  SAT_CHECK(ubm::make_plan(P, rows, cols, capacity, C, &plan), "ubm_moments: no plan for P=%d, rows=%d, cols=%d", P, rows, cols);
  SAT_CHECK(ids && label && view, "ubm_moments: null pointer (ids, label, view)");
  SAT_CHECK(table && count, "ubm_moments: null pointer (table, count)");
  SAT_CHECK(aligned16(ids) && aligned16(view) && aligned(label, 4), "ubm_moments: ids and view must be 16-byte and label 4-byte aligned");
  SAT_CHECK(aligned(table, 8) && aligned(count, 8), "ubm_moments: table and count must be 8-byte aligned");
  const u64 px = (u64)plan.pixels, cap = (u64)capacity < px ? (u64)capacity : px;             // rows that can be written
  const u64 tbytes = 8 * cap * (u64)(UBM_TABLE_FIXED + C);
  SAT_CHECK(!overlap(table, tbytes, ids, 4 * px) && !overlap(table, tbytes, label, px) && !overlap(table, tbytes, view, 4 * px) &&
                !overlap(table, tbytes, count, 8),
            "ubm_moments: table overlaps an input");
  MomK a;
  a.ids = ids; a.label = label; a.view = view; a.table = (u64*)table; a.count = count;
  a.capacity = cap; a.scale = adc_scale; a.C = C; a.width = UBM_TABLE_FIXED + C;
  a.pixels = (unsigned)plan.pixels; a.rc = (unsigned)rows * (unsigned)cols; a.rows = (unsigned)rows; a.cols = (unsigned)cols;
  a.trips = (unsigned)plan.trips; a.span = (unsigned)plan.span;
  hipStream_t st = (hipStream_t)stream;
  clear_kernel<<<dim3((unsigned)plan.clear_grid), dim3(UBM_LANES), 0, st>>>((u64*)table, count, cap, (u64)a.width);
  SAT_LAUNCH_CHECK("ubm_moments (clear)");
  moment_kernel<<<dim3((unsigned)plan.grid), dim3(UBM_LANES), 0, st>>>(a);
  SAT_LAUNCH_CHECK("ubm_moments (accumulate)");
  return UBM_OK;
}
