// libubresnet_overlap.so: the pair table of two id maps (include/ubresnet_overlap.h).  It links against none of the other
// libraries and shares ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream.  The clear grid, the scratch
// layout, the pair key, its home slot and the probe limit come from ../ubr_overlap_plan.h, which tests/overlap_host.cpp runs on
// the host; trip, grid and span from ../ubr_walk_plan.h (tests/walk_host.cpp); the loads, the wave round and the trip loop of
// the insert from ../ubr_walk.h, the weight of a pixel from ../ubr_adc_rule.h -- libubresnet_moment.so walks the pixels with the
// same three headers -- and the wave sums and the count / scan / rank of the numbering from ../ubr_wave.h.
//
// Loops and their bounds ("ClusterOverlap"):
//   the trip loop of a workgroup (walk::trip_loop, ubr_walk.h) runs over the host-computed span; the clear strides over the
//     host-given slots
//   a wave round (walk::wave_round, ubr_walk.h) ends after one trip per distinct pair among its lanes: each trip clears at
//     least one bit of `rem`
//   lds_slot makes at most LDS_PROBES probes; claim_slot and find_slot at most `probes` = min(slots, 128)
//   the scan makes the host-computed trips of ubr_scan_plan.h
// No loop reads a word to wait for another workgroup's store.
#include <hip/hip_runtime.h>
#include "../../../include/ubresnet_overlap.h"
#include "../ubr_overlap_plan.h"
#include "../ubr_adc_rule.h"
#include "../ubr_sat.h"
#include "../ubr_walk.h"

#define UBH_VERSION 1

SAT_RETURN_CODES(UBH);
SAT_EXPORTS(ubh, UBH_VERSION)
using namespace sat;

static_assert(ubh::LANES == UBH_LANES && ubh::TRIP_PIXELS == UBH_TRIP_PIXELS && ubh::MAX_GRID == UBH_MAX_GRID &&
                  ubh::LDS_SLOTS == UBH_LDS_SLOTS && ubh::COLUMNS == UBH_COLUMNS && ubh::SLOT_WORDS == UBH_SLOT_WORDS &&
                  ubh::MAX_PROBES == UBH_MAX_PROBES && ubh::MIN_SLOTS == UBH_MIN_SLOTS && ubh::MAX_SLOTS == UBH_MAX_SLOTS &&
                  ubh::MAX_WEIGHT == UBH_MAX_WEIGHT && ubh::MAX_SCALE == UBH_MAX_SCALE,
              "the plan is the geometry of the public header");
static_assert(ubh::LANE_PIXELS == 4 && ubh::WAVE == 64 && ubh::SLOT_WORDS == 5 && ubh::COLUMNS == 6,
              "the kernels unroll four pixels per lane, five slot words and six columns");

namespace {

typedef unsigned long long u64;
constexpr int WAVES = ubh::LANES / ubh::WAVE;
constexpr unsigned COUNT_MASK = (1u << ubh::COUNT_BITS) - 1u;

// a slot in scratch: {key, first, pixels, weighted, Q}
enum { S_KEY = 0, S_FIRST = 1, S_PIXELS = 2, S_WEIGHTED = 3, S_Q = 4 };

struct OvK {
  const int32_t* a;
  const int32_t* b;
  const float* view;             // or null
  u64* slot;                     // [slots][SLOT_WORDS]
  u64* status;
  u64 mask;                      // slots - 1
  float scale;
  int shift;                     // 64 - log2 slots
  int probes;
  unsigned pixels;
  unsigned trips, span;
};

// ---------------------------------------------------------------------------------------------------------------------------
// launch 1: every slot empty
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(UBH_LANES) void clear_kernel(u64* __restrict__ slot, u64 slots) {
  for (u64 i = (u64)blockIdx.x * UBH_LANES + threadIdx.x; i < slots; i += (u64)gridDim.x * UBH_LANES) {
    u64* s = slot + i * ubh::SLOT_WORDS;
    s[S_KEY] = ubh::EMPTY_KEY;
    s[S_FIRST] = ubh::NO_FIRST;
    s[S_PIXELS] = 0ull;
    s[S_WEIGHTED] = 0ull;
    s[S_Q] = 0ull;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the table in scratch
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 home_of(const OvK& k, u64 key) { return (key * ubh::GOLDEN) >> k.shift; }

// The slot that belongs to `key`: one that holds it, or the first empty one of its probe sequence, taken by a compare-and-swap of
// 0 to the key.  A key, once in a slot, never leaves it, so the plain load that spares the swap can only miss a key that arrives
// later -- and then the swap returns it.  null where the `probes` slots all belong to other keys.
__device__ __forceinline__ u64* claim_slot(const OvK& k, u64 key) {
  const u64 h = home_of(k, key);
  for (int p = 0; p < k.probes; ++p) {
    u64* s = k.slot + ((h + (u64)p) & k.mask) * ubh::SLOT_WORDS;
    u64 old = __hip_atomic_load(s + S_KEY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == ubh::EMPTY_KEY) old = atomicCAS(s + S_KEY, (u64)ubh::EMPTY_KEY, key);
    if (old == ubh::EMPTY_KEY || old == key) return s;
  }
  return nullptr;
}

// the sums of a group of pixels of one pair, to memory; npix > 0
__device__ __forceinline__ void to_memory(const OvK& k, u64 key, u64 first, u64 npix, u64 nweighted, u64 q) {
  u64* s = claim_slot(k, key);
  if (s == nullptr) {                                             // dropped, wholly: no earlier or later group of the pair finds one
    atomicAdd(k.status, npix);
    return;
  }
  atomicAdd(s + S_PIXELS, npix);
  if (nweighted != 0ull) atomicAdd(s + S_WEIGHTED, nweighted);
  if (q != 0ull) atomicAdd(s + S_Q, q);
  atomicMin(s + S_FIRST, first);
}

// the slot that holds `key`, read-only (launches 3 and 5: launch 2 is complete); null at an empty slot or at the probe limit
__device__ __forceinline__ const u64* find_slot(const u64* __restrict__ slot, u64 mask, int shift, int probes, u64 key) {
  const u64 h = (key * ubh::GOLDEN) >> shift;
  for (int p = 0; p < probes; ++p) {
    const u64* s = slot + ((h + (u64)p) & mask) * ubh::SLOT_WORDS;
    const u64 old = s[S_KEY];
    if (old == key) return s;
    if (old == ubh::EMPTY_KEY) return nullptr;
  }
  return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------------
// launch 2: insert
// ---------------------------------------------------------------------------------------------------------------------------
// the key of the pair of one pixel: (a + 1) << 32 | (b + 1), a negative id counting as -1; 0 where the pixel does not take part
__device__ __forceinline__ u64 key_of(int a, int b) {
  const u64 ka = a < 0 ? 0ull : (u64)(unsigned)a + 1ull, kb = b < 0 ? 0ull : (u64)(unsigned)b + 1ull;
  return ka << 32 | kb;
}

// The LDS table of a workgroup: LDS_SLOTS slots keyed by the pair (0: free).  A free slot holds first at its maximum and zero sums.
struct Lds {
  u64* key;
  u64* first;
  u64* sum;                      // [LDS_SLOTS][3]: pixels, weighted, Q
  unsigned* used;
};

// the LDS slot of `key`, claimed if need be; -1 if the LDS_PROBES slots from its home on belong to other pairs
__device__ __forceinline__ int lds_slot(const Lds& s, u64 key) {
  const int h = (int)((key * ubh::GOLDEN) >> 58);
  static_assert(ubh::LDS_SLOTS == 64, "the home LDS slot is the top six bits of the hash");
  for (int p = 0; p < ubh::LDS_PROBES; ++p) {
    const int slot = (h + p) & (ubh::LDS_SLOTS - 1);
    const u64 old = atomicCAS(s.key + slot, (u64)ubh::EMPTY_KEY, key);
    if (old == ubh::EMPTY_KEY) {
      atomicAdd(s.used, 1u);
      return slot;
    }
    if (old == key) return slot;
  }
  return -1;
}

// the sums of a group of pixels of one pair: into the LDS slot of the pair, or into memory directly where it has none
__device__ __forceinline__ void push(const Lds& s, const OvK& k, u64 key, unsigned first, unsigned cnt, unsigned q) {
  const u64 npix = (u64)(cnt & COUNT_MASK), nweighted = (u64)(cnt >> ubh::COUNT_BITS);
  const int slot = lds_slot(s, key);
  if (slot < 0) {
    to_memory(k, key, (u64)first, npix, nweighted, (u64)q);
    return;
  }
  atomicAdd(s.sum + slot * 3 + 0, npix);
  if (nweighted != 0ull) atomicAdd(s.sum + slot * 3 + 1, nweighted);
  if (q != 0u) atomicAdd(s.sum + slot * 3 + 2, (u64)q);
  atomicMin(s.first + slot, (u64)first);
}

// One wave round: every lane brings the sums of those of its four pixels that belong to the pair `key` (0: none): cnt = pixels |
// weighted << COUNT_BITS, the charge q and the smallest pixel index `first`.  The lanes that share a pair are summed across the
// wave, and the first of them sends the sums on; a lane alone with its pair sends its own (walk::wave_round).  The pixels of a
// wave ascend with the lane, so the group's smallest index is its leader's.
__device__ __forceinline__ void wave_round(const Lds& s, const OvK& k, u64 key, unsigned first, unsigned cnt, unsigned q) {
  walk::wave_round(key, key != ubh::EMPTY_KEY, [&](const wv::KeyGroup<u64>& g, int lane) {
    const unsigned tc = wv::sum_all(g.member ? cnt : 0u);
    const unsigned tq = wv::sum_all(g.member ? q : 0u);
    if (lane == g.leader) push(s, k, g.key, first, tc, tq);
  }, [&] { push(s, k, key, first, cnt, q); });
}

// the four pixels p .. p + 3 of a lane, whose ids are a4 and b4 (-1 past the end of the image)
__device__ __forceinline__ void lane_pixels(const Lds& s, const OvK& k, unsigned p, const int4 a4, const int4 b4) {
  const u64 key[4] = {key_of(a4.x, b4.x), key_of(a4.y, b4.y), key_of(a4.z, b4.z), key_of(a4.w, b4.w)};
  unsigned part = 0u;                                             // bit j: pixel p + j takes part
#pragma unroll
  for (int j = 0; j < 4; ++j) part |= (unsigned)(key[j] != ubh::EMPTY_KEY) << j;
  if (__ballot(part != 0u) == 0ull) return;                       // wave-uniform
  unsigned w[4] = {0u, 0u, 0u, 0u};
  u64 one = ubh::EMPTY_KEY;
  bool mixed = false;
  if (part != 0u) {
    if (k.view != nullptr) {
      float v[4];
      if (p + 3u < k.pixels) {                                    // p is a multiple of four: the load is aligned
        const float4 v4 = *(const float4*)(k.view + p);
        v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p + (unsigned)j < k.pixels ? k.view[p + j] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((part >> j) & 1u) w[j] = adc::weight_of(v[j], k.scale).w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((part >> j) & 1u)) continue;
      if (one == ubh::EMPTY_KEY) one = key[j];
      else mixed = mixed || key[j] != one;
    }
  }
  if (__ballot(mixed) == 0ull) {                                  // wave-uniform: every lane's pixels that take part are of one pair
    unsigned cnt = 0u, q = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                 // w is 0 where the pixel does not take part
      cnt += ((part >> j) & 1u) + ((w[j] != 0u ? 1u : 0u) << ubh::COUNT_BITS);
      q += w[j];
    }
    wave_round(s, k, one, p + (unsigned)(__ffs((int)part) - 1), cnt, q);   // part == 0: `one` is 0 and the lane is not active
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      wave_round(s, k, key[j], p + (unsigned)j, 1u + ((w[j] != 0u ? 1u : 0u) << ubh::COUNT_BITS), w[j]);
  }
}

// the occupied LDS slots to memory, one lane per slot; the LDS table is empty afterwards.  Every lane of the workgroup calls it.
__device__ __forceinline__ void flush(const Lds& s, const OvK& k) {
  __syncthreads();                                                // every add of the trips before has landed
  if (threadIdx.x < ubh::LDS_SLOTS) {
    const int slot = threadIdx.x;
    const u64 key = s.key[slot];
    if (key != ubh::EMPTY_KEY) {
      to_memory(k, key, s.first[slot], s.sum[slot * 3 + 0], s.sum[slot * 3 + 1], s.sum[slot * 3 + 2]);
      s.key[slot] = ubh::EMPTY_KEY;
      s.first[slot] = ubh::NO_FIRST;
      s.sum[slot * 3 + 0] = 0ull; s.sum[slot * 3 + 1] = 0ull; s.sum[slot * 3 + 2] = 0ull;
    }
  }
  if (threadIdx.x == 0) *s.used = 0u;
  __syncthreads();
}

__global__ __launch_bounds__(UBH_LANES) void insert_kernel(const OvK k) {
  __shared__ u64 s_key[ubh::LDS_SLOTS];
  __shared__ u64 s_first[ubh::LDS_SLOTS];
  __shared__ u64 s_sum[ubh::LDS_SLOTS * 3];
  __shared__ unsigned s_used;
  const Lds s = {s_key, s_first, s_sum, &s_used};
  if (threadIdx.x < ubh::LDS_SLOTS) {
    s_key[threadIdx.x] = ubh::EMPTY_KEY;
    s_first[threadIdx.x] = ubh::NO_FIRST;
    s_sum[threadIdx.x * 3 + 0] = 0ull; s_sum[threadIdx.x * 3 + 1] = 0ull; s_sum[threadIdx.x * 3 + 2] = 0ull;
  }
  if (threadIdx.x == 0) s_used = 0u;
  __syncthreads();
  struct Ids { int4 a, b; };
  walk::trip_loop(k.trips, k.span, &s_used, (unsigned)ubh::FLUSH_ABOVE,
                  [&](unsigned p) { return Ids{walk::load_ids(k.a, p, k.pixels), walk::load_ids(k.b, p, k.pixels)}; },
                  [&](unsigned p, const Ids& i) { lane_pixels(s, k, p, i.a, i.b); }, [&] { flush(s, k); });
}

// ---------------------------------------------------------------------------------------------------------------------------
// launches 3 to 5: count, scan, number.  A lane holds four consecutive pixels; bit j of its mask: pixel p + j is the root of its
// pair, the pixel whose index the pair's slot holds as `first`.  A pixel whose predecessor in the lane has the same pair is no
// root and is not looked up.  root[j] is the slot of a root.
// ---------------------------------------------------------------------------------------------------------------------------
struct NumK {
  const int32_t* a;
  const int32_t* b;
  const u64* slot;
  u64 mask;
  int shift, probes;
  unsigned pixels;
};

__device__ __forceinline__ unsigned root_mask(const NumK& k, unsigned p, const u64* (&root)[4]) {
  const int4 a4 = walk::load_ids(k.a, p, k.pixels), b4 = walk::load_ids(k.b, p, k.pixels);
  const u64 key[4] = {key_of(a4.x, b4.x), key_of(a4.y, b4.y), key_of(a4.z, b4.z), key_of(a4.w, b4.w)};
  unsigned m = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    root[j] = nullptr;
    if (key[j] == ubh::EMPTY_KEY || (j > 0 && key[j] == key[j - 1])) continue;
    const u64* s = find_slot(k.slot, k.mask, k.shift, k.probes, key[j]);
    if (s != nullptr && s[S_FIRST] == (u64)(p + (unsigned)j)) {
      root[j] = s;
      m |= 1u << j;
    }
  }
  return m;
}

__global__ __launch_bounds__(UBH_LANES) void count_kernel(const NumK k, unsigned* __restrict__ counts) {
  __shared__ unsigned s_wave[WAVES];
  const u64* root[4];
  const unsigned m = root_mask(k, blockIdx.x * (unsigned)scanplan::PIXEL_BLOCK + threadIdx.x * 4u, root);
  wv::block_total<WAVES>(wv::mask_count<4>(m), s_wave, [counts](unsigned t) { counts[blockIdx.x] = t; });
}

// ONE workgroup; an exclusive scan of the block counts in place; count[0] = the total
__global__ __launch_bounds__(UBH_LANES) void scan_kernel(unsigned* __restrict__ counts, long blocks, long trips, u64* __restrict__ count) {
  __shared__ unsigned s_wave[WAVES];
  wv::scan_block_counts<WAVES>(counts, blocks, trips, count, s_wave);
}

// root number r < capacity writes row r from its slot, whose sums are complete
__global__ __launch_bounds__(UBH_LANES) void number_kernel(const NumK k, const unsigned* __restrict__ counts, long long* __restrict__ table,
                                                           u64 capacity) {
  __shared__ unsigned s_wave[WAVES];
  const u64* root[4];
  const unsigned m = root_mask(k, blockIdx.x * (unsigned)scanplan::PIXEL_BLOCK + threadIdx.x * 4u, root);
  const unsigned before = wv::block_rank<WAVES, 4>(m, s_wave);
  u64 r = (u64)counts[blockIdx.x] + before;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!((m >> j) & 1u)) continue;
    if (r < capacity) {
      const u64* s = root[j];
      const u64 key = s[S_KEY];
      long long* row = table + r * (u64)UBH_COLUMNS;
      row[0] = (long long)(key >> 32) - 1;
      row[1] = (long long)(key & 0xFFFFFFFFull) - 1;
      row[2] = (long long)s[S_FIRST];
      row[3] = (long long)s[S_PIXELS];
      row[4] = (long long)s[S_WEIGHTED];
      row[5] = (long long)s[S_Q];
    }
    ++r;
  }
}

}  // namespace

extern "C" int64_t ubh_default_slots(int64_t capacity) { return ubh::default_slots(capacity); }

extern "C" int64_t ubh_scratch_bytes(int P, int rows, int cols, int64_t slots) {
  ubh::Plan plan;
  return ubh::make_plan(P, rows, cols, slots, &plan) ? plan.scratch_bytes : 0;
}

extern "C" int ubh_overlap(const int32_t* ids_a, const int32_t* ids_b, const float* view_or_null, float adc_scale, long long* table,
                           int64_t capacity, unsigned long long* count, unsigned long long* status, void* scratch, int64_t slots, int P,
                           int rows, int cols, void* stream) {
  SAT_CHECK(ubh::valid_scale(adc_scale), "ubh_overlap: adc_scale=%g must be a power of two in 1..%d", (double)adc_scale, UBH_MAX_SCALE);
  SAT_CHECK(capacity >= 1, "ubh_overlap: capacity=%lld must be >= 1", (long long)capacity);
  SAT_CHECK(ubh::valid_slots(slots), "ubh_overlap: slots=%lld must be a power of two in %d..%d", (long long)slots, UBH_MIN_SLOTS,
            UBH_MAX_SLOTS);
  const char* why;
  SAT_CHECK(ubh::valid_image(P, rows, cols, &why), "ubh_overlap: P=%d, rows=%d, cols=%d: %s", P, rows, cols, why);
  ubh::Plan plan;
  SAT_CHECK(ubh::make_plan(P, rows, cols, slots, &plan), "ubh_overlap: no plan for P=%d, rows=%d, cols=%d, slots=%lld", P, rows, cols,
            (long long)slots);
  SAT_CHECK(ids_a && ids_b, "ubh_overlap: null pointer (ids_a, ids_b)");
  SAT_CHECK(table && count && status && scratch, "ubh_overlap: null pointer (table, count, status, scratch)");
  SAT_CHECK(aligned16(ids_a) && aligned16(ids_b) && aligned16(view_or_null), "ubh_overlap: ids_a, ids_b and view must be 16-byte aligned");
  SAT_CHECK(aligned(table, 8) && aligned(count, 8) && aligned(status, 8), "ubh_overlap: table, count and status must be 8-byte aligned");
  SAT_CHECK(aligned16(scratch), "ubh_overlap: scratch must be 16-byte aligned");
  const u64 px = (u64)plan.pixels, cap = (u64)capacity < px ? (u64)capacity : px;             // rows that can be written
  const u64 tbytes = 8 * cap * (u64)UBH_COLUMNS, sbytes = (u64)plan.scratch_bytes;
  SAT_CHECK(!overlap(table, tbytes, ids_a, 4 * px) && !overlap(table, tbytes, ids_b, 4 * px) && !overlap(table, tbytes, view_or_null, 4 * px) &&
                !overlap(table, tbytes, count, 8) && !overlap(table, tbytes, status, 16) && !overlap(count, 8, status, 16),
            "ubh_overlap: table, count or status overlaps an input or one another");
  SAT_CHECK(!overlap(scratch, sbytes, ids_a, 4 * px) && !overlap(scratch, sbytes, ids_b, 4 * px) && !overlap(scratch, sbytes, view_or_null, 4 * px) &&
                !overlap(scratch, sbytes, table, tbytes) && !overlap(scratch, sbytes, count, 8) && !overlap(scratch, sbytes, status, 16),
            "ubh_overlap: scratch overlaps another buffer");
  OvK k;
  k.a = ids_a; k.b = ids_b; k.view = view_or_null; k.slot = (u64*)scratch; k.status = status;
  k.mask = (u64)slots - 1ull; k.scale = adc_scale; k.shift = 64 - plan.log2_slots; k.probes = (int)plan.probes;
  k.pixels = (unsigned)plan.pixels; k.trips = (unsigned)plan.trips; k.span = (unsigned)plan.span;
  NumK n;
  n.a = ids_a; n.b = ids_b; n.slot = (const u64*)scratch; n.mask = k.mask; n.shift = k.shift; n.probes = k.probes; n.pixels = k.pixels;
  unsigned* counts = (unsigned*)((char*)scratch + plan.slot_bytes);
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(UBH_LANES), grid((unsigned)plan.blocks.blocks);
  clear_kernel<<<dim3((unsigned)plan.clear_grid), block, 0, st>>>((u64*)scratch, (u64)slots);
  SAT_LAUNCH_CHECK("ubh_overlap (clear)");
  insert_kernel<<<dim3((unsigned)plan.grid), block, 0, st>>>(k);
  SAT_LAUNCH_CHECK("ubh_overlap (insert)");
  count_kernel<<<grid, block, 0, st>>>(n, counts);
  SAT_LAUNCH_CHECK("ubh_overlap (count)");
  scan_kernel<<<dim3(1), block, 0, st>>>(counts, (long)plan.blocks.blocks, (long)plan.blocks.scan_trips, count);
  SAT_LAUNCH_CHECK("ubh_overlap (scan)");
  number_kernel<<<grid, block, 0, st>>>(n, counts, table, cap);
  SAT_LAUNCH_CHECK("ubh_overlap (number)");
  return UBH_OK;
}
