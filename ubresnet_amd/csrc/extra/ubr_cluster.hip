// libubresnet_cluster.so: connected components of event products (include/ubresnet_cluster.h).  It links against none of the
// other libraries and shares ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream.  Tile, pixel block, grids
// and the scratch layout come from ../ubr_cluster_plan.h, which tests/cluster_host.cpp runs on the host together with a model of
// the find and union loops below; the workgroup count, rank and scan of the numbering, the key walk and the wave sum of the tally
// come from ../ubr_wave.h.
//
// Loops and their bounds ("EventClusters"):
//   find     x = parent[x] while parent[x] < x: x strictly decreases, at most x trips
//   unite    every trip ends the loop or replaces the larger root by a smaller index; both indices only decrease: at most a + b trips
//   the scan kernel's trip loop and the gather's stride loop have host-computed trip counts
// No loop reads a word to wait for another workgroup's store: a stale or a fresh parent both lead to the same root.
#include <hip/hip_runtime.h>
#include "../../../include/ubresnet_cluster.h"
#include "../ubr_cluster_plan.h"
#include "../ubr_sat.h"
#include "../ubr_wave.h"

#define UBI_VERSION 1

SAT_RETURN_CODES(UBI);
SAT_EXPORTS(ubi, UBI_VERSION)
using namespace sat;

static_assert(ubi::TILE_H == UBI_TILE_H && ubi::TILE_W == UBI_TILE_W && ubi::LANES == UBI_LANES && ubi::BORDER_LANES == UBI_BORDER_LANES &&
                  ubi::PIXEL_BLOCK == UBI_PIXEL_BLOCK && ubi::SCAN_WIDTH == UBI_SCAN_WIDTH && ubi::MAX_GRID == UBI_MAX_GRID &&
                  ubi::MAX_CLASSES == UBI_MAX_CLASSES && ubi::TABLE_FIXED == UBI_TABLE_FIXED,
              "the plan is the geometry of the public header");
static_assert(ubi::LANE_PIXELS == 4 && ubi::SCAN_LANE_COUNTS == 4 && ubi::WAVE == 64 && ubi::TILE_W == 64,
              "the kernels unroll four pixels / counts per lane and hold a tile row in a wave");

namespace {

typedef unsigned long long u64;
constexpr int TH = ubi::TILE_H, TW = ubi::TILE_W;
constexpr unsigned NOT_LIT = 255u;                              // the LDS key of a pixel that is not lit

// THE lit test, of every pass: the pixel's label is neither the fill label nor outside the classes
__device__ __forceinline__ bool is_lit(unsigned v, int C, int fill) { return v != (unsigned)fill && (int)v < C; }

// ---------------------------------------------------------------------------------------------------------------------------
// find and union on a parent forest with parent[x] <= x, in LDS (SCOPE workgroup) or in global memory (SCOPE agent).  The loads
// are relaxed atomic loads, so that each is a load of its own; the only store is atomicMin.
// ---------------------------------------------------------------------------------------------------------------------------
template <int SCOPE>
__device__ __forceinline__ int find(const int* parent, int x) {
  for (;;) {
    const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, SCOPE);
    if (p >= x || p < 0) return x;                             // a root -- or not a forest: leave rather than climb
    x = p;                                                     // p < x: strictly down
  }
}

template <int SCOPE>
__device__ __forceinline__ void unite(int* parent, int a, int b) {
  for (;;) {
    a = find<SCOPE>(parent, a);
    b = find<SCOPE>(parent, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(parent + b, a);                  // b: the larger root
    if (old >= b) return;                                      // b was a root still: linked
    b = old;                                                   // old < b: b had been linked meanwhile; unite its old parent with a
  }
}

struct LabelK {
  const uint8_t* label;
  int32_t* root;
  u64* status;
  int rows, cols, C, fill, conn8, by_class;
  unsigned tiles_x, tiles_y;
};

struct Tile {
  long plane;                                                   // offset of the plane's first pixel
  int y0, x0;
};

__device__ __forceinline__ Tile tile_of(const LabelK& k, unsigned t) {
  const unsigned tx = t % k.tiles_x, t2 = t / k.tiles_x, ty = t2 % k.tiles_y, p = t2 / k.tiles_y;
  Tile r;
  r.plane = (long)p * ((long)k.rows * k.cols);
  r.y0 = (int)ty * TH;
  r.x0 = (int)tx * TW;
  return r;
}

// launch 1 of ubi_label: one workgroup per tile; wave w holds tile rows w, w + 4, .., lane l column l
__global__ __launch_bounds__(UBI_LANES) void local_kernel(const LabelK k) {
  __shared__ int s_par[ubi::TILE_PIXELS];
  __shared__ unsigned char s_key[ubi::TILE_PIXELS];
  __shared__ unsigned s_foreign[ubi::WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Tile t = tile_of(k, blockIdx.x);
  const int gx = t.x0 + lane;
  unsigned foreign = 0;                                         // wave-uniform
  // row runs: a lit pixel starts at the first pixel of its run, found from the ballot of the run starts
  for (int r = wave; r < TH; r += ubi::WAVES) {
    const int gy = t.y0 + r;
    const bool inside = gy < k.rows && gx < k.cols;
    const unsigned v = inside ? (unsigned)k.label[t.plane + (long)gy * k.cols + gx] : (unsigned)k.fill;
    const bool lit = is_lit(v, k.C, k.fill);
    const unsigned key = lit ? (k.by_class ? v : 0u) : NOT_LIT;
    const unsigned left = (unsigned)__shfl_up((int)key, 1);
    const bool joined = lane > 0 && lit && left == key;
    const u64 starts = __ballot(!joined);                       // bit 0 is always set
    const int start = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));
    const int i = r * TW + lane;
    s_key[i] = (unsigned char)key;
    s_par[i] = lit ? r * TW + start : -1;
    foreign += (unsigned)__popcll(__ballot(v != (unsigned)k.fill && !lit));
  }
  __syncthreads();
  // one union per adjacent pixel of the row above; where the pixel above is adjacent, its row run holds the diagonals
  for (int r = wave; r < TH; r += ubi::WAVES) {
    if (r == 0) continue;
    const int i = r * TW + lane, up = i - TW;
    const unsigned key = s_key[i];
    if (key == NOT_LIT) continue;
    if (s_key[up] == key) {
      unite<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, i, up);
    } else if (k.conn8) {
      if (lane > 0 && s_key[up - 1] == key) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, i, up - 1);
      if (lane < TW - 1 && s_key[up + 1] == key) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, i, up + 1);
    }
  }
  __syncthreads();
  for (int r = wave; r < TH; r += ubi::WAVES) {
    const int gy = t.y0 + r;
    if (gy >= k.rows || gx >= k.cols) continue;
    const int i = r * TW + lane;
    int out = -1;
    if (s_par[i] >= 0) {
      const int f = find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, i);
      out = (int)(t.plane + (long)(t.y0 + f / TW) * k.cols + (t.x0 + f % TW));
    }
    k.root[t.plane + (long)gy * k.cols + gx] = out;
  }
  wv::block_total<ubi::WAVES>(foreign, s_foreign, [&k](unsigned n) {
    if (n) atomicAdd(k.status, (u64)n);
  });
}

// launch 2 of ubi_label: one workgroup per tile; lanes 0..TW-1 the pixels of the tile's last row, united with the three pixels
// below; lanes TW..TW+TH-1 those of its last column, united with the three pixels to the right.  Every pair of adjacent pixels
// of different tiles is one of these: of two rows either side of a tile boundary the upper is a last row, and of two columns
// either side of one in the same tile row the left is a last column.
__global__ __launch_bounds__(UBI_BORDER_LANES) void border_kernel(const LabelK k) {
  const Tile t = tile_of(k, blockIdx.x);
  const int i = threadIdx.x;
  if (i >= TW + TH) return;
  const bool row_item = i < TW;
  const int y = row_item ? t.y0 + TH - 1 : t.y0 + (i - TW), x = row_item ? t.x0 + i : t.x0 + TW - 1;
  if (y >= k.rows || x >= k.cols) return;
  const uint8_t* label = k.label + t.plane;
  const unsigned v = label[(long)y * k.cols + x];
  if (!is_lit(v, k.C, k.fill)) return;
  const int q = (int)(t.plane + (long)y * k.cols + x);
  for (int d = -1; d <= 1; ++d) {
    const int ny = row_item ? y + 1 : y + d, nx = row_item ? x + d : x + 1;
    if (d != 0 && !k.conn8) continue;                           // d != 0: the diagonal neighbours
    if (ny < 0 || ny >= k.rows || nx < 0 || nx >= k.cols) continue;
    const unsigned nv = label[(long)ny * k.cols + nx];
    if (!is_lit(nv, k.C, k.fill) || (k.by_class && nv != v)) continue;
    unite<__HIP_MEMORY_SCOPE_AGENT>(k.root, q, (int)(t.plane + (long)ny * k.cols + nx));
  }
}

// launch 3 of ubi_label: root[q] = find(q), in place.  A pixel that another lane has flattened already names the same root.
__global__ __launch_bounds__(UBI_LANES) void flatten_kernel(int32_t* root, unsigned pixels) {
  for (int j = 0; j < ubi::LANE_PIXELS; ++j) {
    const unsigned q = blockIdx.x * (unsigned)UBI_PIXEL_BLOCK + (unsigned)j * UBI_LANES + threadIdx.x;
    if (q >= pixels) continue;
    const int p = __hip_atomic_load(root + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p < 0 || p >= (int)q) continue;
    const int r = find<__HIP_MEMORY_SCOPE_AGENT>(root, p);
    if (r != p) __hip_atomic_store(root + q, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// numbering: count, scan, number.  A lane holds four consecutive pixels; bit j of its mask: pixel q + j is a root.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned root_mask(const int32_t* __restrict__ root, unsigned q, unsigned pixels, int (&r)[4]) {
  unsigned m = 0u;
  for (unsigned j = 0; j < 4u; ++j) {
    r[j] = q + j < pixels ? root[q + j] : -1;
    m |= (unsigned)(r[j] == (int)(q + j)) << j;                // q + j < 2^31
  }
  return m;
}

__global__ __launch_bounds__(UBI_LANES) void count_kernel(const int32_t* __restrict__ root, unsigned pixels, unsigned* __restrict__ scratch) {
  __shared__ unsigned s_wave[ubi::WAVES];
  int r[4];
  const unsigned m = root_mask(root, blockIdx.x * (unsigned)UBI_PIXEL_BLOCK + threadIdx.x * 4u, pixels, r);
  wv::block_total<ubi::WAVES>(wv::mask_count<4>(m), s_wave, [scratch](unsigned t) { scratch[blockIdx.x] = t; });
}

// ONE workgroup; an exclusive scan of the block counts in place, UBI_SCAN_WIDTH per trip, four per lane; count[0] = total
__global__ __launch_bounds__(UBI_LANES) void scan_kernel(unsigned* __restrict__ scratch, long blocks, long trips, u64* __restrict__ count) {
  __shared__ unsigned s_wave[ubi::WAVES];
  wv::scan_block_counts<ubi::WAVES>(scratch, blocks, trips, count, s_wave);
}

// ids = the cluster number at the roots and -1 at the pixels that are not lit; the root of cluster k < capacity also stores the
// constants of table row k: the root, zero sums and maxima, and minima above every row and column
__global__ __launch_bounds__(UBI_LANES) void number_kernel(const int32_t* __restrict__ root, unsigned pixels, const unsigned* __restrict__ scratch,
                                                           int32_t* __restrict__ ids, long long* __restrict__ table, u64 capacity, int C,
                                                           int rows, int cols) {
  __shared__ unsigned s_wave[ubi::WAVES];
  const unsigned q = blockIdx.x * (unsigned)UBI_PIXEL_BLOCK + threadIdx.x * 4u;
  int r[4];
  const unsigned m = root_mask(root, q, pixels, r);
  const unsigned before = wv::block_rank<ubi::WAVES, 4>(m, s_wave);
  u64 kq = (u64)scratch[blockIdx.x] + before;
  const int width = UBI_TABLE_FIXED + C;
  for (unsigned j = 0; j < 4u; ++j) {
    if (q + j >= pixels) break;
    if (r[j] < 0) ids[q + j] = -1;
    if (!((m >> j) & 1u)) continue;
    ids[q + j] = (int32_t)kq;                                  // the clusters are no more than the pixels: < 2^31
    if (kq < capacity) {
      long long* row = table + kq * (u64)width;
      row[0] = (long long)(q + j);
      row[1] = 0; row[2] = rows; row[3] = 0; row[4] = cols; row[5] = 0; row[6] = 0; row[7] = 0;
      for (int c = 0; c < C; ++c) row[UBI_TABLE_FIXED + c] = 0;
    }
    ++kq;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// tally: lane l of slot j holds pixel block * 1024 + j * 256 + l, so the pixels of a wave ascend with the lane.  The lanes of a
// wave that share a cluster number are found by ballot and combined before one lane goes to memory; a lane alone with its
// number goes by itself, after the loop, together with the other such lanes.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tally_row(u64* row, u64 n, int ymin, int ymax, int xmin, int xmax, u64 sum, u64 bad) {
  atomicAdd(row + 1, n);
  atomicMin(row + 2, (u64)ymin);
  atomicMax(row + 3, (u64)ymax);
  atomicMin(row + 4, (u64)xmin);
  atomicMax(row + 5, (u64)xmax);
  if (sum) atomicAdd(row + 6, sum);
  if (bad) atomicAdd(row + 7, bad);
}

__global__ __launch_bounds__(UBI_LANES) void tally_kernel(const uint8_t* __restrict__ label, const uint16_t* __restrict__ confidence,
                                                          const int32_t* __restrict__ root, int32_t* ids, u64* table, u64 capacity, int C,
                                                          int fill, unsigned pixels, unsigned rc, unsigned cols) {
  const int lane = threadIdx.x & 63;
  const int width = UBI_TABLE_FIXED + C;
  for (int j = 0; j < ubi::LANE_PIXELS; ++j) {
    const unsigned q = blockIdx.x * (unsigned)UBI_PIXEL_BLOCK + (unsigned)j * UBI_LANES + threadIdx.x;
    int k = -1;
    unsigned lab = NOT_LIT;
    if (q < pixels) {
      const int r = root[q];
      lab = label[q];
      if (r >= 0 && r < (int)pixels && is_lit(lab, C, fill)) {
        k = ids[r];                                            // a root's number: the numbering pass stored it
        if (r != (int)q) ids[q] = k;
      }
    }
    const bool counted = k >= 0 && (u64)k < capacity;
    u64 rem = __ballot(counted);
    if (rem == 0ull) continue;                                  // wave-uniform
    int y = 0, x = 0;
    u64 fx = 0ull;
    bool bad = false;
    if (counted) {
      const unsigned o = q % rc;
      y = (int)(o / cols);
      x = (int)(o - (unsigned)y * cols);
      unsigned h = confidence[q];
      if (h == 0x8000u) h = 0u;
      bad = (h & 0x8000u) != 0u || (h & 0x7C00u) == 0x7C00u;
      if (!bad) {
        const unsigned e = h >> 10, m = h & 1023u;
        fx = e == 0u ? (u64)m : (u64)(1024u + m) << (e - 1u);
      }
    }
    bool solo = false;
    while (rem != 0ull) {                                       // wave-uniform: one trip per distinct number among the counted lanes
      const wv::KeyGroup<int> g = wv::next_key_group(rem, k, counted);
      const unsigned n = (unsigned)__popcll(g.lanes);
      if (n == 1u) {
        solo = solo || lane == g.leader;
        continue;
      }
      // a cluster lies in one plane, so its rows ascend with the lane: the first and the last member hold the extremes
      const int last = 63 - __clzll((long long)g.lanes);
      const int ymin = __shfl(y, g.leader), ymax = __shfl(y, last);
      int xmin, xmax;
      if (ymin == ymax) {                                       // one row: the columns ascend as well
        xmin = __shfl(x, g.leader);
        xmax = __shfl(x, last);
      } else {
        xmin = g.member ? x : 0x7FFFFFFF;
        xmax = g.member ? x : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
          xmin = min(xmin, __shfl_xor(xmin, d));
          xmax = max(xmax, __shfl_xor(xmax, d));
        }
      }
      const u64 sum = wv::sum_all(g.member ? fx : 0ull);
      const u64 nbad = (u64)__popcll(__ballot(g.member && bad));
      u64* row = table + (u64)g.key * (u64)width;
      if (lane == g.leader) tally_row(row, (u64)n, ymin, ymax, xmin, xmax, sum, nbad);
      for (int c = 0; c < C; ++c) {
        const unsigned nc = (unsigned)__popcll(__ballot(g.member && lab == (unsigned)c));
        if (nc != 0u && lane == g.leader) atomicAdd(row + UBI_TABLE_FIXED + c, (u64)nc);
      }
    }
    if (solo) {
      u64* row = table + (u64)k * (u64)width;
      tally_row(row, 1ull, y, y, x, x, fx, bad ? 1ull : 0ull);
      atomicAdd(row + UBI_TABLE_FIXED + lab, 1ull);            // lab < C: the pixel is lit
    }
  }
}

// out[i] = ids[index[i]] over the first min(*count, capacity) entries of a pixel list
__global__ __launch_bounds__(UBI_LANES) void gather_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ index,
                                                           const u64* __restrict__ count, long capacity, int32_t* __restrict__ out, long pixels) {
  long m = capacity;
  const u64 c = *count;
  if (c < (u64)m) m = (long)c;
  for (long i = (long)blockIdx.x * UBI_LANES + threadIdx.x; i < m; i += (long)gridDim.x * UBI_LANES) {
    const long q = index[i];
    out[i] = q >= 0 && q < pixels ? ids[q] : -1;
  }
}

// the image checks every call shares; -> 0 or -1 with the message set
int check_image(const char* who, int P, int rows, int cols, ubi::Plan* plan) {
  SAT_CHECK(P >= 1 && rows >= 1 && cols >= 1, "%s: P=%d, rows=%d, cols=%d must be positive", who, P, rows, cols);
  SAT_CHECK(ubi::make_plan(P, rows, cols, plan), "%s: P=%d x rows=%d x cols=%d must be below 2^31 pixels (int32 pixel index)", who, P, rows,
            cols);
  return 0;
}

int check_classes(const char* who, int C, int fill_label) {
  SAT_CHECK(C >= 1 && C <= UBI_MAX_CLASSES, "%s: C=%d must be 1..%d", who, C, UBI_MAX_CLASSES);
  SAT_CHECK(fill_label >= 0 && fill_label <= 255, "%s: fill_label=%d must be 0..255", who, fill_label);
  return 0;
}

}  // namespace

extern "C" int64_t ubi_scratch_bytes(int P, int rows, int cols) {
  ubi::Plan plan;
  if (!ubi::make_plan(P, rows, cols, &plan)) {
    set_error("ubi_scratch_bytes: P=%d, rows=%d, cols=%d must be positive and below 2^31 pixels", P, rows, cols);
    return 0;
  }
  return plan.scratch_bytes;
}

extern "C" int ubi_label(const uint8_t* label, int C, int fill_label, int connectivity, int by_class, int32_t* root,
                         unsigned long long* status, int P, int rows, int cols, void* stream) {
  if (check_classes("ubi_label", C, fill_label)) return UBI_EINVAL;
  SAT_CHECK(connectivity == 4 || connectivity == 8, "ubi_label: connectivity=%d must be 4 or 8", connectivity);
  SAT_CHECK(by_class == 0 || by_class == 1, "ubi_label: by_class=%d must be 0 or 1", by_class);
  ubi::Plan plan;
  if (check_image("ubi_label", P, rows, cols, &plan)) return UBI_EINVAL;
  SAT_CHECK(label && root && status, "ubi_label: null pointer (label, root, status)");
  SAT_CHECK(aligned(root, 4) && aligned(status, 8), "ubi_label: root must be 4-byte aligned and status 8-byte aligned");
  const u64 px = (u64)plan.pixels;
  SAT_CHECK(!overlap(root, 4 * px, label, px) && !overlap(status, 8, label, px) && !overlap(status, 8, root, 4 * px),
            "ubi_label: root, status and label overlap");
  LabelK k;
  k.label = label; k.root = root; k.status = status;
  k.rows = rows; k.cols = cols; k.C = C; k.fill = fill_label; k.conn8 = connectivity == 8; k.by_class = by_class;
  k.tiles_x = (unsigned)plan.tiles_x; k.tiles_y = (unsigned)plan.tiles_y;
  hipStream_t st = (hipStream_t)stream;
  local_kernel<<<dim3((unsigned)plan.tiles), dim3(UBI_LANES), 0, st>>>(k);
  SAT_LAUNCH_CHECK("ubi_label (local)");
  border_kernel<<<dim3((unsigned)plan.tiles), dim3(UBI_BORDER_LANES), 0, st>>>(k);
  SAT_LAUNCH_CHECK("ubi_label (border)");
  flatten_kernel<<<dim3((unsigned)plan.blocks), dim3(UBI_LANES), 0, st>>>(root, (unsigned)plan.pixels);
  SAT_LAUNCH_CHECK("ubi_label (flatten)");
  return UBI_OK;
}

extern "C" int ubi_tabulate(const uint8_t* label, const uint16_t* confidence, const int32_t* root, int C, int fill_label, int32_t* ids,
                            long long* table, int64_t capacity, unsigned long long* count, void* scratch, int P, int rows, int cols,
                            void* stream) {
  if (check_classes("ubi_tabulate", C, fill_label)) return UBI_EINVAL;
  SAT_CHECK(capacity >= 1, "ubi_tabulate: capacity=%lld must be >= 1", (long long)capacity);
  ubi::Plan plan;
  if (check_image("ubi_tabulate", P, rows, cols, &plan)) return UBI_EINVAL;
  SAT_CHECK(label && confidence && root, "ubi_tabulate: null pointer (label, confidence, root)");
  SAT_CHECK(ids && table && count, "ubi_tabulate: null pointer (ids, table, count)");
  SAT_CHECK(scratch, "ubi_tabulate: null pointer (scratch)");
  SAT_CHECK(aligned(confidence, 2) && aligned(root, 4) && aligned(ids, 4) && aligned(table, 8) && aligned(count, 8),
            "ubi_tabulate: confidence must be 2-byte, root / ids 4-byte and table / count 8-byte aligned");
  SAT_CHECK(aligned16(scratch), "ubi_tabulate: scratch must be 16-byte aligned");
  const u64 px = (u64)plan.pixels, cap = (u64)capacity < px ? (u64)capacity : px;          // rows that can be written
  const void* outs[4] = {ids, table, count, scratch};
  const u64 obytes[4] = {4 * px, 8 * cap * (u64)(UBI_TABLE_FIXED + C), 8, (u64)plan.scratch_bytes};
  for (int i = 0; i < 4; ++i) {
    SAT_CHECK(!overlap(outs[i], obytes[i], label, px) && !overlap(outs[i], obytes[i], confidence, 2 * px) &&
                  !overlap(outs[i], obytes[i], root, 4 * px),
              "ubi_tabulate: an output or scratch overlaps an input");
    for (int j = i + 1; j < 4; ++j) SAT_CHECK(!overlap(outs[i], obytes[i], outs[j], obytes[j]), "ubi_tabulate: two outputs overlap");
  }
  const unsigned pixels = (unsigned)plan.pixels;
  const dim3 grid((unsigned)plan.blocks), block(UBI_LANES);
  hipStream_t st = (hipStream_t)stream;
  count_kernel<<<grid, block, 0, st>>>(root, pixels, (unsigned*)scratch);
  SAT_LAUNCH_CHECK("ubi_tabulate (count)");
  scan_kernel<<<dim3(1), block, 0, st>>>((unsigned*)scratch, (long)plan.blocks, (long)plan.scan_trips, count);
  SAT_LAUNCH_CHECK("ubi_tabulate (scan)");
  number_kernel<<<grid, block, 0, st>>>(root, pixels, (const unsigned*)scratch, ids, table, (u64)capacity, C, rows, cols);
  SAT_LAUNCH_CHECK("ubi_tabulate (number)");
  tally_kernel<<<grid, block, 0, st>>>(label, confidence, root, ids, (u64*)table, (u64)capacity, C, fill_label, pixels,
                                       (unsigned)rows * (unsigned)cols, (unsigned)cols);
  SAT_LAUNCH_CHECK("ubi_tabulate (tally)");
  return UBI_OK;
}

extern "C" int ubi_gather_ids(const int32_t* ids, const int32_t* index, const unsigned long long* list_count, int64_t list_capacity,
                              int32_t* out, int64_t pixels, void* stream) {
  SAT_CHECK(list_capacity >= 1 && list_capacity <= ubi::MAX_PIXELS, "ubi_gather_ids: list_capacity=%lld must be in 1..2^31-1",
            (long long)list_capacity);
  SAT_CHECK(pixels >= 1 && pixels <= ubi::MAX_PIXELS, "ubi_gather_ids: pixels=%lld must be in 1..2^31-1", (long long)pixels);
  SAT_CHECK(ids && index && list_count && out, "ubi_gather_ids: null pointer (ids, index, list_count, out)");
  SAT_CHECK(aligned(ids, 4) && aligned(index, 4) && aligned(out, 4) && aligned(list_count, 8),
            "ubi_gather_ids: ids, index and out must be 4-byte aligned and list_count 8-byte aligned");
  const u64 n4 = 4ull * (u64)list_capacity;
  SAT_CHECK(!overlap(out, n4, ids, 4ull * (u64)pixels) && !overlap(out, n4, index, n4) && !overlap(out, n4, list_count, 8),
            "ubi_gather_ids: out overlaps an input");
  gather_kernel<<<dim3((unsigned)ubi::stride_grid(list_capacity)), dim3(UBI_LANES), 0, (hipStream_t)stream>>>(
      ids, index, list_count, (long)list_capacity, out, (long)pixels);
  SAT_LAUNCH_CHECK("ubi_gather_ids");
  return UBI_OK;
}
