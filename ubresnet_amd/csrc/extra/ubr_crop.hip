// libubresnet_crop.so: training crops out of a whole labelled view (include/ubresnet_crop.h).  It links against none of the other
// libraries and shares ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream.  The rule -- geometry, label
// conversion, the selection of one crop, the check of a table row -- is ../ubr_crop_rule.h, which tests/crop_host.cpp runs on
// the host; Philox comes with it from ../ubr_det_rule.h.  The workgroup scan of the occupancy rows is that of ../ubr_wave.h.
#include <hip/hip_runtime.h>
#include "../../../include/ubresnet_crop.h"
#include "../ubr_sat.h"
#include "../ubr_crop_rule.h"
#include "../ubr_wave.h"

#define UBN_VERSION 1

SAT_RETURN_CODES(UBN);
SAT_EXPORTS(ubn, UBN_VERSION)
using namespace sat;

static_assert(UBN_LANES == 256 && UBN_TABLE_FIELDS == 8 && UBN_MIN_CELL == 4, "the kernels take four pixels per lane, four waves per workgroup");

namespace {

typedef unsigned long long u64;
const int WAVES = UBN_LANES / 64;

// ---------------------------------------------------------------------------------------------------------------------------
// four consecutive elements: 16-byte accesses where the address allows, element accesses otherwise
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load4_words(const uint32_t* p, uint32_t v[4]) {
  if (((uintptr_t)p & 15) == 0) {
    const uint4 x = *(const uint4*)p;
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  } else {
    for (int j = 0; j < 4; ++j) v[j] = p[j];
  }
}

__device__ __forceinline__ void store4_words(uint32_t* p, const uint32_t v[4]) {
  if (((uintptr_t)p & 15) == 0) {
    *(uint4*)p = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
    for (int j = 0; j < 4; ++j) p[j] = v[j];
  }
}

__device__ __forceinline__ void store4_labels(long long* p, const long long v[4]) {
  if (((uintptr_t)p & 15) == 0) {
    ((longlong2*)p)[0] = make_longlong2(v[0], v[1]);
    ((longlong2*)p)[1] = make_longlong2(v[2], v[3]);
  } else {
    for (int j = 0; j < 4; ++j) p[j] = v[j];
  }
}

// the converted labels of elements e .. e + 3 of a label image of `kind`
__device__ __forceinline__ void load4_labels(const void* label, int kind, size_t e, int32_t off, long long L[4]) {
  if (kind == UBN_LABEL_U8) {
    const uint8_t* p = (const uint8_t*)label + e;
    if (((uintptr_t)p & 3) == 0) {
      const uint32_t x = *(const uint32_t*)p;
      for (int j = 0; j < 4; ++j) L[j] = ubn::label_of_int((int64_t)((x >> (8 * j)) & 255u), off);
    } else {
      for (int j = 0; j < 4; ++j) L[j] = ubn::label_of_int((int64_t)p[j], off);
    }
  } else if (kind == UBN_LABEL_I64) {
    const long long* p = (const long long*)label + e;
    long long v[4];
    if (((uintptr_t)p & 15) == 0) {
      const longlong2 a = ((const longlong2*)p)[0], b = ((const longlong2*)p)[1];
      v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
      for (int j = 0; j < 4; ++j) v[j] = p[j];
    }
    for (int j = 0; j < 4; ++j) L[j] = ubn::label_of_int(v[j], off);
  } else {
    uint32_t v[4];
    load4_words((const uint32_t*)label + e, v);
    for (int j = 0; j < 4; ++j) L[j] = ubn::label_of_float(__uint_as_float(v[j]), off);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// occupancy
// ---------------------------------------------------------------------------------------------------------------------------
struct occ_t {
  const float* image;
  const void* label;
  int kind;
  int32_t off;
  uint32_t mask;
  int stacked;
  float thr;
  int P, rows, cols, g, CR, CC;
  int32_t* sat;
};

// THE predicate: bit j is set iff pixel (r, c + j) of count plane q counts (c a multiple of 4).  Lit: the plane's value, or any
// of the P values of a stacked pixel, is > thr.  The labels are read only where something is lit and a mask is on.
__device__ __forceinline__ unsigned count_mask(const occ_t& a, int q, int r, int c) {
  const size_t rc = (size_t)a.rows * a.cols, o = (size_t)r * a.cols + c;
  const int p0 = a.stacked ? 0 : q, p1 = a.stacked ? a.P : q + 1;
  unsigned m = 0u;
  for (int p = p0; p < p1; ++p) {
    uint32_t v[4];
    load4_words((const uint32_t*)a.image + p * rc + o, v);
    for (int j = 0; j < 4; ++j) m |= (unsigned)ubn::lit(__uint_as_float(v[j]), a.thr) << j;
  }
  if (a.kind != UBN_LABEL_NONE && m) {
    long long L[4];
    load4_labels(a.label, a.kind, (a.stacked ? 0 : q * rc) + o, a.off, L);
    unsigned ok = 0u;
    for (int j = 0; j < 4; ++j) ok |= (unsigned)ubn::label_counts(L[j], a.mask) << j;
    m &= ok;
  }
  return m;
}

// launch 1: one workgroup per (count plane, cell row).  A wave takes a cell at a time, a lane four pixels of one row of it per
// trip; the cell's count is the popcounts of four ballots per trip.  The counts of the row of cells go through the LDS into an
// inclusive scan along the row, which is row i + 1 of the table before the walk down; column 0 and row 0 are zero.
__global__ __launch_bounds__(UBN_LANES) void count_rows_kernel(const occ_t a) {
  __shared__ int32_t s_cnt[UBN_MAX_CELL_COLS];
  __shared__ int32_t s_wave[WAVES];
  const int q = blockIdx.x / a.CR, i = blockIdx.x - q * a.CR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = a.g, qpr = g >> 2, quads = g * qpr, sh = __ffs(qpr) - 1;      // quads of a cell's row, of a cell
  for (int j = wave; j < a.CC; j += WAVES) {
    int32_t c = 0;                                                          // wave-uniform
    for (int u0 = 0; u0 < quads; u0 += 64) {
      const int u = u0 + lane;
      const unsigned m = u < quads ? count_mask(a, q, i * g + (u >> sh), j * g + 4 * (u & (qpr - 1))) : 0u;
      c += (int32_t)wv::mask_count<4>(m);
    }
    if (lane == 0) s_cnt[j] = c;
  }
  __syncthreads();
  int32_t* row = a.sat + ((size_t)q * (a.CR + 1) + i + 1) * (a.CC + 1);
  int32_t carry = 0;
  for (int j0 = 0; j0 < a.CC; j0 += UBN_LANES) {
    const int j = j0 + (int)threadIdx.x;
    int32_t total;
    const int32_t upto = wv::block_scan<WAVES, int32_t>(j < a.CC ? s_cnt[j] : 0, s_wave, &total);
    if (j < a.CC) row[j + 1] = carry + upto;
    carry += total;
    __syncthreads();                                                        // s_wave is written again in the next trip
  }
  if (threadIdx.x == 0) row[0] = 0;
  if (i == 0) {
    int32_t* top = a.sat + (size_t)q * (a.CR + 1) * (a.CC + 1);
    for (int j = threadIdx.x; j <= a.CC; j += UBN_LANES) top[j] = 0;
  }
}

// launch 2: one thread per (count plane, table column) adds the rows up on its way down
__global__ __launch_bounds__(UBN_LANES) void sum_columns_kernel(int32_t* __restrict__ sat, int Q, int CR, int CC) {
  const int t = blockIdx.x * UBN_LANES + threadIdx.x;
  if (t >= Q * (CC + 1)) return;
  const int q = t / (CC + 1), j = t - q * (CC + 1);
  int32_t* s = sat + (size_t)q * (CR + 1) * (CC + 1) + j;
  int32_t acc = 0;
  for (int i = 1; i <= CR; ++i) {
    acc += s[(size_t)i * (CC + 1)];
    s[(size_t)i * (CC + 1)] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// choose: one thread per crop; the rule is ubn::choose
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(UBN_LANES) void choose_kernel(const int32_t* __restrict__ sat, const ubn::Geometry geo, uint32_t seed_lo,
                                                           uint32_t seed_hi, uint32_t number, int K, int T, int32_t min_lit, int flip_rows,
                                                           int flip_cols, int32_t* __restrict__ table) {
  const int k = blockIdx.x * UBN_LANES + threadIdx.x;
  if (k >= K) return;
  const ubn::Row r = ubn::choose(sat, geo, seed_lo, seed_hi, number, (uint32_t)k, T, min_lit, flip_rows, flip_cols);
  uint32_t* t = (uint32_t*)table + (size_t)k * UBN_TABLE_FIELDS;
  uint32_t lo[4], hi[4];
  for (int f = 0; f < 4; ++f) {
    lo[f] = (uint32_t)r.f[f];
    hi[f] = (uint32_t)r.f[4 + f];
  }
  store4_words(t, lo);
  store4_words(t + 4, hi);
}

// ---------------------------------------------------------------------------------------------------------------------------
// gather: blockIdx.y is the crop, a lane takes four consecutive output pixels of one row
// ---------------------------------------------------------------------------------------------------------------------------
struct gather_t {
  const float* image;
  const void* label;
  int kind;
  int32_t off;
  const float* weight;
  int stacked, P, rows, cols, H, W;
  const int32_t* table;
  float* out_image;
  long long* out_label;
  float* out_weight;
  u64* status;
};

__device__ __forceinline__ void reverse4(uint32_t v[4]) {
  const uint32_t a = v[0], b = v[1];
  v[0] = v[3]; v[1] = v[2]; v[2] = b; v[3] = a;
}

__global__ __launch_bounds__(UBN_LANES) void gather_kernel(const gather_t a) {
  const int k = blockIdx.y;
  const int32_t* t = a.table + (size_t)k * UBN_TABLE_FIELDS;
  const int32_t plane = t[0], row0 = t[1], col0 = t[2], fr = t[6], fc = t[7];
  const bool valid = ubn::row_is_valid(plane, row0, col0, fr, fc, a.stacked, a.P, a.rows, a.cols, a.H, a.W);
  if (!valid && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.status, (u64)1);
  const int wq = a.W >> 2;
  const long u = (long)blockIdx.x * UBN_LANES + threadIdx.x;
  if (u >= (long)a.H * wq) return;
  const int y = (int)(u / wq), x = 4 * (int)(u - (long)y * wq);
  const size_t hw = (size_t)a.H * a.W, at = (size_t)y * a.W + x;
  const int C = a.stacked ? a.P : 1;
  uint32_t v[4] = {0u, 0u, 0u, 0u};
  long long L[4] = {0, 0, 0, 0};
  if (!valid) {                                                    // nothing is read through the row
    for (int c = 0; c < C; ++c) store4_words((uint32_t*)a.out_image + ((size_t)k * C + c) * hw + at, v);
    store4_labels(a.out_label + (size_t)k * hw + at, L);
    store4_words((uint32_t*)a.out_weight + (size_t)k * hw + at, v);
    return;
  }
  const int sr = row0 + (fr ? a.H - 1 - y : y), sc = fc ? col0 + a.W - 4 - x : col0 + x;
  const size_t rc = (size_t)a.rows * a.cols, so = (size_t)sr * a.cols + sc;
  for (int c = 0; c < C; ++c) {
    load4_words((const uint32_t*)a.image + (size_t)(a.stacked ? c : plane) * rc + so, v);
    if (fc) reverse4(v);
    store4_words((uint32_t*)a.out_image + ((size_t)k * C + c) * hw + at, v);
  }
  const size_t e = (a.stacked ? 0 : (size_t)plane * rc) + so;
  load4_labels(a.label, a.kind, e, a.off, L);
  if (fc) {
    const long long l0 = L[0], l1 = L[1];
    L[0] = L[3]; L[1] = L[2]; L[2] = l1; L[3] = l0;
  }
  store4_labels(a.out_label + (size_t)k * hw + at, L);
  if (a.weight) {
    load4_words((const uint32_t*)a.weight + e, v);
    if (fc) reverse4(v);
  } else {
    for (int j = 0; j < 4; ++j) v[j] = UBX_ONE_BITS;
  }
  store4_words((uint32_t*)a.out_weight + (size_t)k * hw + at, v);
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------
int label_bytes(int kind) { return kind == UBN_LABEL_U8 ? 1 : kind == UBN_LABEL_I64 ? 8 : kind == UBN_LABEL_F32 ? 4 : 0; }

int check_view(const char* who, int P, int rows, int cols) {
  SAT_CHECK(P >= 1 && rows >= 1 && cols >= 1, "%s: P=%d, rows=%d, cols=%d must be positive", who, P, rows, cols);
  SAT_CHECK(P <= UBN_MAX_PLANES, "%s: P=%d must be at most %d", who, P, UBN_MAX_PLANES);
  SAT_CHECK(ubn::view_is_legal(P, rows, cols), "%s: P=%d x rows=%d x cols=%d must be below 2^31 pixels", who, P, rows, cols);
  return 0;
}

}  // namespace

extern "C" int ubn_occupancy(const float* image, const void* label, int label_kind, int32_t label_offset, uint32_t class_mask,
                             int stacked, float adc_threshold, int P, int rows, int cols, int cell, int32_t* sat, void* stream) {
  SAT_CHECK(image && sat, "ubn_occupancy: null pointer (image, sat)");
  if (check_view("ubn_occupancy", P, rows, cols)) return UBN_EINVAL;
  SAT_CHECK(ubn::cell_is_legal(cell), "ubn_occupancy: cell=%d must be a power of two in %d..%d", cell, UBN_MIN_CELL, UBN_MAX_CELL);
  SAT_CHECK(rows % cell == 0 && cols % cell == 0, "ubn_occupancy: cell=%d must divide rows=%d and cols=%d", cell, rows, cols);
  SAT_CHECK(cols / cell <= UBN_MAX_CELL_COLS, "ubn_occupancy: cols / cell = %d must be at most %d", cols / cell, UBN_MAX_CELL_COLS);
  SAT_CHECK(label_kind >= UBN_LABEL_NONE && label_kind <= UBN_LABEL_F32, "ubn_occupancy: label_kind=%d must be 0..3", label_kind);
  SAT_CHECK((label == nullptr) == (label_kind == UBN_LABEL_NONE), "ubn_occupancy: a label needs a kind and a kind a label (label_kind=%d)",
            label_kind);
  SAT_CHECK(aligned(image, 4) && aligned(sat, 4), "ubn_occupancy: image and sat must be 4-byte aligned");
  SAT_CHECK(!label || aligned(label, (uintptr_t)label_bytes(label_kind)), "ubn_occupancy: label must be %d-byte aligned", label_bytes(label_kind));
  const int Q = stacked ? 1 : P, CR = rows / cell, CC = cols / cell;
  const u64 px = (u64)P * (u64)rows * (u64)cols, sbytes = 4ull * (u64)Q * (u64)(CR + 1) * (u64)(CC + 1);
  SAT_CHECK(!overlap(sat, sbytes, image, 4 * px) && !overlap(sat, sbytes, label, (u64)label_bytes(label_kind) * (stacked ? px / (u64)P : px)),
            "ubn_occupancy: sat overlaps an input");
  occ_t a;
  a.image = image; a.label = label; a.kind = label_kind; a.off = label_offset; a.mask = class_mask; a.stacked = stacked ? 1 : 0;
  a.thr = adc_threshold; a.P = P; a.rows = rows; a.cols = cols; a.g = cell; a.CR = CR; a.CC = CC; a.sat = sat;
  hipStream_t st = (hipStream_t)stream;
  count_rows_kernel<<<dim3((unsigned)(Q * CR)), dim3(UBN_LANES), 0, st>>>(a);
  SAT_LAUNCH_CHECK("ubn_occupancy (count)");
  sum_columns_kernel<<<dim3((unsigned)((Q * (CC + 1) + UBN_LANES - 1) / UBN_LANES)), dim3(UBN_LANES), 0, st>>>(sat, Q, CR, CC);
  SAT_LAUNCH_CHECK("ubn_occupancy (sum)");
  return UBN_OK;
}

extern "C" int ubn_choose(const int32_t* sat, int Q, int rows, int cols, int H, int W, int cell, const int32_t* planes, int nplanes,
                          int K, int T, int32_t min_lit, uint32_t seed_lo, uint32_t seed_hi, uint32_t number, int flip_rows,
                          int flip_cols, int32_t* table, void* stream) {
  SAT_CHECK(sat && table, "ubn_choose: null pointer (sat, table)");
  if (check_view("ubn_choose", Q, rows, cols)) return UBN_EINVAL;
  SAT_CHECK(H >= 1 && W >= 1 && H <= rows && W <= cols, "ubn_choose: the crop H=%d x W=%d must be positive and fit rows=%d x cols=%d", H, W,
            rows, cols);
  SAT_CHECK(ubn::cell_is_legal(cell), "ubn_choose: cell=%d must be a power of two in %d..%d", cell, UBN_MIN_CELL, UBN_MAX_CELL);
  SAT_CHECK(ubn::cell_fits(cell, rows, cols, H, W), "ubn_choose: cell=%d must divide H=%d, W=%d, rows - H=%d and cols - W=%d", cell, H, W,
            rows - H, cols - W);
  SAT_CHECK(!planes || (nplanes >= 1 && nplanes <= Q), "ubn_choose: nplanes=%d must be 1..Q=%d", nplanes, Q);
  ubn::Geometry geo;
  SAT_CHECK(ubn::make_geometry(Q, rows, cols, H, W, cell, planes, nplanes, &geo), "ubn_choose: planes must be distinct and in 0..%d", Q - 1);
  SAT_CHECK(K >= 1 && K <= UBN_MAX_CROPS, "ubn_choose: K=%d must be 1..%d", K, UBN_MAX_CROPS);
  SAT_CHECK(T >= 1 && T <= UBN_MAX_TRIES, "ubn_choose: T=%d must be 1..%d", T, UBN_MAX_TRIES);
  SAT_CHECK(min_lit >= 0, "ubn_choose: min_lit=%d must be >= 0", (int)min_lit);
  SAT_CHECK(aligned(sat, 4) && aligned(table, 4), "ubn_choose: sat and table must be 4-byte aligned");
  SAT_CHECK(!overlap(table, 4ull * UBN_TABLE_FIELDS * (u64)K, sat, 4ull * (u64)Q * (u64)(geo.CR + 1) * (u64)(geo.CC + 1)),
            "ubn_choose: table overlaps sat");
  choose_kernel<<<dim3((unsigned)((K + UBN_LANES - 1) / UBN_LANES)), dim3(UBN_LANES), 0, (hipStream_t)stream>>>(
      sat, geo, seed_lo, seed_hi, number, K, T, min_lit, flip_rows ? 1 : 0, flip_cols ? 1 : 0, table);
  SAT_LAUNCH_CHECK("ubn_choose");
  return UBN_OK;
}

extern "C" int ubn_gather(const float* image, const void* label, int label_kind, int32_t label_offset, const float* weight, int stacked,
                          int P, int rows, int cols, int H, int W, const int32_t* table, int K, float* out_image, int64_t* out_label,
                          float* out_weight, unsigned long long* status, void* stream) {
  SAT_CHECK(image && label && table, "ubn_gather: null pointer (image, label, table)");
  SAT_CHECK(out_image && out_label && out_weight && status, "ubn_gather: null pointer (out_image, out_label, out_weight, status)");
  if (check_view("ubn_gather", P, rows, cols)) return UBN_EINVAL;
  SAT_CHECK(H >= 1 && W >= 1 && H <= rows && W <= cols, "ubn_gather: the crop H=%d x W=%d must be positive and fit rows=%d x cols=%d", H, W,
            rows, cols);
  SAT_CHECK(W % 4 == 0, "ubn_gather: W=%d must be a multiple of 4", W);
  SAT_CHECK(label_kind >= UBN_LABEL_U8 && label_kind <= UBN_LABEL_F32, "ubn_gather: label_kind=%d must be 1..3", label_kind);
  SAT_CHECK(K >= 1 && K <= UBN_MAX_CROPS, "ubn_gather: K=%d must be 1..%d", K, UBN_MAX_CROPS);
  SAT_CHECK(aligned(image, 4) && aligned(weight, 4) && aligned(table, 4) && aligned(out_image, 4) && aligned(out_weight, 4),
            "ubn_gather: image, weight, table, out_image and out_weight must be 4-byte aligned");
  SAT_CHECK(aligned(label, (uintptr_t)label_bytes(label_kind)), "ubn_gather: label must be %d-byte aligned", label_bytes(label_kind));
  SAT_CHECK(aligned(out_label, 8) && aligned(status, 8), "ubn_gather: out_label and status must be 8-byte aligned");
  const u64 px = (u64)P * (u64)rows * (u64)cols, lpx = stacked ? px / (u64)P : px, crop = (u64)K * (u64)H * (u64)W;
  const void* ins[4] = {image, label, weight, table};
  const u64 ibytes[4] = {4 * px, (u64)label_bytes(label_kind) * lpx, 4 * lpx, 4ull * UBN_TABLE_FIELDS * (u64)K};
  const void* outs[4] = {out_image, out_label, out_weight, status};
  const u64 obytes[4] = {4 * crop * (u64)(stacked ? P : 1), 8 * crop, 4 * crop, 8};
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 4; ++j) SAT_CHECK(!overlap(outs[i], obytes[i], ins[j], ibytes[j]), "ubn_gather: an output or status overlaps an input");
    for (int j = i + 1; j < 4; ++j) SAT_CHECK(!overlap(outs[i], obytes[i], outs[j], obytes[j]), "ubn_gather: two outputs overlap");
  }
  gather_t a;
  a.image = image; a.label = label; a.kind = label_kind; a.off = label_offset; a.weight = weight; a.stacked = stacked ? 1 : 0;
  a.P = P; a.rows = rows; a.cols = cols; a.H = H; a.W = W; a.table = table;
  a.out_image = out_image; a.out_label = (long long*)out_label; a.out_weight = out_weight; a.status = status;
  const u64 quads = (u64)H * (u64)(W / 4);
  gather_kernel<<<dim3((unsigned)((quads + UBN_LANES - 1) / UBN_LANES), (unsigned)K), dim3(UBN_LANES), 0, (hipStream_t)stream>>>(a);
  SAT_LAUNCH_CHECK("ubn_gather");
  return UBN_OK;
}
