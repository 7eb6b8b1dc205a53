// libubresnet_blend.so: blended stitching of overlapping tiles (include/ubresnet_blend.h).  It links against none of the other
// libraries and shares ubr_sat.h with them; the launches are plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../../include/ubresnet_blend.h"
#include "../ubr_sat.h"

#define UBV_VERSION 1

SAT_RETURN_CODES(UBV);
SAT_EXPORTS(ubv, UBV_VERSION)
using namespace sat;

namespace {

// a unit: four floats of a row (vector path) or one (scalar path)
template <bool VEC> struct unit_of { typedef float type; };
template <> struct unit_of<true> { typedef float4 type; };

// the descriptors of a call, by value in the launch arguments: every index into them below is uniform over the workgroup
struct tiles_t {
  int plane[UBV_MAX_TILES], row0[UBV_MAX_TILES], col0[UBV_MAX_TILES];
};

// log(exp(a) + exp(b)) by the rules of the header (ubr_tta.hip's lae).  The four steps of the last line are separate fp32
// operations.
__device__ __forceinline__ float lae(float a, float b) {
  if (a != a || b != b) return a + b;
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  if (lo == -INFINITY) return hi;
  if (hi == lo) return __fadd_rn(hi, (float)M_LN2);
  return __fadd_rn(hi, log1pf(expf(__fsub_rn(lo, hi))));
}

__device__ __forceinline__ float blended(float a, float x, float wr, float wc) { return lae(a, __fadd_rn(x, __fadd_rn(wr, wc))); }
__device__ __forceinline__ float4 blended(float4 a, float4 x, float wr, float4 wc) {
  return make_float4(blended(a.x, x.x, wr, wc.x), blended(a.y, x.y, wr, wc.y), blended(a.z, x.z, wr, wc.z), blended(a.w, x.w, wr, wc.w));
}

__device__ __forceinline__ float minus_inf(float) { return -INFINITY; }
__device__ __forceinline__ float4 minus_inf(float4) { return make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY); }

template <bool VEC>
__global__ __launch_bounds__(UBV_BLOCK) void blend_begin_kernel(typename unit_of<VEC>::type* __restrict__ out, long nunits) {
  typedef typename unit_of<VEC>::type U;
  for (long i = (long)blockIdx.x * UBV_BLOCK + threadIdx.x; i < nunits; i += (long)gridDim.x * UBV_BLOCK) out[i] = minus_inf(U());
}

// Unit i of the tiles = (tile t, tile row y, unit xu of the row's twu units).  The lane of the FIRST tile of the call that covers
// the unit's view pixels owns them: it reads out once per class, applies every covering tile in ascending order and stores once;
// the lanes of the later covering tiles leave.  So every view pixel is written by one lane of the launch and no order between
// lanes shows.  On the vector path a unit is whole inside or whole outside every tile and the view (the launch checks what that
// needs), so one coverage test serves its four pixels.  The loops over the tiles are uniform: the descriptors are scalar reads.
template <bool VEC>
__global__ __launch_bounds__(UBV_BLOCK) void blend_kernel(const float* __restrict__ logp, const float* __restrict__ lw_rows,
                                                          const float* __restrict__ lw_cols, float* __restrict__ out,
                                                          const tiles_t T, int n, int C, int th, int tw, int twu, int rows,
                                                          int cols, unsigned nunits) {
  typedef typename unit_of<VEC>::type U;
  const unsigned per_tile = (unsigned)th * (unsigned)twu;
  const unsigned trips = (nunits + UBV_BLOCK - 1) / UBV_BLOCK;
  for (unsigned trip = blockIdx.x; trip < trips; trip += gridDim.x) {
    const unsigned i = trip * UBV_BLOCK + threadIdx.x;
    if (i >= nunits) continue;
    const int t = (int)(i / per_tile);
    const unsigned rem = i - (unsigned)t * per_tile;
    const int y = (int)(rem / (unsigned)twu);
    const int x = (int)(rem - (unsigned)y * (unsigned)twu) * (VEC ? 4 : 1);
    int p = 0, r = 0, c = 0;
    for (int j = 0; j < n; ++j)
      if (j == t) {
        p = T.plane[j];
        r = T.row0[j] + y;
        c = T.col0[j] + x;
      }
    if (r >= rows || c >= cols) continue;                      // the part of a tile outside the view
    unsigned long long cover = 0ull;
    bool first = true;
    for (int j = 0; j < n; ++j) {
      const bool in = T.plane[j] == p && (unsigned)(r - T.row0[j]) < (unsigned)th && (unsigned)(c - T.col0[j]) < (unsigned)tw;
      if (in) {
        cover |= 1ull << j;
        if (j < t) first = false;
      }
    }
    if (!first) continue;                                      // an earlier tile's lane owns these pixels
    for (int ch = 0; ch < C; ++ch) {
      U* dst = (U*)(out + (((long)p * C + ch) * rows + r) * cols + c);
      U a = *dst;
      for (int j = 0; j < n; ++j) {
        if (!((cover >> j) & 1ull)) continue;
        const int yy = r - T.row0[j], xx = c - T.col0[j];      // 0 <= yy < th, 0 <= xx (+ 3) < tw by the coverage test
        const float wr = lw_rows[(long)j * th + yy];
        const U wc = *(const U*)(lw_cols + (long)j * tw + xx);
        const U v = *(const U*)(logp + (((long)j * C + ch) * th + yy) * tw + xx);
        a = blended(a, v, wr, wc);
      }
      *dst = a;
    }
  }
}

}  // namespace

extern "C" int ubv_blend_begin(float* out, int64_t nelem, void* stream) {
  SAT_CHECK(out, "ubv_blend_begin: null pointer (out)");
  SAT_CHECK(nelem > 0 && nelem <= (int64_t)(1ll << 40), "ubv_blend_begin: nelem=%lld must be in 1..2^40", (long long)nelem);
  SAT_CHECK(aligned(out, 4), "ubv_blend_begin: out must be 4-byte aligned");
  const bool vec = nelem % 4 == 0 && aligned(out, 16);
  const long nunits = vec ? nelem / 4 : nelem;
  const long trips = (nunits + UBV_BLOCK - 1) / UBV_BLOCK;
  const dim3 grid((unsigned)(trips > UBV_MAX_GRID ? UBV_MAX_GRID : trips)), block(UBV_BLOCK);
  if (vec)
    blend_begin_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>((float4*)out, nunits);
  else
    blend_begin_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(out, nunits);
  SAT_LAUNCH_CHECK("ubv_blend_begin");
  return UBV_OK;
}

extern "C" int ubv_blend_tiles(const float* logp, int C, int th, int tw, const int32_t* desc_host, int n, const float* lw_rows,
                               const float* lw_cols, float* out, int P, int rows, int cols, void* stream) {
  SAT_CHECK(logp && lw_rows && lw_cols && out, "ubv_blend_tiles: null pointer (logp, lw_rows, lw_cols, out)");
  SAT_CHECK(desc_host, "ubv_blend_tiles: desc_host is null");
  SAT_CHECK(n >= 1 && n <= UBV_MAX_TILES, "ubv_blend_tiles: n=%d must be 1..%d (UBV_MAX_TILES)", n, UBV_MAX_TILES);
  SAT_CHECK(C >= 1 && C <= UBV_MAX_CLASSES, "ubv_blend_tiles: C=%d must be 1..%d (UBV_MAX_CLASSES)", C, UBV_MAX_CLASSES);
  SAT_CHECK(th > 0 && tw > 0, "ubv_blend_tiles: th=%d, tw=%d must be positive", th, tw);
  SAT_CHECK((long long)th * tw <= (1ll << 24), "ubv_blend_tiles: th=%d x tw=%d exceeds 2^24 pixels", th, tw);
  SAT_CHECK(P >= 1 && rows > 0 && cols > 0, "ubv_blend_tiles: P=%d, rows=%d, cols=%d must be positive", P, rows, cols);
  SAT_CHECK((long long)P * C <= (1ll << 40) / rows / cols, "ubv_blend_tiles: P=%d x C=%d x rows=%d x cols=%d exceeds 2^40 elements",
            P, C, rows, cols);
  tiles_t T;
  bool col4 = true;
  for (int j = 0; j < UBV_MAX_TILES; ++j) T.plane[j] = T.row0[j] = T.col0[j] = 0;
  for (int j = 0; j < n; ++j) {
    const int32_t* d = desc_host + 3 * j;
    SAT_CHECK(d[0] >= 0 && d[0] < P, "ubv_blend_tiles: tile %d: plane=%d must be in 0..P-1 (P=%d)", j, (int)d[0], P);
    SAT_CHECK(d[1] >= 0 && d[1] < rows && d[2] >= 0 && d[2] < cols,
              "ubv_blend_tiles: tile %d: origin (%d, %d) is outside the %d x %d view", j, (int)d[1], (int)d[2], rows, cols);
    T.plane[j] = d[0];
    T.row0[j] = d[1];
    T.col0[j] = d[2];
    col4 = col4 && d[2] % 4 == 0;
  }
  SAT_CHECK(aligned(logp, 4) && aligned(lw_rows, 4) && aligned(lw_cols, 4) && aligned(out, 4),
            "ubv_blend_tiles: logp, lw_rows, lw_cols and out must be 4-byte aligned");
  const unsigned long long obytes = 4ull * (unsigned long long)P * C * rows * cols;
  SAT_CHECK(!overlap(logp, 4ull * n * C * th * tw, out, obytes), "ubv_blend_tiles: logp overlaps out");
  SAT_CHECK(!overlap(lw_rows, 4ull * n * th, out, obytes), "ubv_blend_tiles: lw_rows overlaps out");
  SAT_CHECK(!overlap(lw_cols, 4ull * n * tw, out, obytes), "ubv_blend_tiles: lw_cols overlaps out");
  const bool vec = col4 && tw % 4 == 0 && cols % 4 == 0 && aligned(logp, 16) && aligned(lw_cols, 16) && aligned(out, 16);
  const int twu = vec ? tw / 4 : tw;
  const unsigned nunits = (unsigned)n * (unsigned)th * (unsigned)twu;                   // <= 64 * 2^24
  const unsigned trips = (nunits + UBV_BLOCK - 1) / UBV_BLOCK;
  const dim3 grid(trips > UBV_MAX_GRID ? UBV_MAX_GRID : trips), block(UBV_BLOCK);
  if (vec)
    blend_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(logp, lw_rows, lw_cols, out, T, n, C, th, tw, twu, rows, cols, nunits);
  else
    blend_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(logp, lw_rows, lw_cols, out, T, n, C, th, tw, twu, rows, cols, nunits);
  SAT_LAUNCH_CHECK("ubv_blend_tiles");
  return UBV_OK;
}
