// libubresnet_det.so: detector effects on a prepared training batch, in place (include/ubresnet_det.h).  It links against none of
// the other libraries and shares ubr_sat.h with them; the launch is a plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/ubresnet_det.h"
#include "ubr_det_rule.h"
#include "ubr_sat.h"

#define UBX_VERSION 1

SAT_RETURN_CODES(UBX);
SAT_EXPORTS(ubx, UBX_VERSION)
using namespace sat;

namespace {

// the whole launch, by value in the kernel's arguments; the per-plane rows are in `tab` on the device
struct DetK {
  float* img;            // [B][P][H][W]
  long long* lab;        // [B][H][W] or null (then set_label == 0)
  float* wgt;            // [B][H][W] or null (then set_weight == 0)
  const uint32_t* tab;   // [B][P][rowwords]: gain bits, then the mask words
  int P, H, W;
  int groups;            // per row: ceil(W / UBX_LANE_PIXELS)
  unsigned items;        // B * H * groups  (<= B*H*W < 2^31)
  int rowwords;          // 1 + ceil(W / 32)
  float sigma;
  int noise_all;
  uint32_t seed, seq;
  int set_label, set_weight;
  long long dead_label;
  float dead_weight;
  int vec;               // image is 16-byte aligned and W % 4 == 0: vector loads and stores
};

// A lane owns UBX_LANE_PIXELS = 4 consecutive columns c0 .. c0 + 3 of one row, with all planes; the groups of the batch are
// walked grid-strided.  c0 is a multiple of 4, so the four mask bits sit in one word of the row of (b, p): the row's words are
// read once per lane, plane and trip (the table is a few KB and stays in the caches).  One Philox call per plane serves the
// four columns, and is made only where one of them takes noise: on thresholded crops, 97 to 99 % zeros, most lanes make none.
// NOISE = false (sigma == 0) holds no random number and no library call at all.  Whether loads and stores are vectors is the
// same for every lane (k.vec): that branch does not diverge.  Every element is read and written by the one lane that owns it.
template <bool NOISE>
__global__ __launch_bounds__(UBX_BLOCK) void detector_kernel(const DetK k) {
  const unsigned stride = gridDim.x * UBX_BLOCK;
  const long plane = (long)k.H * k.W;
  for (unsigned g = blockIdx.x * UBX_BLOCK + threadIdx.x; g < k.items; g += stride) {
    const unsigned row = g / (unsigned)k.groups;            // b * H + r
    const unsigned grp = g - row * (unsigned)k.groups;
    const int c0 = (int)grp * UBX_LANE_PIXELS;
    const unsigned b = row / (unsigned)k.H;
    const unsigned r = row - b * (unsigned)k.H;
    const int left = k.W - c0;                              // >= 1
    const uint32_t valid = left >= 4 ? 0xFu : ((1u << left) - 1u);   // bits at or beyond W are ignored
    const long opix = (long)row * k.W + c0;                 // the lane's first pixel in a one-plane array
    uint32_t alldead = valid;
    for (int p = 0; p < k.P; ++p) {
      const uint32_t* trow = k.tab + ((long)b * k.P + p) * k.rowwords;
      const uint32_t gain = trow[0];
      const uint32_t dead = (trow[1 + (c0 >> 5)] >> (c0 & 31)) & valid;
      alldead &= dead;
      float* q = k.img + opix + ((long)b * (k.P - 1) + p) * plane;
      float x[4];
      if (k.vec) {
        const float4 v = *reinterpret_cast<const float4*>(q);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = (valid >> j & 1u) ? q[j] : 0.0f;
      }
      uint32_t noise = 0;                                   // the columns that take noise
      if (NOISE) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (ubx::noisy(x[j], k.noise_all != 0)) noise |= 1u << j;
        noise &= valid & ~dead;
      }
      if (dead == 0 && gain == UBX_ONE_BITS && noise == 0) continue;   // nothing changes: the bytes stay as they are
      float y[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = ubx::gained(x[j], (dead >> j & 1u) != 0, gain);
      if (NOISE && noise != 0) {
        const ubx::Words w = ubx::words(k.seed, k.seq, grp, r, b * (unsigned)k.P + (unsigned)p);
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
          if ((noise >> (2 * pair) & 3u) == 0) continue;
          const float rad = ubx::radius(w.w[2 * pair]), ang = ubx::angle(w.w[2 * pair + 1]);
          if (noise >> (2 * pair) & 1u) y[2 * pair] = ubx::noised(y[2 * pair], k.sigma, ubx::normal_even(rad, ang));
          if (noise >> (2 * pair + 1) & 1u) y[2 * pair + 1] = ubx::noised(y[2 * pair + 1], k.sigma, ubx::normal_odd(rad, ang));
        }
      }
      if (k.vec) {
        *reinterpret_cast<float4*>(q) = make_float4(y[0], y[1], y[2], y[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (valid >> j & 1u) q[j] = y[j];
      }
    }
    if (alldead != 0 && (k.set_label | k.set_weight)) {    // dead in every plane: runs of dead wires are rare and short
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (alldead >> j & 1u) {
          if (k.set_label) k.lab[opix + j] = k.dead_label;
          if (k.set_weight) k.wgt[opix + j] = k.dead_weight;
        }
    }
  }
}

struct Region {
  const char* name;
  uintptr_t lo;
  unsigned long long bytes;
};

inline bool overlap(const Region& a, const Region& b) {
  return a.lo != 0 && b.lo != 0 && a.lo < b.lo + b.bytes && b.lo < a.lo + a.bytes;
}

}  // namespace

extern "C" int ubx_apply(float* image, int64_t* label, float* weight, int B, int P, int H, int W, const uint32_t* table,
                         float sigma, int noise_all, uint32_t seed, uint32_t seq,
                         int set_label, int64_t dead_label, int set_weight, float dead_weight, void* stream) {
  SAT_CHECK(image && table, "ubx_apply: null pointer (image, table)");
  SAT_CHECK(label || !set_label, "ubx_apply: null label with set_label");
  SAT_CHECK(weight || !set_weight, "ubx_apply: null weight with set_weight");
  SAT_CHECK(B >= 1 && P >= 1 && H >= 1 && W >= 1, "ubx_apply: B=%d P=%d H=%d W=%d must all be >= 1", B, P, H, W);
  const long long npix = (long long)B * H * W;
  SAT_CHECK(npix < (1ll << 31), "ubx_apply: B*H*W=%lld must be below 2^31", npix);
  SAT_CHECK(isfinite(sigma) && sigma >= 0.0f, "ubx_apply: sigma=%g must be finite and >= 0", (double)sigma);
  SAT_CHECK(isfinite(dead_weight), "ubx_apply: dead_weight=%g must be finite", (double)dead_weight);
  SAT_CHECK(aligned(image, 4) && aligned(label, 8) && aligned(weight, 4) && aligned(table, 4),
            "ubx_apply: a pointer lacks its natural alignment (4 bytes for float and uint32, 8 for int64_t)");
  const int rowwords = 1 + (W + 31) / 32;
  const unsigned long long pix4 = 4ull * (unsigned long long)npix;
  const Region reg[4] = {{"image", (uintptr_t)image, pix4 * P}, {"label", (uintptr_t)label, 2 * pix4},
                         {"weight", (uintptr_t)weight, pix4}, {"table", (uintptr_t)table, 4ull * B * P * rowwords}};
  for (int d = 0; d < 4; ++d)
    for (int e = d + 1; e < 4; ++e)
      SAT_CHECK(!overlap(reg[d], reg[e]), "ubx_apply: %s overlaps %s", reg[d].name, reg[e].name);
  DetK k{};
  k.img = image; k.lab = (long long*)label; k.wgt = weight; k.tab = table;
  k.P = P; k.H = H; k.W = W;
  k.groups = (W + UBX_LANE_PIXELS - 1) / UBX_LANE_PIXELS;
  k.items = (unsigned)((long long)B * H * k.groups);
  k.rowwords = rowwords;
  k.sigma = sigma; k.noise_all = noise_all != 0;
  k.seed = seed; k.seq = seq;
  k.set_label = set_label != 0; k.set_weight = set_weight != 0;
  k.dead_label = (long long)dead_label; k.dead_weight = dead_weight;
  k.vec = aligned(image, 16) && W % 4 == 0;
  long long blocks = ((long long)k.items + UBX_BLOCK - 1) / UBX_BLOCK;
  if (blocks > UBX_MAX_GRID) blocks = UBX_MAX_GRID;
  if (sigma > 0.0f)
    detector_kernel<true><<<dim3((unsigned)blocks), dim3(UBX_BLOCK), 0, (hipStream_t)stream>>>(k);
  else
    detector_kernel<false><<<dim3((unsigned)blocks), dim3(UBX_BLOCK), 0, (hipStream_t)stream>>>(k);
  SAT_LAUNCH_CHECK("ubx_apply");
  return UBX_OK;
}
