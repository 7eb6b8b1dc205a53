// libubresnet_aug.so: device-side augmentation of training batches (include/ubresnet_aug.h).  It links against none of the other
// libraries and shares ubr_sat.h with them; the launch is a plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "../../include/ubresnet_aug.h"
#include "ubr_sat.h"

#define UBA_VERSION 1

SAT_RETURN_CODES(UBA);
SAT_EXPORTS(uba, UBA_VERSION)
using namespace sat;

namespace {

typedef long long ll2 __attribute__((ext_vector_type(2)));

// the whole launch, by value in the kernel's arguments: 1 KB of per-image words and the rest
struct AugK {
  const float* img;      // [B][P][H][W]
  const float* lab;      // [B][H][W] wire labels
  const float* wgt;      // [B][H][W] or null (every source weight is 1.0f)
  float* oimg;           // [B][P][H][W]
  long long* olab;       // [B][H][W]
  float* owgt;           // [B][H][W]
  int P, H, W;
  int groups;            // per row: ceil(W / UBA_LANE_PIXELS)
  unsigned items;        // B * H * groups  (<= B*H*W < 2^31)
  int pad, off;
  float thr;
  int pad_label;
  float pad_weight;
  int vec;               // the three outputs are 16-byte aligned and W % 4 == 0: vector stores
  unsigned par[UBA_MAX_BATCH];   // flip_rows | flip_cols << 1 | off_r << 2 | off_c << 17
};

// |v| < 2^31 -> trunc(v) + off (v_cvt_i32_f32 truncates toward zero; the value is in range); NaN fails the compare
__device__ __forceinline__ long long to_label(float v, int off) {
  return fabsf(v) < 2147483648.0f ? (long long)(int)v + (long long)off : LLONG_MIN;
}

// A lane owns UBA_LANE_PIXELS = 4 consecutive output columns of one row, with all planes; the groups of the batch are walked
// grid-strided.  Consecutive lanes write consecutive 16 bytes of an image row (32 of the labels); their source columns are
// consecutive too, ascending or -- under flip_cols -- descending, at an arbitrary element offset, so they are loaded by
// elements: a wave's loads of one j cover one contiguous stretch of a source row.  Row and image are decoded once per lane
// and trip in 32-bit arithmetic; element offsets into the P-plane image are 64-bit.  Whether the stores are vectors is the
// same for every lane (k.vec): that branch does not diverge.
template <bool THR>
__global__ __launch_bounds__(UBA_BLOCK) void augment_batch_kernel(const AugK k) {
  const unsigned stride = gridDim.x * UBA_BLOCK;
  const int Hp = k.H + 2 * k.pad, Wp = k.W + 2 * k.pad;
  for (unsigned g = blockIdx.x * UBA_BLOCK + threadIdx.x; g < k.items; g += stride) {
    const unsigned row = g / (unsigned)k.groups;            // b * H + r
    const int c0 = (int)(g - row * (unsigned)k.groups) * UBA_LANE_PIXELS;
    const unsigned b = row / (unsigned)k.H;
    const int r = (int)(row - b * (unsigned)k.H);
    const unsigned w = k.par[b];
    const int offr = (int)((w >> 2) & 0x7fffu), offc = (int)(w >> 17);
    int pr = r + offr;
    if (w & 1u) pr = Hp - 1 - pr;
    const int sr = pr - k.pad;
    const bool rowin = (unsigned)sr < (unsigned)k.H;
    int pc = c0 + offc;
    if (w & 2u) pc = Wp - 1 - pc;
    const int sc0 = pc - k.pad, step = (w & 2u) ? -1 : 1;   // source column of output column c0 + j: sc0 + j * step
    bool in[4];
    int sc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sc[j] = sc0 + j * step;
      in[j] = rowin && (unsigned)sc[j] < (unsigned)k.W && c0 + j < k.W;
    }
    const long spix = ((long)b * k.H + sr) * k.W;            // the source row in a one-plane array (used only where in[j])
    const long opix = (long)row * k.W + c0;                  // the lane's first output pixel in a one-plane array
    const long plane = (long)k.H * k.W;
    bool dark[4] = {true, true, true, true};
    for (int p = 0; p < k.P; ++p) {
      const long sbase = spix + ((long)b * (k.P - 1) + p) * plane;
      const long obase = opix + ((long)b * (k.P - 1) + p) * plane;
      float x[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        x[j] = in[j] ? k.img[sbase + sc[j]] : 0.0f;
        if (THR) {
          const bool lo = x[j] < k.thr;                      // NaN < thr is false
          if (in[j] && lo) x[j] = 0.0f;
          dark[j] = dark[j] && lo;
        }
      }
      if (k.vec) {
        *reinterpret_cast<float4*>(k.oimg + obase) = make_float4(x[0], x[1], x[2], x[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c0 + j < k.W) k.oimg[obase + j] = x[j];
      }
    }
    long long o[4];
    float q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (in[j]) {
        const float v = k.lab[spix + sc[j]];
        o[j] = (THR && dark[j]) ? 0ll : to_label(v, k.off);
        q[j] = k.wgt != nullptr ? k.wgt[spix + sc[j]] : 1.0f;
      } else {
        o[j] = (long long)k.pad_label;
        q[j] = k.pad_weight;
      }
    }
    if (k.vec) {
      ll2* d = reinterpret_cast<ll2*>(k.olab + opix);
      ll2 lo2, hi2;
      lo2.x = o[0]; lo2.y = o[1]; hi2.x = o[2]; hi2.y = o[3];
      d[0] = lo2;
      d[1] = hi2;
      *reinterpret_cast<float4*>(k.owgt + opix) = make_float4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < k.W) {
          k.olab[opix + j] = o[j];
          k.owgt[opix + j] = q[j];
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

extern "C" int uba_augment_batch(const float* image, const float* label_wire, const float* weight,
                                 float* image_out, int64_t* label_out, float* weight_out,
                                 int B, int P, int H, int W, int pad, const int32_t* params,
                                 int32_t label_offset, int use_threshold, float threshold,
                                 int32_t pad_label, float pad_weight, void* stream) {
  SAT_CHECK(image && label_wire, "uba_augment_batch: null source pointer (image, label_wire)");
  SAT_CHECK(image_out && label_out && weight_out, "uba_augment_batch: null destination pointer (image_out, label_out, weight_out)");
  SAT_CHECK(params, "uba_augment_batch: null params");
  SAT_CHECK(B >= 1 && P >= 1 && H >= 1 && W >= 1, "uba_augment_batch: B=%d P=%d H=%d W=%d must all be >= 1", B, P, H, W);
  SAT_CHECK(B <= UBA_MAX_BATCH, "uba_augment_batch: B=%d exceeds UBA_MAX_BATCH=%d", B, UBA_MAX_BATCH);
  const long long npix = (long long)B * H * W;
  SAT_CHECK(npix < (1ll << 31), "uba_augment_batch: B*H*W=%lld must be below 2^31", npix);
  SAT_CHECK(pad >= 0 && pad <= UBA_MAX_PAD, "uba_augment_batch: pad=%d must be 0..%d", pad, UBA_MAX_PAD);
  SAT_CHECK(aligned(image, 4) && aligned(label_wire, 4) && aligned(weight, 4) && aligned(image_out, 4) &&
                aligned(label_out, 8) && aligned(weight_out, 4),
            "uba_augment_batch: a pointer lacks its natural alignment (4 bytes for float, 8 for int64_t)");
  AugK k{};
  for (int b = 0; b < B; ++b) {
    const int32_t* q = params + 4 * b;
    SAT_CHECK((q[0] == 0 || q[0] == 1) && (q[1] == 0 || q[1] == 1),
              "uba_augment_batch: image %d: flips (%d, %d) must be 0 or 1", b, (int)q[0], (int)q[1]);
    SAT_CHECK(q[2] >= 0 && q[2] <= 2 * pad && q[3] >= 0 && q[3] <= 2 * pad,
              "uba_augment_batch: image %d: offsets (%d, %d) must be 0..2*pad=%d", b, (int)q[2], (int)q[3], 2 * pad);
    k.par[b] = (unsigned)q[0] | (unsigned)q[1] << 1 | (unsigned)q[2] << 2 | (unsigned)q[3] << 17;
  }
  const unsigned long long pix4 = 4ull * (unsigned long long)npix;
  const Region src[3] = {{"image", (uintptr_t)image, pix4 * P}, {"label_wire", (uintptr_t)label_wire, pix4},
                         {"weight", (uintptr_t)weight, pix4}};
  const Region dst[3] = {{"image_out", (uintptr_t)image_out, pix4 * P}, {"label_out", (uintptr_t)label_out, 2 * pix4},
                         {"weight_out", (uintptr_t)weight_out, pix4}};
  for (int d = 0; d < 3; ++d) {
    for (int s = 0; s < 3; ++s)
      SAT_CHECK(!overlap(src[s], dst[d]), "uba_augment_batch: %s overlaps %s (the call works out of place)", src[s].name, dst[d].name);
    for (int e = d + 1; e < 3; ++e)
      SAT_CHECK(!overlap(dst[d], dst[e]), "uba_augment_batch: %s overlaps %s", dst[d].name, dst[e].name);
  }
  k.img = image; k.lab = label_wire; k.wgt = weight;
  k.oimg = image_out; k.olab = (long long*)label_out; k.owgt = weight_out;
  k.P = P; k.H = H; k.W = W;
  k.groups = (W + UBA_LANE_PIXELS - 1) / UBA_LANE_PIXELS;
  k.items = (unsigned)((long long)B * H * k.groups);
  k.pad = pad; k.off = label_offset; k.thr = threshold; k.pad_label = pad_label; k.pad_weight = pad_weight;
  k.vec = aligned(image_out, 16) && aligned(label_out, 16) && aligned(weight_out, 16) && W % 4 == 0;
  long long blocks = ((long long)k.items + UBA_BLOCK - 1) / UBA_BLOCK;
  if (blocks > UBA_MAX_GRID) blocks = UBA_MAX_GRID;
  if (use_threshold)
    augment_batch_kernel<true><<<dim3((unsigned)blocks), dim3(UBA_BLOCK), 0, (hipStream_t)stream>>>(k);
  else
    augment_batch_kernel<false><<<dim3((unsigned)blocks), dim3(UBA_BLOCK), 0, (hipStream_t)stream>>>(k);
  SAT_LAUNCH_CHECK("uba_augment_batch");
  return UBA_OK;
}
