// ubr_aspp_front: the five branches of one ASPP level (models/ASPP_ResNet.py:227-263, eval mode, BatchNorm folded) in ONE launch.
//
//   acat[..., 16b : 16b+16] = relu(conv_b(e) + bias_b)    b = 0..3: 1x1, 3x3 d1, 3x3 d3, 3x3 d5 (C -> 16 each)
//   acat[..., 64 : 64+C]    = MaxPool2d(3, 1, 1)(e)
//
// A workgroup (4 waves) owns an 8 x 16 pixel tile.  Per K-chunk of 4 channel units (32 f16/bf16 or 16 fp32 channels -- one
// MFMA K-step) it stages the 18 x 26 halo tile of `e` (5 pixels on every side, the d5 branch) and the chunk's 28 weight taps in
// LDS, then
//   * every wave runs the 28 taps over its two pixel rows: a branch is exactly one 16-wide tile of the MFMA, weights are the A
//     operand (rows = output channels) and pixels the B operand (columns = the 16 pixels of a row), so a lane ends up with four
//     consecutive output channels of one pixel and stores them as one 8- or 16-byte word;
//   * all threads take the 3x3 maximum of the same staged channels on the VALU and store the pool slice.
// `e` is read from HBM once (plus halo) instead of five times.  The next chunk's global loads are issued before the MFMAs of
// the current one and parked in registers.
//
// LDS images.  Halo: [unit q][pixel] 16-byte slots, unit plane padded to a multiple of 16 slots: the 16 lanes of an MFMA operand
// read (16 consecutive pixels of a row, at any dilated tap offset) cover 16 consecutive slots, and the four units of the wave's
// lane quads sit a multiple of 16 slots apart, so each 16-lane ds_read_b128 group touches every slot of the 256-byte bank row
// once -- no conflict at any dx.  Weights: [tap][lane] in fragment order, the same property.
#include "ubr_common.h"
#include "ubr_host.h"

namespace {

constexpr int A_TH = 8, A_TW = 16, A_HALO = 5;
constexpr int A_HH = A_TH + 2 * A_HALO, A_HW = A_TW + 2 * A_HALO;      // 18 x 26
constexpr int A_NPIX = A_HH * A_HW;                                    // 468
constexpr int A_PLANE = (A_NPIX + 15) / 16 * 16;                       // 480 slots per unit plane
constexpr int A_NTAPS = 28;
constexpr int A_HL = (4 * A_NPIX + 255) / 256;                         // halo units per thread and chunk (8)
constexpr int A_WL = A_NTAPS * 64 / 256;                               // weight units per thread and chunk (7)

struct AsppK {
  const char* x; long x_sn; int x_sy, x_sx;        // bytes
  const char* w;
  const float* bias;
  char* y; long y_sn; int y_sy, y_sx;              // bytes
  int N, H, W, KU;                                 // KU = C / CPU
  int tiles_x, tiles_y;
};

// tap t of the packed image: B1 (1 tap), then B2 / B3 / B4 (3x3 row-major, dilation 1 / 3 / 5)
__host__ __device__ constexpr int aspp_tap_branch(int t) { return t == 0 ? 0 : 1 + (t - 1) / 9; }
__host__ __device__ constexpr int aspp_tap_dy(int t) { return t == 0 ? 0 : (((t - 1) % 9) / 3 - 1) * (2 * ((t - 1) / 9) + 1); }
__host__ __device__ constexpr int aspp_tap_dx(int t) { return t == 0 ? 0 : (((t - 1) % 9) % 3 - 1) * (2 * ((t - 1) / 9) + 1); }

template <typename T> __device__ __forceinline__ void aspp_store4(char* p, const float* v);
template <> __device__ __forceinline__ void aspp_store4<float>(char* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void aspp_store4<bf16_t>(char* p, const float* v) {
  *reinterpret_cast<uint2*>(p) = make_uint2(ET<bf16_t>::pk2(v[0], v[1]), ET<bf16_t>::pk2(v[2], v[3]));
}
template <> __device__ __forceinline__ void aspp_store4<f16_t>(char* p, const float* v) {
  f16x4_t h;
#pragma unroll
  for (int i = 0; i < 4; ++i) h[i] = (_Float16)v[i];
  *reinterpret_cast<uint2*>(p) = __builtin_bit_cast(uint2, h);
}

template <typename T>
__global__ __launch_bounds__(256) void aspp_front_kernel(const AsppK k) {
  constexpr int CPU = ET<T>::CPU;
  constexpr int ESZ = 16 / CPU;
  __shared__ uint4 halo[4 * A_PLANE];
  __shared__ uint4 wl[A_NTAPS * 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, r = lane & 15;
  int b = blockIdx.x;
  const int tx = b % k.tiles_x; b /= k.tiles_x;
  const int ty = b % k.tiles_y;
  const int n = b / k.tiles_y;
  const int ty0 = ty * A_TH, tx0 = tx * A_TW;
  const char* xn = k.x + (long)n * k.x_sn;
  char* yn = k.y + (long)n * k.y_sn;

  // this thread's halo slots: byte offset of the pixel inside the image (-1: outside, zero-filled) and the LDS slot
  int hoff[A_HL], hslot[A_HL];
#pragma unroll
  for (int i = 0; i < A_HL; ++i) {
    const int j = tid + 256 * i;
    const int uq = j & 3, p = j >> 2;
    const int hy = p / A_HW, hx = p - hy * A_HW;
    const int iy = ty0 - A_HALO + hy, ix = tx0 - A_HALO + hx;
    hslot[i] = p < A_NPIX ? uq * A_PLANE + p : -1;
    hoff[i] = (p < A_NPIX && iy >= 0 && iy < k.H && ix >= 0 && ix < k.W) ? iy * k.x_sy + ix * k.x_sx + uq * 16 : -1;
  }

  uint4 hreg[A_HL], wreg[A_WL];
  auto fetch = [&](int c) {
#pragma unroll
    for (int i = 0; i < A_HL; ++i)
      hreg[i] = hoff[i] >= 0 ? ldg16(xn + hoff[i] + c * 64) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int i = 0; i < A_WL; ++i) {
      const int j = tid + 256 * i;
      wreg[i] = ldg16(k.w + ((long)((j >> 6) * k.KU + c * 4) * 16 + (j & 63)) * 16);
    }
  };
  auto park = [&]() {
#pragma unroll
    for (int i = 0; i < A_HL; ++i)
      if (hslot[i] >= 0) halo[hslot[i]] = hreg[i];
#pragma unroll
    for (int i = 0; i < A_WL; ++i) wl[tid + 256 * i] = wreg[i];
  };

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) { acc[i][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  const int nchunk = k.KU >> 2;
  fetch(0);
  park();
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    if (c + 1 < nchunk) fetch(c + 1);
    // ---- 28 taps on the matrix cores: rows 2*wave, 2*wave + 1 of the tile ----
    const int a0 = q * A_PLANE + (2 * wave + A_HALO) * A_HW + A_HALO + r;
#pragma unroll
    for (int t = 0; t < A_NTAPS; ++t) {
      const uint4 wv = wl[t * 64 + lane];
      const int o = a0 + aspp_tap_dy(t) * A_HW + aspp_tap_dx(t);
      const uint4 p0 = halo[o], p1 = halo[o + A_HW];
      const int br = aspp_tap_branch(t);
      acc[br][0] = mma_step<T>(acc[br][0], wv, p0);
      acc[br][1] = mma_step<T>(acc[br][1], wv, p1);
    }
    // ---- 3x3 stride-1 maximum of the same channels (padding = -inf) ----
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int item = tid + 256 * it;
      const int pix = item & 127, uq = item >> 7;
      const int row = pix >> 4, col = pix & 15;
      const int oy = ty0 + row, ox = tx0 + col;
      if (oy < k.H && ox < k.W) {
        float m[CPU];
#pragma unroll
        for (int e = 0; e < CPU; ++e) m[e] = -__builtin_inff();
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int iy = oy + dy, ix = ox + dx;
            if (iy >= 0 && iy < k.H && ix >= 0 && ix < k.W) {
              float f[CPU];
              ET<T>::unpack(halo[uq * A_PLANE + (row + A_HALO + dy) * A_HW + col + A_HALO + dx], f);
#pragma unroll
              for (int e = 0; e < CPU; ++e) m[e] = f[e] > m[e] ? f[e] : m[e];
            }
          }
        }
        stg16(yn + oy * k.y_sy + ox * k.y_sx + (64 + (c * 4 + uq) * CPU) * ESZ, ET<T>::pack(m));
      }
    }
    __syncthreads();
    if (c + 1 < nchunk) {
      park();
      __syncthreads();
    }
  }

  // ---- epilogue: + folded bias, ReLU, store 4 consecutive channels of one pixel per lane and branch ----
  const int ox = tx0 + r;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int oy = ty0 + 2 * wave + rr;
    if (oy < k.H && ox < k.W) {
      char* yp = yn + oy * k.y_sy + ox * k.y_sx;
#pragma unroll
      for (int br = 0; br < 4; ++br) {
        const int ch = 16 * br + 4 * q;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float s = acc[br][rr][i] + k.bias[ch + i];
          v[i] = s > 0.f ? s : 0.f;
        }
        aspp_store4<T>(yp + ch * ESZ, v);
      }
    }
  }
}

}  // namespace

extern "C" int ubr_aspp_front(const ubr_aspp_front_desc* d, void* stream) {
  UBR_CHECK(d != nullptr, "ubr_aspp_front: null descriptor");
  UBR_CHECK(ubr_dtype_ok(d->dtype), "ubr_aspp_front: bad dtype %d", d->dtype);
  const int cpu = ubr_cpu(d->dtype), esz = ubr_esize(d->dtype);
  UBR_CHECK(d->N > 0 && d->H > 0 && d->W > 0, "ubr_aspp_front: empty extent");
  UBR_CHECK(d->C > 0 && d->C % (4 * cpu) == 0, "ubr_aspp_front: C=%d must be a positive multiple of %d", d->C, 4 * cpu);
  UBR_CHECK(d->x.p && d->w && d->bias && d->y.p, "ubr_aspp_front: null pointer");
  UBR_CHECK(ubr_aligned16(d->x.p) && ubr_aligned16(d->w) && ubr_aligned16(d->y.p), "ubr_aspp_front: x / w / y must be 16-byte aligned");
  UBR_CHECK((d->x.sx * esz) % 16 == 0 && (d->x.sy * esz) % 16 == 0 && (d->x.sn * esz) % 16 == 0 &&
            (d->y.sx * esz) % 16 == 0 && (d->y.sy * esz) % 16 == 0 && (d->y.sn * esz) % 16 == 0,
            "ubr_aspp_front: strides must keep 16-byte alignment");
  UBR_CHECK(d->x.sx >= d->C, "ubr_aspp_front: x pixel stride %ld < C %d", (long)d->x.sx, d->C);
  UBR_CHECK(d->y.sx >= 64 + d->C, "ubr_aspp_front: y pixel stride %ld < 64 + C = %d", (long)d->y.sx, 64 + d->C);
  // the kernel forms iy*sy + ix*sx + channel offsets in 32 bits, relative to the image base: bound the whole span of one image
  UBR_CHECK(d->x.sy >= 0 && d->x.sx >= 0 && d->y.sy >= 0 && d->y.sx >= 0 && d->x.sn >= 0 && d->y.sn >= 0,
            "ubr_aspp_front: negative strides are not supported");
  UBR_CHECK(((long)(d->H - 1) * d->x.sy + (long)(d->W - 1) * d->x.sx + d->C) * esz < (1L << 31) &&
            ((long)(d->H - 1) * d->y.sy + (long)(d->W - 1) * d->y.sx + 64 + d->C) * esz < (1L << 31),
            "ubr_aspp_front: image too large for 32-bit offsets");
  AsppK k{};
  k.x = (const char*)d->x.p; k.x_sn = d->x.sn * esz; k.x_sy = (int)(d->x.sy * esz); k.x_sx = (int)(d->x.sx * esz);
  k.w = (const char*)d->w; k.bias = d->bias;
  k.y = (char*)d->y.p; k.y_sn = d->y.sn * esz; k.y_sy = (int)(d->y.sy * esz); k.y_sx = (int)(d->y.sx * esz);
  k.N = d->N; k.H = d->H; k.W = d->W; k.KU = d->C / cpu;
  k.tiles_x = ubr_cdiv(d->W, A_TW); k.tiles_y = ubr_cdiv(d->H, A_TH);
  const long wgs = (long)k.tiles_x * k.tiles_y * d->N;
  UBR_CHECK(wgs < (1L << 31), "ubr_aspp_front: too many tiles");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)wgs), block(256);
  if (d->dtype == UBR_F32) ubr_launch(aspp_front_kernel<float>, grid, block, 0, st, k);
  else if (d->dtype == UBR_BF16) ubr_launch(aspp_front_kernel<bf16_t>, grid, block, 0, st, k);
  else ubr_launch(aspp_front_kernel<f16_t>, grid, block, 0, st, k);
  UBR_LAUNCH_CHECK("ubr_aspp_front");
  return UBR_OK;
}
