// The epilogue contract of the three conv kernels of ubr_conv.hip (conv_igemm_kernel, conv_thin_kernel, conv_pc_kernel), and the
// pieces of it that the kernels share.
//
// A lane holds 4 consecutive output channels of one pixel per accumulator fragment.  Per value, in this order:
//   v = acc + bias;  ReLU if act & 1;  v += addend (gated by a ReLU bit mask where the descriptor has one);  ReLU if act & 2;
// then the value enters the per-channel statistics (plain sums, or the BatchNorm-backward sums on the storage-rounded value) and
// is stored (NHWC in the storage type, or the fused log-softmax in fp32 NCHW).  Results do not depend on which kernel a launch
// gets.  conv_igemm_kernel is written on everything below.  All three kernels share the bias load, the 4-channel primitives and the
// stamp macro; conv_thin_kernel also the statistics step, the log-softmax tail and the statistics flush.  NOT shared:
// conv_thin_kernel's value loop, and conv_pc_kernel's two epilogue paths and per-wave flush, still spell the rule out themselves --
// on finish4 / generic_finish4 / FastEpi those kernels gained scratch (profiles/conv_epilogue_refactor.txt has the figures).
// Whoever changes the rule changes it in finish4, in conv_thin_kernel and twice in conv_pc_kernel.
#pragma once
#include <type_traits>
#include "ubr_common.h"

namespace {

template <typename T> __device__ __forceinline__ void store4(char* p, const float* v);
template <> __device__ __forceinline__ void store4<float>(char* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void store4<bf16_t>(char* p, const float* v) {
  *reinterpret_cast<uint2*>(p) = make_uint2(ET<bf16_t>::pk2(v[0], v[1]), ET<bf16_t>::pk2(v[2], v[3]));
}
template <> __device__ __forceinline__ void store4<f16_t>(char* p, const float* v) {
  f16x4_t h; h[0] = (_Float16)v[0]; h[1] = (_Float16)v[1]; h[2] = (_Float16)v[2]; h[3] = (_Float16)v[3];
  *reinterpret_cast<uint2*>(p) = __builtin_bit_cast(uint2, h);
}
template <typename T> __device__ __forceinline__ void load4(const char* p, float* v);
template <> __device__ __forceinline__ void load4<float>(const char* p, float* v) {
  float4 f = *reinterpret_cast<const float4*>(p); v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
}
template <> __device__ __forceinline__ void load4<bf16_t>(const char* p, float* v) {
  uint2 u = *reinterpret_cast<const uint2*>(p);
  v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
  v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
}
template <> __device__ __forceinline__ void load4<f16_t>(const char* p, float* v) {
  f16x4_t h = __builtin_bit_cast(f16x4_t, *reinterpret_cast<const uint2*>(p));
  v[0] = (float)h[0]; v[1] = (float)h[1]; v[2] = (float)h[2]; v[3] = (float)h[3];
}

// v rounded to the storage type (what a later pass would read back from the stored tensor)
template <typename T> __device__ __forceinline__ void round4(const float* v, float* r);
template <> __device__ __forceinline__ void round4<float>(const float* v, float* r) { r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3]; }
template <> __device__ __forceinline__ void round4<bf16_t>(const float* v, float* r) {
  // round-to-nearest-even on the bit pattern (integer ops; NaN kept as NaN): the result v_cvt_pk_bf16_f32 gives
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t u = __float_as_uint(v[i]);
    const uint32_t rne = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    r[i] = __uint_as_float((u & 0x7fffffffu) > 0x7f800000u ? (u | 0x00400000u) & 0xffff0000u : rne);
  }
}
template <> __device__ __forceinline__ void round4<f16_t>(const float* v, float* r) {
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = (float)(_Float16)v[i];
}

// Two pixel fragments' 4-channel groups (fp32) -> this lane's 16 output bytes after the quad exchange: lane (q, l16) holds channels
// 4q..4q+3 of pixel l16 of fragment 0 (X) and of fragment 1 (Y), 8 bytes each; v_permlane16_swap exchanges the odd quads of X with
// the even quads of Y, so that afterwards an even quad holds channels 4q..4q+7 of its fragment-0 pixel and an odd quad channels
// 4(q-1)..4q+3 of its fragment-1 pixel -- 16 contiguous bytes.
// bf16: converts and swaps in ONE asm statement with early-clobber outputs; wait states by hand (hipcc pads nothing inside asm).
// (The wrong lanes 12-15 once seen after this block were the 16-byte store hazard described at buf_store16: a convert writing the
// data registers of the store issued just before it.)
template <typename T> __device__ __forceinline__ uint4 pack_swap_pair(const float* v0, const float* v1);
template <> __device__ __forceinline__ uint4 pack_swap_pair<bf16_t>(const float* v0, const float* v1) {
  uint2 X, Y;
  asm volatile("v_cvt_pk_bf16_f32 %0, %4, %5\n\tv_cvt_pk_bf16_f32 %1, %6, %7\n\tv_cvt_pk_bf16_f32 %2, %8, %9\n\t"
               "v_cvt_pk_bf16_f32 %3, %10, %11\n\ts_nop 1\n\tv_permlane16_swap_b32 %0, %2\n\tv_permlane16_swap_b32 %1, %3\n\ts_nop 3"
               : "=&v"(X.x), "=&v"(X.y), "=&v"(Y.x), "=&v"(Y.y)
               : "v"(v0[0]), "v"(v0[1]), "v"(v0[2]), "v"(v0[3]), "v"(v1[0]), "v"(v1[1]), "v"(v1[2]), "v"(v1[3]));
  return make_uint4(X.x, X.y, Y.x, Y.y);
}
template <> __device__ __forceinline__ uint4 pack_swap_pair<f16_t>(const float* v0, const float* v1) {
  f16x4_t a, b;
#pragma unroll
  for (int r = 0; r < 4; ++r) { a[r] = (_Float16)v0[r]; b[r] = (_Float16)v1[r]; }
  uint2 X = __builtin_bit_cast(uint2, a), Y = __builtin_bit_cast(uint2, b);
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3\n\ts_nop 3" : "+v"(X.x), "+v"(Y.x), "+v"(X.y), "+v"(Y.y));
  return make_uint4(X.x, X.y, Y.x, Y.y);
}
template <> __device__ __forceinline__ uint4 pack_swap_pair<float>(const float* v0, const float* v1) { return make_uint4(0u, 0u, 0u, 0u); }

typedef __attribute__((ext_vector_type(2))) unsigned ubr_u2;

// 16-byte buffer store with a scalar offset.  gfx950 reads a store's data registers over several cycles; a VALU write to them in the
// next instruction slot corrupts what the store sends (observed: the second dword of lanes 12-15 of each 16-lane row).  hipcc (ROCm 7.2)
// inserts the wait state for stores wider than 8 bytes only when soffset is NOT an SGPR (it assumes the scalar operand fetch hides the
// hazard -- it does not on this part: ISA of the fp32 epilogues, `buffer_store_dwordx4 v[96:99], v135, s[24:27], s90 offen` directly
// followed by `v_pk_add_f32 v[96:97], ...`).  So 16-byte stores fold the scalar offset into the vector one (one v_add) and leave
// soffset zero, which puts them under the compiler's own hazard handling; 8-byte stores are not affected.  (This is what the "stale
// lanes 12-15" failures of the training epilogues in round 3 were; they had first been put down to MFMA result latency and to a
// v_cvt_pk_bf16_f32 next to v_permlane16_swap.)
__device__ __forceinline__ void buf_store16(const ubr_u4& v, __amdgpu_buffer_rsrc_t r, int voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b128(v, r, voff + soff, 0, 0);
}

// diagnostic build (-DUBR_CONV_STAMPS): add the cycles since the last stamp to acc_ (the kernel declares the running stamp t_)
#ifdef UBR_CONV_STAMPS
#define UBR_CONV_STAMP(acc_) do { unsigned long long n_ = __builtin_amdgcn_s_memtime(); acc_ += n_ - t_; t_ = n_; } while (0)
#else
#define UBR_CONV_STAMP(acc_) do { } while (0)
#endif

// bias of this lane's 4-channel group of every cout fragment (zero beyond Cout)
template <int NT> __device__ __forceinline__ void load_bias(float (&bs)[NT][4], const float* bias, int n0, int q, int Cout) {
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ch = n0 + j * 16 + 4 * q + r;
      bs[j][r] = (bias != nullptr && ch < Cout) ? bias[ch] : 0.f;
    }
}

// The value rule of one 4-channel group.  `add`: an addend enters this group (the descriptor has one and the group lies inside
// the output).  `addend(a4, mb)` produces the group's addend and, where has_mask, its mask bits; it runs only when `add`, after the
// first ReLU.  The ReLU bit mask on the addend (bit r of mb gates channel r) is applied as a select, a = bit ? a : 0, then v += a.
// (conv_thin_kernel, EXT == 2, does NOT use this rule for its masked addend: it forms v = fma(a, (float)bit, v) in its own loop.  The two
// give the same sum for a finite a and differ for a non-finite addend under a zero bit -- the select drops it, 0 * inf is NaN -- so
// each kernel keeps the form it has.)
template <typename AD>
__device__ __forceinline__ void finish4(float* v, const f32x4& acc, const float* bs, int act, bool add, bool has_mask, AD&& addend) {
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = acc[r] + bs[r];
  if (act & 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
  }
  if (add) {
    float a4[4];
    unsigned mb = 0u;
    addend(a4, mb);
    if (has_mask) {
#pragma unroll
      for (int r = 0; r < 4; ++r) a4[r] = ((mb >> r) & 1u) ? a4[r] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += a4[r];
  }
  if (act & 2) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
  }
}

// plain statistics of one 4-channel group
__device__ __forceinline__ void stat_add4(float* s1, float* s2, const float* v) {
#pragma unroll
  for (int r = 0; r < 4; ++r) { s1[r] += v[r]; s2[r] += v[r] * v[r]; }
}
// BatchNorm-backward sums of one 4-channel group: g_y = g*[bn(c) > 0], xhat = (c - mean)*invstd (same operations as bn_bwd_kernel)
__device__ __forceinline__ void bnb_accumulate(const float* g, const float* c, const float4& mu, const float4& sc, const float4& sh, const float4& is,
                                               float* s1, float* s2) {
  const float m[4] = {mu.x, mu.y, mu.z, mu.w}, a[4] = {sc.x, sc.y, sc.z, sc.w}, b[4] = {sh.x, sh.y, sh.z, sh.w}, iv[4] = {is.x, is.y, is.z, is.w};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float d = c[r] - m[r];
    const float bn = __builtin_fmaf(d, a[r], b[r]);
    const float xh = d * iv[r];
    const float gy = bn > 0.f ? g[r] : 0.f;
    s1[r] += gy;
    s2[r] += gy * xh;
  }
}

// fused LogSoftmax over the first Cout (<= 16) channels of a pixel (its four quads hold channels ch = 4q .. 4q+3), fp32 NCHW output.
// Every lane of the wave takes part in the exchanges; only `valid` pixels are stored.
__device__ __forceinline__ void logsoftmax16_store(const float* v, int ch, int Cout, bool valid, float* out, int n, int oy, int ox, int OH, int OW) {
  float m = -3.0e38f;
#pragma unroll
  for (int r = 0; r < 4; ++r) if (ch + r < Cout) m = fmaxf(m, v[r]);
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float e = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) if (ch + r < Cout) e += expf(v[r] - m);
  e += __shfl_xor(e, 16, 64);
  e += __shfl_xor(e, 32, 64);
  const float lse = m + logf(e);
  if (valid) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (ch + r < Cout) out[(((long)n * Cout + ch + r) * OH + oy) * OW + ox] = v[r] - lse;
  }
}

// Statistics flush of a 4-wave workgroup, once at its end (conv_igemm_kernel, conv_thin_kernel): the quad-row sums of each wave's fp32
// partials go to red[wave][channel][s1 | s2]; behind a barrier thread c < TN sums the four waves' rows of channel n0 + c in fp64 and
// adds them into the slot stripe blockIdx.x % nslots of `stats` ([nslots][2][Cout]).  (conv_pc_kernel flushes per consumer wave,
// whenever the wave's cout tile changes: another reduction, kept in that kernel.)
template <int NT>
__device__ __forceinline__ void flush_tile_stats(const float (&s1)[NT][4], const float (&s2)[NT][4], float* red, int wave, int l16, int q, int tid, int n0, int Cout,
                                                 double* stats, int nslots) {
  constexpr int TN = NT * 16;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = wave_quadrow_sum16(s1[j][r]);
      const float b = wave_quadrow_sum16(s2[j][r]);
      if (l16 == 0) {
        red[(wave * TN + j * 16 + 4 * q + r) * 2 + 0] = a;
        red[(wave * TN + j * 16 + 4 * q + r) * 2 + 1] = b;
      }
    }
  __syncthreads();
  if (tid < TN) {
    const int ch = n0 + tid;
    if (ch < Cout) {
      double a = 0.0, b = 0.0;
#pragma unroll
      for (int w = 0; w < 4; ++w) { a += (double)red[(w * TN + tid) * 2]; b += (double)red[(w * TN + tid) * 2 + 1]; }
      double* st = stats + (size_t)(blockIdx.x % nslots) * 2 * Cout;
      atomicAdd(&st[ch], a);
      atomicAdd(&st[Cout + ch], b);
    }
  }
}

// Generic (64-bit address) forms: byte offset of channel ch of pixel (n, oy, ox) in an NHWC view with byte strides, and the
// 4-channel load / store there.  The caller has checked that the group lies inside the view.
template <typename T> __device__ __forceinline__ long nhwc_off(long sn, long sy, long sx, int n, int oy, int ox, int ch) {
  return (long)n * sn + (long)oy * sy + (long)ox * sx + (long)ch * (16 / ET<T>::CPU);
}
// One group on the generic path: the (masked) addend from memory, then the value rule.  inside = pixel valid and ch < Cout.
template <typename T, typename K>
__device__ __forceinline__ void generic_finish4(float* v, const f32x4& acc, const float* bs, const K& k, const char* adb, const uint8_t* mask,
                                                int n, int oy, int ox, int ch, bool inside) {
  constexpr int CPU = ET<T>::CPU;
  finish4(v, acc, bs, k.act, adb != nullptr && inside, mask != nullptr, [&](float* a4, unsigned& mb) {
    load4<T>(adb + nhwc_off<T>(k.a_sn, k.a_sy, k.a_sx, n, oy, ox, ch), a4);
    if (mask != nullptr) mb = (unsigned)mask[(((long)n * k.OH + oy) * k.OW + ox) * k.ad_mask_cu + ch / CPU] >> (ch % CPU);
  });
}

// Buffer-addressed ("fast") epilogue of one tile, for plain NHWC output whose per-image extents fit 31-bit offsets: a store's address
// is one per-lane offset computed once plus a SCALAR fragment offset; lanes outside the output (ragged tiles, padded channels) get an
// out-of-range offset, which drops the store / returns a zero addend; all addend and mask loads are issued before the first value is
// finished.  Built once per tile; the caller walks (i, j) in its own order: addend(i, j), finish4, store(i, j).
template <typename T, int FW, int NT, int TWF>
struct FastEpi {
  static constexpr int CPU = ET<T>::CPU, ESZ = 16 / CPU, kOut = (int)0x80000000;
  __amdgpu_buffer_rsrc_t yr, ar, mr;
  int lane_y, lane_a, lane_m;
  int so_y[FW], so_a[FW], so_m[FW];   // per fragment: scalar offsets
  bool okp[FW];                       // pixel inside the output (ragged tiles only)
  bool okc[NT];                       // channel group inside Cout
  bool has_ad, has_mask;
  int mshift;
  ubr_u4 adv[FW][NT];                 // raw addend: 8 bytes (16-bit types) or 16
  unsigned admk[FW][NT];

  // yb / adb: output and addend base of this launch phase (adb may be null); mask: the addend's ReLU bit mask or null
  template <typename K>
  __device__ __forceinline__ void init(const K& k, char* yb, const char* adb, const uint8_t* mask, int n, int oy0, int ox0, int n0, int wave, int l16, int q) {
    constexpr int TN = NT * 16, TH = 4 * FW / TWF, TW = TWF * 16;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const bool full = (ox0 + TW <= k.OW) && (oy0 + TH <= k.OH) && (n0 + TN <= k.Cout);
    const int ysx = (int)k.y_sx, ysy = (int)k.y_sy, asx = (int)k.a_sx, asy = (int)k.a_sy;
    yr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(yb + (long)n * k.y_sn + (long)oy0 * k.y_sy + (long)ox0 * k.y_sx + (long)n0 * ESZ), 0, 0x7fffffff, 0x00020000);
    has_ad = adb != nullptr; has_mask = has_ad && mask != nullptr;
    ar = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(has_ad ? adb + (long)n * k.a_sn + (long)oy0 * k.a_sy + (long)ox0 * k.a_sx + (long)n0 * ESZ : k.x), 0, has_ad ? 0x7fffffff : 0, 0x00020000);
    mr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(has_mask ? (const char*)mask + (((long)n * k.OH + oy0) * k.OW + ox0) * k.ad_mask_cu + n0 / CPU : k.x), 0, has_mask ? 0x7fffffff : 0, 0x00020000);
    lane_y = l16 * ysx + 4 * q * ESZ; lane_a = l16 * asx + 4 * q * ESZ; lane_m = l16 * k.ad_mask_cu + (4 * q) / CPU;
    mshift = (4 * q) % CPU;
#pragma unroll
    for (int i = 0; i < FW; ++i) {
      const int f = wv * FW + i, fr = f / TWF, fc = f % TWF;
      so_y[i] = fr * ysy + fc * 16 * ysx; so_a[i] = fr * asy + fc * 16 * asx; so_m[i] = (fr * k.OW + fc * 16) * k.ad_mask_cu;
      okp[i] = full || ((oy0 + fr < k.OH) && (ox0 + fc * 16 + l16 < k.OW));
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) okc[j] = full || (n0 + j * 16 + 4 * q < k.Cout);
  }
  __device__ __forceinline__ bool inside(int i, int j) const { return okp[i] && okc[j]; }
  __device__ __forceinline__ void prefetch_addend() {
    if (!has_ad) return;
    // Every lane offset, of the addend and of the mask, is formed BEFORE the first load is issued, and nothing is scheduled across
    // that line: a vector instruction that writes a register a load in flight still owns makes the compiler drain the loads first
    // (an s_waitcnt vmcnt in the middle of the cluster, i.e. one exposed round trip per tile).
    int vo_a[FW][NT], vo_m[FW][NT];
#pragma unroll
    for (int i = 0; i < FW; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        vo_a[i][j] = inside(i, j) ? lane_a : kOut;
        vo_m[i][j] = (has_mask && inside(i, j)) ? lane_m : kOut;
        asm volatile("" : "+v"(vo_a[i][j]), "+v"(vo_m[i][j]));        // (pinned here: otherwise the mask offsets sink into the has_mask branch, behind the addend loads)
      }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < FW; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if constexpr (sizeof(T) == 2) {
          const auto t2 = __builtin_amdgcn_raw_buffer_load_b64(ar, vo_a[i][j], so_a[i] + j * 16 * ESZ, 0);
          adv[i][j] = ubr_u4{t2[0], t2[1], 0u, 0u};
        } else {
          adv[i][j] = __builtin_amdgcn_raw_buffer_load_b128(ar, vo_a[i][j], so_a[i] + j * 16 * ESZ, 0);
        }
      }
    if (has_mask) {
#pragma unroll
      for (int i = 0; i < FW; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) admk[i][j] = __builtin_amdgcn_raw_buffer_load_b8(mr, vo_m[i][j], so_m[i] + j * (16 / CPU), 0);
    }
  }
  // the prefetched addend of group (i, j) as floats (only read when has_ad)
  __device__ __forceinline__ void addend(int i, int j, float* a4) const {
    if constexpr (sizeof(T) == 2) {
      const uint2 raw = make_uint2(adv[i][j][0], adv[i][j][1]);
      load4<T>(reinterpret_cast<const char*>(&raw), a4);
    } else {
      a4[0] = __uint_as_float(adv[i][j][0]); a4[1] = __uint_as_float(adv[i][j][1]); a4[2] = __uint_as_float(adv[i][j][2]); a4[3] = __uint_as_float(adv[i][j][3]);
    }
  }
  // the ReLU bits of group (i, j), bit r for channel r (only read when has_mask)
  __device__ __forceinline__ unsigned mask_bits(int i, int j) const { return (admk[i][j] & 0xffu) >> mshift; }
  __device__ __forceinline__ void store(int i, int j, const float* v) const {
    const int vo = inside(i, j) ? lane_y : kOut;
    if constexpr (sizeof(T) == 2) {
      uint2 pk;
      store4<T>(reinterpret_cast<char*>(&pk), v);
      __builtin_amdgcn_raw_buffer_store_b64(ubr_u2{pk.x, pk.y}, yr, vo, so_y[i] + j * 16 * ESZ, 0);
    } else {
      buf_store16(ubr_u4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])}, yr, vo, so_y[i] + j * 16 * ESZ);
    }
  }
};

}  // namespace
