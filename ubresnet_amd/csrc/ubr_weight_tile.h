// The per-lane work of the apply pass of ubw_pixel_weights (include/ubresnet_weight.h), phase by phase.  Plain C++ that a
// host compiler takes as well: the kernel in ubr_weight.hip calls the three phases with a barrier between them, and a host
// program can run them lane by lane over ordinary arrays in the place of the LDS.
#ifndef UBR_WEIGHT_TILE_H
#define UBR_WEIGHT_TILE_H

#include <stdint.h>
#include "../../include/ubresnet_weight.h"

// Launch geometry, not part of the C ABI (tests derive their shapes from it): a workgroup has UBW_BLOCK lanes and a lane takes
// UBW_LANE_PIXELS consecutive pixels.  The count pass runs min(ceil(H*W / (UBW_BLOCK * UBW_LANE_PIXELS)), max(1, UBW_MAX_GRID / B))
// workgroups per image, which stride over the image; the apply pass runs one workgroup per UBW_TILE_H x UBW_TILE_W tile of an
// image (a lane takes UBW_LANE_PIXELS pixels of one tile row).
#define UBW_LANE_PIXELS 4
#define UBW_BLOCK 256
#define UBW_MAX_GRID 2048
#define UBW_TILE_W 64
#define UBW_TILE_H 16

#if defined(__HIPCC__)
#define UBW_HD __host__ __device__ __forceinline__
#else
#define UBW_HD inline
#endif

namespace ubw {

constexpr int TW = UBW_TILE_W, TH = UBW_TILE_H, BLOCK = UBW_BLOCK, LP = UBW_LANE_PIXELS;
constexpr int GX = TW / LP;                 // lanes along a tile row
constexpr int IDS_PAD = 4;                  // columns in front of and behind a tile row of `ids`: the tile starts on a word
constexpr int IDS_STRIDE = TW + 2 * IDS_PAD;
constexpr unsigned NONE = 0xFFu;            // class id of an invalid pixel and of everything outside the image
static_assert(TH * GX == BLOCK && UBW_MAX_RADIUS <= IDS_PAD && IDS_STRIDE % 4 == 0, "tile geometry");

struct alignas(16) LL2 { long long x, y; };
struct alignas(16) F4 { float x, y, z, w; };

struct ApplyK {
  const long long* lab;       // [B][H][W]
  float* wgt;                 // [B][H][W]
  const long long* counts;    // [B][UBW_MAX_CLASSES], complete
  int H, W, C, lo;
  int tiles_x, tiles;         // tiles along a row, tiles of an image
  float max_weight, gain;
  int vlab, vwgt;             // W % 4 == 0 and the region is 16-byte aligned: 16-byte accesses
};

constexpr int ids_bytes(int r) { return r > 0 ? (TH + 2 * r) * IDS_STRIDE : 4; }
constexpr int rm_words(int r) { return r > 0 ? (TH + 2 * r) * TW : 4; }

// decided on the full 64-bit value: a negative label is a huge unsigned one
UBW_HD unsigned class_of(long long v, int C) { return (unsigned long long)v < (unsigned long long)C ? (unsigned)v : NONE; }
// the id a pixel shows to its neighbours: classes below `lo` take no part in an interface
UBW_HD unsigned shown(unsigned id, int lo) { return (id != NONE && id >= (unsigned)lo) ? id : NONE; }

// w_c of include/ubresnet_weight.h from a complete row of counts; 0 for an absent class (no pixel reads it)
UBW_HD float class_weight(const long long* row, int c, float max_weight) {
  const long long n = row[c];
  if (n <= 0) return 0.0f;
  long long V = 0;
  int K = 0;
  for (int i = 0; i < UBW_MAX_CLASSES; ++i) {
    V += row[i];
    K += row[i] > 0;
  }
  double w = (double)V / ((double)K * (double)n);
  const double cap = (double)max_weight;
  if (!(w < cap)) w = cap;
  return (float)w;
}

// Phase 1: lane t classifies its LP pixels of the tile at (x0, y0) of the image `lab` and, with R > 0, writes their shown ids
// into ids[TH + 2R][IDS_STRIDE]; the lanes share the cells of the R-wide halo, NONE where the image ends.  -> the lane's own
// LP class ids, a byte each (NONE beyond the image).
template <int R>
UBW_HD unsigned stage(const ApplyK& k, const long long* lab, int x0, int y0, int t, unsigned char* ids) {
  const int ty = t / GX, tx = (t % GX) * LP;
  const int y = y0 + ty, x = x0 + tx;
  unsigned own = 0xFFFFFFFFu;
  if (y < k.H && x < k.W) {
    const long long* p = lab + (long)y * k.W + x;
    long long v[LP];
    if (k.vlab) {                                            // W % 4 == 0: x + 3 < W
      const LL2 a = reinterpret_cast<const LL2*>(p)[0], b = reinterpret_cast<const LL2*>(p)[1];
      v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
      for (int j = 0; j < LP; ++j) v[j] = x + j < k.W ? p[j] : -1ll;
    }
    own = 0;
    for (int j = 0; j < LP; ++j) own |= class_of(v[j], k.C) << (8 * j);
  }
  if constexpr (R > 0) {
    unsigned sh = 0;
    for (int j = 0; j < LP; ++j) sh |= shown((own >> (8 * j)) & 0xFFu, k.lo) << (8 * j);
    *reinterpret_cast<unsigned*>(ids + (ty + R) * IDS_STRIDE + IDS_PAD + tx) = sh;
    constexpr int HALO_W = TW + 2 * R, NTOP = R * HALO_W, NSIDE = R * TH, TOTAL = 2 * NTOP + 2 * NSIDE;
    for (int i = t; i < TOTAL; i += BLOCK) {
      int ly, lx;                                            // row and column of the cell in `ids`
      if (i < 2 * NTOP) {                                    // the R rows above the tile, then the R rows below it
        const int below = i >= NTOP, j = i - below * NTOP;
        ly = j / HALO_W + (below ? R + TH : 0);
        lx = IDS_PAD - R + j % HALO_W;
      } else {                                               // the R columns left of the tile, then the R columns right of it
        int j = i - 2 * NTOP;
        const int right = j >= NSIDE;
        j -= right * NSIDE;
        ly = R + j / R;
        lx = (right ? IDS_PAD + TW : IDS_PAD - R) + j % R;
      }
      const int yy = y0 + ly - R, xx = x0 + lx - IDS_PAD;
      unsigned u = NONE;
      if (yy >= 0 && yy < k.H && xx >= 0 && xx < k.W) u = shown(class_of(lab[(long)yy * k.W + xx], k.C), k.lo);
      ids[ly * IDS_STRIDE + lx] = (unsigned char)u;
    }
  }
  return own;
}

// Phase 2 (R > 0): rm[ly][x] = the set, one bit per class, of the shown ids in columns x-R .. x+R of row ly of `ids`.  A work
// item is LP pixels of a row: three words of ids (the columns of the group, the four before and the four behind) give the four sets.
template <int R>
UBW_HD void row_sets(int t, const unsigned char* ids, unsigned short* rm) {
  constexpr int ROWS = TH + 2 * R;
  for (int i = t; i < ROWS * GX; i += BLOCK) {
    const int ly = i / GX, gx = (i % GX) * LP;
    const unsigned* w = reinterpret_cast<const unsigned*>(ids + ly * IDS_STRIDE + gx);
    // whole words: the bytes of columns 0..3-R and 68+R..71 of a row are never written by phase 1 and are uninitialised on
    // purpose; only columns 4-R..7+R of the twelve are used below
    const unsigned w3[3] = {w[0], w[1], w[2]};
    unsigned m[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 4 - R; c <= 7 + R; ++c) {
      const unsigned id = (w3[c >> 2] >> (8 * (c & 3))) & 0xFFu;
      m[c] = (1u << (id & 31u)) & 0xFFFFu;                   // NONE -> bit 31 -> the empty set
    }
    unsigned o[LP];
    for (int p = 0; p < LP; ++p) {
      o[p] = 0;
      for (int c = 4 + p - R; c <= 4 + p + R; ++c) o[p] |= m[c];
    }
    unsigned* q = reinterpret_cast<unsigned*>(rm + ly * TW + gx);
    q[0] = o[0] | (o[1] << 16);
    q[1] = o[2] | (o[3] << 16);
  }
}

// Phase 3: the lane's LP weights.  The set of a pixel's window is the union of 2R+1 row sets; it is an interface pixel if it
// takes part itself and the set holds another class.
template <int R>
UBW_HD void finish(const ApplyK& k, float* wgt, int x0, int y0, int t, unsigned own, const unsigned short* rm, const float* wc) {
  const int ty = t / GX, tx = (t % GX) * LP;
  const int y = y0 + ty, x = x0 + tx;
  if (y >= k.H || x >= k.W) return;
  unsigned a = 0, b = 0;
  if constexpr (R > 0) {
    for (int dy = 0; dy <= 2 * R; ++dy) {
      const unsigned* q = reinterpret_cast<const unsigned*>(rm + (ty + dy) * TW + tx);
      a |= q[0];
      b |= q[1];
    }
  }
  const unsigned set[LP] = {a & 0xFFFFu, a >> 16, b & 0xFFFFu, b >> 16};
  float o[LP];
  for (int j = 0; j < LP; ++j) {
    const unsigned id = (own >> (8 * j)) & 0xFFu;
    float w = wc[id & (UBW_MAX_CLASSES - 1)];
    if (R > 0 && id >= (unsigned)k.lo && (set[j] & ~(1u << (id & 31u))) != 0) w = w * k.gain;
    o[j] = id == NONE ? 0.0f : w;
  }
  float* p = wgt + (long)y * k.W + x;
  if (k.vwgt) {
    F4 f;
    f.x = o[0]; f.y = o[1]; f.z = o[2]; f.w = o[3];
    *reinterpret_cast<F4*>(p) = f;
  } else {
    for (int j = 0; j < LP; ++j)
      if (x + j < k.W) p[j] = o[j];
  }
}

}  // namespace ubw

#endif
