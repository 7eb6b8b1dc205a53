// The apply pass of ubw_pixel_weights run on the host: the three phases of ubresnet_amd/csrc/ubr_weight_tile.h called lane by
// lane, tile by tile, with ordinary arrays in the place of the LDS.  tests/test_cpu_weights.py compiles this file and compares
// its output with tests/weights_ref.py.  `counts` is an input here (the count pass is not part of the header).
#include <cstdint>
#include <vector>
#include "ubr_weight_tile.h"

using namespace ubw;

template <int R>
static void run_tile(const ApplyK& k, const long long* lab, float* wgt, const long long* row, int x0, int y0) {
  std::vector<unsigned> ids_words((ids_bytes(R) + 3) / 4), rm_words_((rm_words(R) + 1) / 2);
  unsigned char* ids = reinterpret_cast<unsigned char*>(ids_words.data());
  unsigned short* rm = reinterpret_cast<unsigned short*>(rm_words_.data());
  float wc[UBW_MAX_CLASSES];
  unsigned own[BLOCK];
  for (int t = 0; t < UBW_MAX_CLASSES; ++t) wc[t] = class_weight(row, t, k.max_weight);
  for (int t = 0; t < BLOCK; ++t) own[t] = stage<R>(k, lab, x0, y0, t, ids);
  if (R > 0)
    for (int t = 0; t < BLOCK; ++t) row_sets<R>(t, ids, rm);
  for (int t = 0; t < BLOCK; ++t) finish<R>(k, wgt, x0, y0, t, own[t], rm, wc);
}

extern "C" int host_apply(const long long* label, float* weight, const long long* counts, int B, int H, int W, int C,
                          float max_weight, int radius, float gain, int lo, int vector) {
  ApplyK k{};
  k.lab = label; k.wgt = weight; k.counts = counts; k.H = H; k.W = W; k.C = C; k.lo = lo;
  k.tiles_x = (W + TW - 1) / TW;
  k.tiles = k.tiles_x * ((H + TH - 1) / TH);
  k.max_weight = max_weight; k.gain = gain;
  k.vlab = vector && W % 4 == 0 && (uintptr_t)label % 16 == 0;
  k.vwgt = vector && W % 4 == 0 && (uintptr_t)weight % 16 == 0;
  const long n = (long)H * W;
  for (int b = 0; b < B; ++b)
    for (int tile = 0; tile < k.tiles; ++tile) {
      const int y0 = tile / k.tiles_x * TH, x0 = tile % k.tiles_x * TW;
      const long long* lab = label + b * n;
      float* wgt = weight + b * n;
      const long long* row = counts + b * UBW_MAX_CLASSES;
      switch (radius) {
        case 0: run_tile<0>(k, lab, wgt, row, x0, y0); break;
        case 1: run_tile<1>(k, lab, wgt, row, x0, y0); break;
        case 2: run_tile<2>(k, lab, wgt, row, x0, y0); break;
        case 3: run_tile<3>(k, lab, wgt, row, x0, y0); break;
        default: run_tile<4>(k, lab, wgt, row, x0, y0); break;
      }
    }
  return k.vlab + 2 * k.vwgt;
}
