// The rule of libubresnet_crop.so (include/ubresnet_crop.h states it) as inline functions that a host compiler takes as well:
// the kernels in extra/ubr_crop.hip call them on the device, tests/crop_host.cpp compiles them into a stand-alone program with
// the host sanitizers on.  Integers only, apart from the two compares of the lit test and of the float label rule.  Philox is
// ubx::philox of ubr_det_rule.h, included and not restated; the draws of this library carry UBN_PHILOX_TAG in its fourth
// counter word, those of the detector library UBX_PHILOX_TAG.
#ifndef UBR_CROP_RULE_H
#define UBR_CROP_RULE_H

#include <stdint.h>
#include "../../include/ubresnet_crop.h"
#include "ubr_det_rule.h"

namespace ubn {

const int64_t MAX_PIXELS = 2147483647;      // P * rows * cols at most
const int64_t NO_LABEL = INT64_MIN;         // the converted label of a float that is no integer below 2^31 in magnitude

// everything ubn_choose needs to know about the view, the crop and the planes a crop may come from
struct Geometry {
  int Q, CR, CC, NR, NC;    // count planes, cells of the view, crop positions
  int hc, wc, g;            // cells of a crop, pixels of a cell
  int nplanes;
  uint8_t plane[UBN_MAX_PLANES];
};

UBX_HD bool cell_is_legal(int g) { return g >= UBN_MIN_CELL && g <= UBN_MAX_CELL && (g & (g - 1)) == 0; }

// the view is one the library takes at all: positive, P <= UBN_MAX_PLANES, below 2^31 pixels
UBX_HD bool view_is_legal(int P, int rows, int cols) {
  return P >= 1 && P <= UBN_MAX_PLANES && rows >= 1 && cols >= 1 && (int64_t)P * rows * cols <= MAX_PIXELS;
}

// g divides H, W, rows - H and cols - W, and the crop fits
UBX_HD bool cell_fits(int g, int rows, int cols, int H, int W) {
  return cell_is_legal(g) && H >= 1 && W >= 1 && H <= rows && W <= cols && H % g == 0 && W % g == 0 && (rows - H) % g == 0 &&
         (cols - W) % g == 0;
}

// the largest legal cell for a view and a crop; 0 where there is none (ubresnet_amd/crops.py makes the same choice)
UBX_HD int largest_cell(int rows, int cols, int H, int W) {
  for (int g = UBN_MAX_CELL; g >= UBN_MIN_CELL; g >>= 1)
    if (cell_fits(g, rows, cols, H, W)) return g;
  return 0;
}

// planes == nullptr: all Q in order.  False where the cell does not fit or the list is not nplanes distinct planes below Q.
UBX_HD bool make_geometry(int Q, int rows, int cols, int H, int W, int g, const int32_t* planes, int nplanes, Geometry* out) {
  if (Q < 1 || Q > UBN_MAX_PLANES || !cell_fits(g, rows, cols, H, W)) return false;
  out->Q = Q;
  out->g = g;
  out->CR = rows / g;
  out->CC = cols / g;
  out->NR = (rows - H) / g + 1;
  out->NC = (cols - W) / g + 1;
  out->hc = H / g;
  out->wc = W / g;
  if (!planes) nplanes = Q;
  if (nplanes < 1 || nplanes > Q) return false;
  out->nplanes = nplanes;
  for (int a = 0; a < UBN_MAX_PLANES; ++a) out->plane[a] = 0;
  for (int a = 0; a < nplanes; ++a) {
    const int32_t p = planes ? planes[a] : a;
    if (p < 0 || p >= Q) return false;
    for (int b = 0; b < a; ++b)
      if (out->plane[b] == p) return false;
    out->plane[a] = (uint8_t)p;
  }
  return true;
}

// ---- the predicate's parts ---------------------------------------------------------------------------------------------------
UBX_HD bool lit(float x, float thr) { return x > thr; }                      // strict; NaN is not lit

UBX_HD int64_t label_of_int(int64_t v, int32_t off) { return (int64_t)((uint64_t)v + (uint64_t)(int64_t)off); }
UBX_HD int64_t label_of_float(float v, int32_t off) {                        // ubd_prep_batch's rule; NaN fails the compare
  return fabsf(v) < 2147483648.0f ? (int64_t)(int32_t)v + (int64_t)off : NO_LABEL;
}
UBX_HD bool label_counts(int64_t L, uint32_t class_mask) { return L >= 0 && L < 32 && ((class_mask >> (int)L) & 1u) != 0u; }

// ---- the selection -------------------------------------------------------------------------------------------------------------
// counting pixels of the hc x wc cells at cell (i, j) of count plane `plane`
UBX_HD int32_t window(const int32_t* sat, const Geometry& geo, int plane, int i, int j) {
  const int32_t* s = sat + (int64_t)plane * (geo.CR + 1) * (geo.CC + 1);
  const int w = geo.CC + 1;
  return s[(int64_t)(i + geo.hc) * w + j + geo.wc] - s[(int64_t)i * w + j + geo.wc] - s[(int64_t)(i + geo.hc) * w + j] +
         s[(int64_t)i * w + j];
}

struct Row {
  int32_t f[UBN_TABLE_FIELDS];    // plane, row0, col0, lit, try, accepted, flip_rows, flip_cols
};

// row k of the table.  `sat` is dereferenced here: device memory in the kernel, host memory in tests/crop_host.cpp.
UBX_HD Row choose(const int32_t* sat, const Geometry& geo, uint32_t seed_lo, uint32_t seed_hi, uint32_t number, uint32_t k, int T,
                  int32_t min_lit, int flip_rows, int flip_cols) {
  Row best = {{0, 0, 0, 0, 0, 0, 0, 0}};
  int32_t best_n = -1;
  int accepted = 0;
  for (int t = 0; t < T && !accepted; ++t) {
    const ubx::Words w = ubx::philox(seed_lo, seed_hi, number, k, (uint32_t)t, UBN_PHILOX_TAG);
    const int plane = geo.plane[w.w[0] % (uint32_t)geo.nplanes];
    const int i = (int)(w.w[1] % (uint32_t)geo.NR), j = (int)(w.w[2] % (uint32_t)geo.NC);
    const int32_t n = window(sat, geo, plane, i, j);
    accepted = n >= min_lit;
    if (accepted || n > best_n) {                                 // strictly more: the earliest try wins a tie
      best_n = n;
      best.f[0] = plane;
      best.f[1] = i * geo.g;
      best.f[2] = j * geo.g;
      best.f[3] = n;
      best.f[4] = t;
      best.f[6] = (int32_t)(w.w[3] & 1u) & (flip_rows ? 1 : 0);
      best.f[7] = (int32_t)((w.w[3] >> 1) & 1u) & (flip_cols ? 1 : 0);
    }
  }
  best.f[5] = accepted;
  return best;
}

// ---- the gather's row check ----------------------------------------------------------------------------------------------------
// the fields of a table row that ubn_gather reads name a crop inside the view
UBX_HD bool row_is_valid(int32_t plane, int32_t row0, int32_t col0, int32_t fr, int32_t fc, int stacked, int P, int rows, int cols, int H,
                         int W) {
  return plane >= 0 && plane < (stacked ? 1 : P) && row0 >= 0 && row0 <= rows - H && col0 >= 0 && col0 <= cols - W && (fr == 0 || fr == 1) &&
         (fc == 0 || fc == 1);
}

}  // namespace ubn

#endif
