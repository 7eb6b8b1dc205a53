// The rule of libubresnet_crop.so (ubresnet_amd/csrc/ubr_crop_rule.h, and ubx::philox of ubr_det_rule.h through it) as a
// stand-alone program for a host compiler, so that tests/test_cpu_crops.py can run it under the host sanitizers:
//   crop_host words k0 k1 c0 c1 c2                        -> `W w0 w1 w2 w3`, the Philox words with UBN_PHILOX_TAG as c3
//   crop_host cell rows cols H W                          -> `C g`, the largest legal cell or 0
//   crop_host labels offset mask bits...                  -> per fp32 bit pattern `L label counts`
//   crop_host ints offset mask values...                  -> per int64 `L label counts`
//   crop_host valid stacked P rows cols H W plane row0 col0 fr fc   -> `V 0|1`
//   crop_host choose FILE Q rows cols H W g K T min_lit seed_lo seed_hi number flip_rows flip_cols [planes...]
//        FILE holds the Q * (CR + 1) * (CC + 1) int32 of the table as text; -> K lines `T plane row0 col0 lit try accepted fr fc`
// The table lives in a vector of exactly its size: a read outside it is the sanitizer's to report.  Exit 2 on bad usage, 1 where
// the geometry is refused.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ubr_crop_rule.h"

static long long num(const char* s) { return std::strtoll(s, nullptr, 0); }
static unsigned long long unum(const char* s) { return std::strtoull(s, nullptr, 0); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "words" && argc == 7) {
    const ubx::Words w = ubx::philox((uint32_t)unum(argv[2]), (uint32_t)unum(argv[3]), (uint32_t)unum(argv[4]), (uint32_t)unum(argv[5]),
                                     (uint32_t)unum(argv[6]), UBN_PHILOX_TAG);
    std::printf("W %u %u %u %u\n", w.w[0], w.w[1], w.w[2], w.w[3]);
    return 0;
  }
  if (mode == "cell" && argc == 6) {
    std::printf("C %d\n", ubn::largest_cell((int)num(argv[2]), (int)num(argv[3]), (int)num(argv[4]), (int)num(argv[5])));
    return 0;
  }
  if ((mode == "labels" || mode == "ints") && argc >= 4) {
    const int32_t off = (int32_t)num(argv[2]);
    const uint32_t mask = (uint32_t)unum(argv[3]);
    for (int a = 4; a < argc; ++a) {
      int64_t L;
      if (mode == "labels") {
        L = ubn::label_of_float(ubx::from_bits((uint32_t)unum(argv[a])), off);
      } else {
        L = ubn::label_of_int((int64_t)num(argv[a]), off);
      }
      std::printf("L %" PRId64 " %d\n", L, ubn::label_counts(L, mask) ? 1 : 0);
    }
    return 0;
  }
  if (mode == "valid" && argc == 13) {
    int v[11];
    for (int a = 0; a < 11; ++a) v[a] = (int)num(argv[2 + a]);
    std::printf("V %d\n", ubn::row_is_valid(v[6], v[7], v[8], v[9], v[10], v[0], v[1], v[2], v[3], v[4], v[5]) ? 1 : 0);
    return 0;
  }
  if (mode == "choose" && argc >= 17) {
    const int Q = (int)num(argv[3]), rows = (int)num(argv[4]), cols = (int)num(argv[5]), H = (int)num(argv[6]), W = (int)num(argv[7]);
    const int g = (int)num(argv[8]), K = (int)num(argv[9]), T = (int)num(argv[10]);
    const int32_t min_lit = (int32_t)num(argv[11]);
    const uint32_t seed_lo = (uint32_t)unum(argv[12]), seed_hi = (uint32_t)unum(argv[13]), number = (uint32_t)unum(argv[14]);
    const int fr = (int)num(argv[15]), fc = (int)num(argv[16]);
    std::vector<int32_t> planes;
    for (int a = 17; a < argc; ++a) planes.push_back((int32_t)num(argv[a]));
    ubn::Geometry geo;
    if (!ubn::view_is_legal(Q, rows, cols) ||
        !ubn::make_geometry(Q, rows, cols, H, W, g, planes.empty() ? nullptr : planes.data(), (int)planes.size(), &geo)) {
      std::fprintf(stderr, "crop_host: the geometry is refused\n");
      return 1;
    }
    std::vector<int32_t> sat((size_t)Q * (size_t)(geo.CR + 1) * (size_t)(geo.CC + 1));
    std::FILE* f = std::fopen(argv[2], "r");
    if (!f) return 2;
    for (auto& v : sat) {
      long long x;
      if (std::fscanf(f, "%lld", &x) != 1) {
        std::fclose(f);
        std::fprintf(stderr, "crop_host: the table file is short\n");
        return 2;
      }
      v = (int32_t)x;
    }
    std::fclose(f);
    for (int k = 0; k < K; ++k) {
      const ubn::Row r = ubn::choose(sat.data(), geo, seed_lo, seed_hi, number, (uint32_t)k, T, min_lit, fr, fc);
      std::printf("T %d %d %d %d %d %d %d %d\n", r.f[0], r.f[1], r.f[2], r.f[3], r.f[4], r.f[5], r.f[6], r.f[7]);
    }
    return 0;
  }
  std::fprintf(stderr, "usage: crop_host words|cell|labels|ints|valid|choose ...\n");
  return 2;
}
