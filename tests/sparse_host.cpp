// The launch plan of libubresnet_sparse.so's compaction (ubresnet_amd/csrc/ubr_sparse_plan.h, plain C++ for a host compiler) as a
// stand-alone program, so that tests/test_cpu_sparse.py can run it under the host sanitizers:
//   sparse_host P rows cols [P rows cols ...]
// For every image given, and for every image of 1 x n x 1 pixels with n from 1 to a few pixel blocks, it runs the host
// restatement of the three launches (count, scan, write) over four occupancies and three capacities and holds the result
// against brute force; the plan beneath it is tests/scan_host.cpp's.  It prints one line per image, `I P rows cols pixels
// blocks scan_trips scratch_bytes`, then `G lanes lane_pixels pixel_block scan_width max_grid`, and exits 1 at the first
// disagreement.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ubr_sparse_plan.h"

static int fail(const char* what, int64_t P, int64_t rows, int64_t cols, int occ, int64_t cap) {
  std::fprintf(stderr, "sparse_host: %s (image %lld x %lld x %lld, occupancy %d, capacity %lld)\n", what, (long long)P, (long long)rows,
               (long long)cols, occ, (long long)cap);
  return 1;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int check_image(int64_t P, int64_t rows, int64_t cols, bool print) {
  ubz::Plan p;
  if (!ubz::make_plan(P, rows, cols, &p)) return fail("make_plan refused", P, rows, cols, -1, 0);
  const int64_t n = P * rows * cols;                           // (that the plan tiles n is tests/scan_host.cpp's to check)
  if (print)
    std::printf("I %lld %lld %lld %lld %lld %lld %lld\n", (long long)P, (long long)rows, (long long)cols, (long long)p.pixels,
                (long long)p.blocks, (long long)p.scan_trips, (long long)p.scratch_bytes);
  std::vector<uint8_t> lit((size_t)n);
  // exactly scratch_words words and exactly capacity entries: a step outside either is the sanitizer's to report
  std::vector<uint32_t> scratch((size_t)p.scratch_words);
  uint32_t seed = (uint32_t)(n * 2654435761u) + 17u;
  for (int occ = 0; occ < 4; ++occ) {
    for (int64_t q = 0; q < n; ++q)
      lit[(size_t)q] = occ == 0 ? 0 : occ == 1 ? 1 : occ == 2 ? (uint8_t)((q / ubz::PIXEL_BLOCK) % 2 == 0) : (uint8_t)((lcg(seed) >> 24) < 77);
    std::vector<int32_t> brute;
    for (int64_t q = 0; q < n; ++q)
      if (lit[(size_t)q]) brute.push_back((int32_t)q);
    const int64_t total = (int64_t)brute.size();
    const int64_t caps[3] = {total > 0 ? total : 1, total > 1 ? total - 1 : 1, 1};
    for (int64_t cap : caps) {
      for (auto& w : scratch) w = 0xDEADBEEFu;                 // the pass must write every word it later reads
      ubz::host_count(p, lit.data(), scratch.data());
      uint64_t sum = 0;
      for (int64_t b = 0; b < p.blocks; ++b) sum += scratch[(size_t)b];
      if ((int64_t)sum != total) return fail("the block counts do not sum to the total", P, rows, cols, occ, cap);
      const uint64_t got = ubz::host_scan(p, scratch.data());
      if ((int64_t)got != total) return fail("the scan's total", P, rows, cols, occ, cap);
      uint32_t run = 0;
      for (int64_t b = 0; b < p.blocks; ++b) {
        if (scratch[(size_t)b] != run) return fail("the scan is not the exclusive prefix", P, rows, cols, occ, cap);
        for (int64_t q = b * ubz::PIXEL_BLOCK; q < (b + 1) * ubz::PIXEL_BLOCK && q < n; ++q) run += lit[(size_t)q];
      }
      std::vector<int32_t> out((size_t)cap, -7);
      ubz::host_write(p, lit.data(), scratch.data(), cap, out.data());
      for (int64_t k = 0; k < cap; ++k) {
        const int32_t want = k < total ? brute[(size_t)k] : -7;
        if (out[(size_t)k] != want) return fail("the written list", P, rows, cols, occ, cap);
      }
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if ((argc - 1) % 3) {
    std::fprintf(stderr, "usage: sparse_host [P rows cols]...\n");
    return 2;
  }
  for (int a = 1; a + 2 < argc; a += 3)
    if (check_image(std::atoll(argv[a]), std::atoll(argv[a + 1]), std::atoll(argv[a + 2]), true)) return 1;
  for (int64_t n = 1; n <= 3 * ubz::PIXEL_BLOCK + 1; ++n)
    if (check_image(1, n, 1, false)) return 1;
  // what the plan refuses: no pixel, and 2^31 pixels or more
  ubz::Plan p;
  if (ubz::make_plan(0, 4, 4, &p) || ubz::make_plan(1, -1, 4, &p) || ubz::make_plan(1, 4, 0, &p) || ubz::make_plan(2, 32768, 32768, &p) ||
      ubz::make_plan(1, 1 << 30, 1 << 30, &p) || !ubz::make_plan(1, 2147483647, 1, &p) || !ubz::make_plan(3, 1008, 3456, &p))
    return fail("what make_plan refuses", 0, 0, 0, -1, 0);
  if (p.blocks != 10206 || p.scan_trips != 10 || p.scratch_bytes != 4 * 10208) return fail("the plan of the full event", 3, 1008, 3456, -1, 0);
  if (ubz::stride_grid(0) != 0 || ubz::stride_grid(1) != 1 || ubz::stride_grid(ubz::LANES + 1) != 2 ||
      ubz::stride_grid((int64_t)ubz::MAX_GRID * ubz::LANES + 1) != ubz::MAX_GRID)
    return fail("stride_grid", 0, 0, 0, -1, 0);
  std::printf("G %d %d %d %d %d\n", ubz::LANES, ubz::LANE_PIXELS, ubz::PIXEL_BLOCK, ubz::SCAN_WIDTH, ubz::MAX_GRID);
  return 0;
}
