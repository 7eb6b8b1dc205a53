// The launch plan and the limits of libubresnet_moment.so (ubresnet_amd/csrc/ubr_moment_plan.h, plain C++ for a host compiler) as
// a stand-alone program, so that tests/test_cpu_moment.py can run it under the host sanitizers:
//   moment_host P rows cols capacity C [P rows cols capacity C ...]
// For every image given, and for every image of 1 x 1 x n pixels with n from 1 to a few trips, it checks that the plan's walk is
// ubr_walk_plan.h's (that the walk tiles the pixels, and the scales it accepts, are tests/walk_host.cpp's to check) and the clear
// grid.  Then it checks what the plan refuses and the overflow bound over every accepted plane shape with power-of-two sides and
// at the largest planes.  It prints one line per image,
// `I P rows cols pixels trips span grid clear_grid`, then `B <worst column over all accepted shapes>`, then `G lanes trip_pixels
// max_grid slots probes flush_above`, and exits 1 at the first disagreement.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "ubr_moment_plan.h"

static int fail(const char* what, int64_t P, int64_t rows, int64_t cols) {
  std::fprintf(stderr, "moment_host: %s (image %lld x %lld x %lld)\n", what, (long long)P, (long long)rows, (long long)cols);
  return 1;
}

static int check_image(int64_t P, int64_t rows, int64_t cols, int64_t capacity, int64_t C, bool print) {
  ubm::Plan p;
  if (!ubm::make_plan(P, rows, cols, capacity, C, &p)) return fail("make_plan refused", P, rows, cols);
  const int64_t n = P * rows * cols;
  const walk::Walk w = walk::make_walk(n);
  if (p.pixels != n || p.trips != w.trips || p.span != w.span || p.grid != w.grid) return fail("the walk is not the walk plan's", P, rows, cols);
  const int64_t words = (capacity < n ? capacity : n) * (ubm::TABLE_FIXED + C);
  if (p.clear_grid < 1 || p.clear_grid > ubm::MAX_GRID || (p.clear_grid < ubm::MAX_GRID && p.clear_grid * ubm::LANES < words))
    return fail("clear grid", P, rows, cols);
  if (print)
    std::printf("I %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)P, (long long)rows, (long long)cols, (long long)p.pixels,
                (long long)p.trips, (long long)p.span, (long long)p.grid, (long long)p.clear_grid);
  return 0;
}

int main(int argc, char** argv) {
  if ((argc - 1) % 5) {
    std::fprintf(stderr, "usage: moment_host [P rows cols capacity C]...\n");
    return 2;
  }
  for (int a = 1; a + 4 < argc; a += 5)
    if (check_image(std::atoll(argv[a]), std::atoll(argv[a + 1]), std::atoll(argv[a + 2]), std::atoll(argv[a + 3]), std::atoll(argv[a + 4]), true))
      return 1;
  for (int64_t n = 1; n <= 3 * ubm::TRIP_PIXELS + 1; n += (n < 70 ? 1 : 127))
    if (check_image(1, 1, n > ubm::MAX_COLS ? ubm::MAX_COLS : n, 1 + n % 7, 1 + n % ubm::MAX_CLASSES, false)) return 1;
  if (check_image(1, 3, ubm::TRIP_PIXELS + 1, 5, 4, false) || check_image(3, 1008, 3456, 65536, 4, false) ||
      check_image(1, 1024, 4096, 1, 16, false))
    return 1;
  // what the plan refuses
  ubm::Plan p;
  const char* why;
  if (ubm::make_plan(0, 4, 4, 1, 1, &p) || ubm::make_plan(1, -1, 4, 1, 1, &p) || ubm::make_plan(1, 4, 0, 1, 1, &p) ||
      ubm::make_plan(1, 4097, 4, 1, 1, &p) || ubm::make_plan(1, 4, 4097, 1, 1, &p) || ubm::make_plan(1, 2048, 2049, 1, 1, &p) ||
      ubm::make_plan(1, 4096, 1025, 1, 1, &p) || ubm::make_plan(512, 1024, 4096, 1, 1, &p) || ubm::make_plan(1, 4, 4, 0, 1, &p) ||
      ubm::make_plan(1, 4, 4, 1, 0, &p) || ubm::make_plan(1, 4, 4, 1, 17, &p) || !ubm::make_plan(1, 2048, 2048, 1, 16, &p) ||
      !ubm::make_plan(1, 4096, 1024, 1, 1, &p) || !ubm::make_plan(3, 1008, 3456, 65536, 4, &p))
    return fail("what make_plan refuses", 0, 0, 0);
  if (p.trips != 5103 || p.span != 5 || p.grid != 1021 || p.clear_grid != ubm::MAX_GRID) return fail("the plan of the full event", 3, 1008, 3456);
  if (ubm::valid_image(1 << 20, 1 << 20, 1 << 20, &why) || !ubm::valid_image(3, 1008, 3456, &why) || *why != 0)
    return fail("valid_image", 0, 0, 0);
  // the overflow bound: over every accepted plane of power-of-two sides and the planes next to them
  uint64_t worst = 0;
  for (int64_t rows = 1; rows <= ubm::MAX_ROWS; rows *= 2)
    for (int64_t cols = 1; cols <= ubm::MAX_COLS; cols *= 2)
      for (int64_t dr = -1; dr <= 0; ++dr)
        for (int64_t dc = -1; dc <= 0; ++dc) {
          const int64_t r = rows + dr, c = cols + dc;
          if (r < 1 || c < 1 || !ubm::valid_image(1, r, c, &why)) continue;
          // by brute force on the corner pixel: no pixel has a larger r^2, r c or c^2 than (max - 1)^2
          const uint64_t far = (uint64_t)((r > c ? r : c) - 1);
          if ((uint64_t)(r - 1) * (uint64_t)(r - 1) > far * far || (uint64_t)(c - 1) * (uint64_t)(c - 1) > far * far ||
              (uint64_t)(r - 1) * (uint64_t)(c - 1) > far * far)
            return fail("worst_column is no bound", 1, r, c);
          const uint64_t b = ubm::worst_column(r, c);
          if (b / (uint64_t)ubm::MAX_WEIGHT / (uint64_t)(r * c) != far * far) return fail("worst_column wrapped", 1, r, c);
          if (b > worst) worst = b;
        }
  if (worst != ubm::worst_column(1024, 4096) || worst != ubm::worst_column(4096, 1024) || worst >= ((uint64_t)1 << 62))
    return fail("the largest accepted plane is not the worst, or the bound is not below 2^62", 1, 1024, 4096);
  std::printf("B %llu\n", (unsigned long long)worst);
  std::printf("G %d %d %d %d %d %d\n", ubm::LANES, ubm::TRIP_PIXELS, ubm::MAX_GRID, ubm::SLOTS, ubm::PROBES, ubm::FLUSH_ABOVE);
  return 0;
}
