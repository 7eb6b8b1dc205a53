// The launch plans of libubresnet_calib.so (ubresnet_amd/csrc/ubr_calib_plan.h, plain C++ for a host compiler) as a stand-alone
// program, so that tests/test_cpu_calib.py can run it under the host sanitizers:
//   calib_host N H W K [N H W K ...]
// For every call given, and for a sweep of small ones, it checks the plan, walks the first launch on the host into buffers of
// exactly the planned sizes (every pixel of every image must be met exactly once, every row written whole), adds the rows in the
// finish's order and holds the table and the counters against brute force.  It prints one line per call given,
// `A N H W K hw trips gx rows row_words scratch_bytes`, then `G block unroll lane_pixels trip_pixels max_rows max_temps finish_sub
// finish_words apply_max_grid`, and exits 1 at the first disagreement.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ubr_calib_plan.h"

static int fail(const char* what, int64_t N, int64_t H, int64_t W, int64_t K) {
  std::fprintf(stderr, "calib_host: %s (N %lld, H %lld, W %lld, K %lld)\n", what, (long long)N, (long long)H, (long long)W, (long long)K);
  return 1;
}

static int check_call(int64_t N, int64_t H, int64_t W, int64_t K, bool print) {
  ubf::Plan p;
  if (!ubf::make_plan(N, H, W, K, &p)) return fail("make_plan refused", N, H, W, K);
  if (p.hw != H * W || p.trips < 1 || (p.trips - 1) * ubf::TRIP_PIXELS >= p.hw || p.trips * ubf::TRIP_PIXELS < p.hw)
    return fail("trips do not tile the image", N, H, W, K);
  if (p.gx < 1 || p.gx > p.trips || p.rows != N * p.gx || (p.rows > ubf::MAX_ROWS && p.gx != 1) || p.row_words != 3 * K + 3 ||
      p.row_words > ubf::FINISH_WORDS || p.scratch_bytes != 8 * p.rows * p.row_words)
    return fail("grid or scratch layout", N, H, W, K);
  if (print)
    std::printf("A %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)N, (long long)H, (long long)W, (long long)K, (long long)p.hw,
                (long long)p.trips, (long long)p.gx, (long long)p.rows, (long long)p.row_words, (long long)p.scratch_bytes);
  // exactly N * hw pixels and exactly scratch_bytes of rows: a step outside either is the sanitizer's to report
  std::vector<uint8_t> seen((size_t)(N * p.hw), 0);
  std::vector<uint64_t> rows((size_t)(p.scratch_bytes / 8), 0xDEADBEEFDEADBEEFull);
  ubf::host_walk(p, N, K, seen.data(), rows.data());
  for (uint8_t s : seen)
    if (s != 1) return fail("a pixel is not met exactly once", N, H, W, K);
  for (uint64_t w : rows)
    if (w == 0xDEADBEEFDEADBEEFull) return fail("a word of a row is not written", N, H, W, K);
  // the finish: three groups, image n in group n % 4 (group 3 is not below G: left out)
  const int64_t G = 3;
  std::vector<uint8_t> group((size_t)N);
  for (int64_t n = 0; n < N; ++n) group[(size_t)n] = (uint8_t)(n % 4);
  std::vector<double> table((size_t)(G * K * 3), 0.0);
  std::vector<uint64_t> counters((size_t)(G * 3), 0);
  ubf::host_finish(p, N, K, G, group.data(), rows.data(), table.data(), counters.data());
  for (int64_t g = 0; g < G; ++g) {
    uint64_t images = 0;
    for (int64_t n = 0; n < N; ++n) images += (n % 4 == g);
    const uint64_t want = images * (uint64_t)p.hw;
    if (counters[(size_t)(g * 3)] != want || counters[(size_t)(g * 3 + 1)] != 0 || counters[(size_t)(g * 3 + 2)] != 0)
      return fail("the counters of a group", N, H, W, K);
    for (int64_t k = 0; k < K; ++k)
      if (table[(size_t)((g * K + k) * 3)] != (double)want || table[(size_t)((g * K + k) * 3 + 1)] != 0.0)      // integers: exact in any order
        return fail("the table of a group", N, H, W, K);
  }
  return 0;
}

static int check_apply(int64_t n, int64_t th, int64_t tw) {
  for (int v = 0; v < 2; ++v) {
    ubf::ApplyPlan a;
    const bool vec = v == 1;
    if (vec && (th * tw) % ubf::LANE_PIXELS) {
      if (ubf::make_apply_plan(n, th, tw, true, &a)) return fail("the vector path took a tile that is no multiple of four", n, th, tw, 0);
      continue;
    }
    if (!ubf::make_apply_plan(n, th, tw, vec, &a)) return fail("make_apply_plan refused", n, th, tw, 0);
    const int64_t pixels = n * th * tw;
    if (a.units * (vec ? ubf::LANE_PIXELS : 1) != pixels || a.trips < 1 || (a.trips - 1) * ubf::TRIP_UNITS >= a.units ||
        a.trips * ubf::TRIP_UNITS < a.units || a.grid < 1 || a.grid > a.trips || a.grid > ubf::APPLY_MAX_GRID)
      return fail("the apply plan", n, th, tw, 0);
    // the walk: every unit exactly once, no unit of a vector path straddles two tiles
    std::vector<uint8_t> seen((size_t)a.units, 0);
    for (int64_t g = 0; g < a.grid; ++g)
      for (int64_t t = g; t < a.trips; t += a.grid)
        for (int u = 0; u < ubf::UNROLL; ++u)
          for (int lane = 0; lane < ubf::BLOCK; ++lane) {
            const int64_t i = t * ubf::TRIP_UNITS + (int64_t)u * ubf::BLOCK + lane;
            if (i >= a.units) continue;
            seen[(size_t)i] += 1;
            const int64_t p0 = i * (vec ? ubf::LANE_PIXELS : 1), p1 = p0 + (vec ? ubf::LANE_PIXELS : 1) - 1;
            if (p0 / (th * tw) != p1 / (th * tw)) return fail("a unit straddles two tiles", n, th, tw, 0);
          }
    for (uint8_t s : seen)
      if (s != 1) return fail("an apply unit is not met exactly once", n, th, tw, 0);
  }
  return 0;
}

int main(int argc, char** argv) {
  if ((argc - 1) % 4) {
    std::fprintf(stderr, "usage: calib_host [N H W K]...\n");
    return 2;
  }
  for (int a = 1; a + 3 < argc; a += 4)
    if (check_call(std::atoll(argv[a]), std::atoll(argv[a + 1]), std::atoll(argv[a + 2]), std::atoll(argv[a + 3]), true)) return 1;
  for (int64_t hw = 1; hw <= 3 * ubf::TRIP_PIXELS + 1; hw += (hw < 16 ? 1 : 509))
    for (int64_t N : {1, 2, 5})
      for (int64_t K : {1, 33, 64})
        if (check_call(N, 1, hw, K, false)) return 1;
  if (check_call(ubf::MAX_ROWS + 52, 1, ubf::TRIP_PIXELS + 1, 2, false)) return 1;     // more images than MAX_ROWS: one workgroup per image, two trips
  for (int64_t n : {1, 3})
    for (int64_t th : {1, 7, 32})
      for (int64_t tw : {1, 9, 12, 833})
        if (check_apply(n, th, tw)) return 1;
  if (check_apply(10, 512, 832)) return 1;
  // what the plans refuse
  ubf::Plan p;
  ubf::ApplyPlan ap;
  if (ubf::make_plan(0, 4, 4, 1, &p) || ubf::make_plan(65536, 4, 4, 1, &p) || ubf::make_plan(1, 0, 4, 1, &p) || ubf::make_plan(1, 4, -1, 1, &p) ||
      ubf::make_plan(1, 4, 4, 0, &p) || ubf::make_plan(1, 4, 4, 65, &p) || ubf::make_plan(2, 1 << 20, 1 << 20, 1, &p) ||
      !ubf::make_plan(1, 1 << 20, 1 << 20, 64, &p) || ubf::make_apply_plan(0, 1, 1, false, &ap) || ubf::make_apply_plan(1, 1, 0, false, &ap) ||
      ubf::make_apply_plan(2, 1 << 20, 1 << 20, false, &ap) || !ubf::make_plan(3, 1008, 3456, 33, &p))
    return fail("what the plans refuse", 0, 0, 0, 0);
  if (p.trips != 1701 || p.gx != 256 || p.rows != 768 || p.row_words != 102 || p.scratch_bytes != 8 * 768 * 102)
    return fail("the plan of the full event", 3, 1008, 3456, 33);
  std::printf("G %d %d %d %d %d %d %d %d %d\n", ubf::BLOCK, ubf::UNROLL, ubf::LANE_PIXELS, ubf::TRIP_PIXELS, ubf::MAX_ROWS, ubf::MAX_TEMPS,
              ubf::FINISH_SUB, ubf::FINISH_WORDS, ubf::APPLY_MAX_GRID);
  return 0;
}
