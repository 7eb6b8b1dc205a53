// The launch plan of libubresnet_cluster.so (ubresnet_amd/csrc/ubr_cluster_plan.h, plain C++ for a host compiler) as a
// stand-alone program, so that tests/test_cpu_cluster.py can run it under the host sanitizers:
//   cluster_host P rows cols [P rows cols ...]
// For every image given, and for every image of 1 x n x 1 pixels with n from 1 to a few pixel blocks, it checks the tiles of
// the plan (its pixel blocks and scratch layout are tests/scan_host.cpp's), then runs the host restatement of count / scan /
// number over four root maps and holds the numbering against brute force.  Then it runs the model of the kernels' union loop: random unions on random forests, with and without an
// adversary that links roots between any two memory operations of the loop, and checks that every loop ends within its bound
// and that the forest has exactly the components of the union graph, each rooted at its smallest member.  It prints one line per
// image, `I P rows cols pixels tiles_y tiles_x tiles blocks scan_trips scratch_bytes`, then `G tile_h tile_w lanes border_lanes
// pixel_block scan_width max_grid`, and exits 1 at the first disagreement.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ubr_cluster_plan.h"

static int fail(const char* what, int64_t P, int64_t rows, int64_t cols, int variant) {
  std::fprintf(stderr, "cluster_host: %s (image %lld x %lld x %lld, variant %d)\n", what, (long long)P, (long long)rows, (long long)cols,
               variant);
  return 1;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int check_image(int64_t P, int64_t rows, int64_t cols, bool print) {
  ubi::Plan p;
  if (!ubi::make_plan(P, rows, cols, &p)) return fail("make_plan refused", P, rows, cols, -1);
  const int64_t n = P * rows * cols;
  if ((p.tiles_y - 1) * ubi::TILE_H >= rows || p.tiles_y * ubi::TILE_H < rows || (p.tiles_x - 1) * ubi::TILE_W >= cols ||
      p.tiles_x * ubi::TILE_W < cols || p.tiles != P * p.tiles_y * p.tiles_x || p.tiles > n || p.tiles > ubi::MAX_PIXELS)
    return fail("tiles do not tile the planes", P, rows, cols, -1);
  if (print)
    std::printf("I %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)P, (long long)rows, (long long)cols, (long long)p.pixels,
                (long long)p.tiles_y, (long long)p.tiles_x, (long long)p.tiles, (long long)p.blocks, (long long)p.scan_trips,
                (long long)p.scratch_bytes);
  // every pixel lies in exactly one lane slot of one block
  if (ubi::lane_pixel(0, 0, 0) != 0 || ubi::lane_pixel(p.blocks - 1, ubi::LANES - 1, ubi::LANE_PIXELS - 1) != p.blocks * ubi::PIXEL_BLOCK - 1)
    return fail("lane_pixel", P, rows, cols, -1);
  std::vector<int32_t> root((size_t)n), ids((size_t)n);
  std::vector<uint32_t> scratch((size_t)p.scratch_words);        // exactly the planned words: a step outside is the sanitizer's
  uint32_t seed = (uint32_t)(n * 2654435761u) + 29u;
  for (int variant = 0; variant < 4; ++variant) {
    // a root map: -1 (not lit), q (a root) or the last root before q; variant 0 none lit, 1 every pixel a root, 2 one root, 3 random
    int32_t last = -1;
    for (int64_t q = 0; q < n; ++q) {
      const uint32_t r = lcg(seed) >> 24;
      int32_t v;
      if (variant == 0) v = -1;
      else if (variant == 1) v = (int32_t)q;
      else if (variant == 2) v = 0;
      else v = r < 60 ? -1 : (r < 120 || last < 0) ? (int32_t)q : last;
      if (v == (int32_t)q) last = v;
      root[(size_t)q] = v;
    }
    for (auto& w : scratch) w = 0xDEADBEEFu;                     // the pass must write every word it later reads
    for (auto& w : ids) w = -7;
    ubi::host_count(p, root.data(), scratch.data());
    const uint64_t total = ubi::host_scan(p, scratch.data());
    ubi::host_number(p, root.data(), scratch.data(), ids.data());
    int64_t k = 0;
    for (int64_t q = 0; q < n; ++q) {
      const int32_t want = root[(size_t)q] < 0 ? -1 : root[(size_t)q] == (int32_t)q ? (int32_t)k++ : -7;
      if (ids[(size_t)q] != want) return fail("the numbering is not the ascending root order", P, rows, cols, variant);
    }
    if ((int64_t)total != k) return fail("the scan's total", P, rows, cols, variant);
  }
  return 0;
}

// ---- the union loop ----
struct Brute {                                                    // components by relabelling: O(n) per union, beyond doubt
  std::vector<int32_t> comp;
  explicit Brute(int32_t n) : comp((size_t)n) {
    for (int32_t i = 0; i < n; ++i) comp[(size_t)i] = i;
  }
  void join(int32_t a, int32_t b) {
    const int32_t ca = comp[(size_t)a], cb = comp[(size_t)b];
    if (ca == cb) return;
    const int32_t lo = ca < cb ? ca : cb, hi = ca < cb ? cb : ca;
    for (auto& c : comp)
      if (c == hi) c = lo;
  }
};

static int check_unions(int32_t n, int unions, uint32_t seed, bool adversary) {
  std::vector<int32_t> parent((size_t)n);
  Brute brute(n);
  // an adversarial start: a forest of long chains (parent[x] = x - 1 within a chain), the deepest a find can meet
  for (int32_t x = 0; x < n; ++x) {
    const bool head = x == 0 || (lcg(seed) >> 24) < 24;
    parent[(size_t)x] = head ? x : x - 1;
    if (!head) brute.join(x, x - 1);
  }
  int64_t adversary_trips = 0;
  for (int u = 0; u < unions; ++u) {
    const int32_t a = (int32_t)(lcg(seed) % (uint32_t)n), b = (int32_t)(lcg(seed) % (uint32_t)n);
    int64_t trips = 0;
    int depth = 0;
    // the other workgroups: between any two memory operations of this union, another complete union may land
    auto between = [&]() {
      if (!adversary || depth > 0 || (lcg(seed) >> 24) >= 96) return;
      ++depth;
      const int32_t c = (int32_t)(lcg(seed) % (uint32_t)n), d = (int32_t)(lcg(seed) % (uint32_t)n);
      ubi::model_unite(parent.data(), c, d, &adversary_trips, [] {});
      brute.join(c, d);
      --depth;
    };
    ubi::model_unite(parent.data(), a, b, &trips, between);
    brute.join(a, b);
    // each trip of a find and of the union loop lowers an index or is the loop's last: a + b bounds the union's own trips,
    // a and b its finds' on every trip
    if (trips > 2 * ((int64_t)a + b + 2) * ((int64_t)a + b + 2)) {
      std::fprintf(stderr, "cluster_host: a union of %d and %d took %lld trips\n", a, b, (long long)trips);
      return 1;
    }
    for (int32_t x = 0; x < n; ++x)
      if (parent[(size_t)x] > x || parent[(size_t)x] < 0) {
        std::fprintf(stderr, "cluster_host: parent[%d] = %d is not at or below its pixel\n", x, parent[(size_t)x]);
        return 1;
      }
  }
  for (int32_t x = 0; x < n; ++x) {
    int64_t t = 0;
    if (ubi::model_find(parent.data(), x, &t) != brute.comp[(size_t)x] || t > (int64_t)x + 1) {
      std::fprintf(stderr, "cluster_host: pixel %d of %d: the forest's root is not the smallest member of its component (adversary %d)\n", x, n,
                   (int)adversary);
      return 1;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if ((argc - 1) % 3) {
    std::fprintf(stderr, "usage: cluster_host [P rows cols]...\n");
    return 2;
  }
  for (int a = 1; a + 2 < argc; a += 3)
    if (check_image(std::atoll(argv[a]), std::atoll(argv[a + 1]), std::atoll(argv[a + 2]), true)) return 1;
  for (int64_t n = 1; n <= 3 * ubi::PIXEL_BLOCK + 1; n += (n < 70 ? 1 : 61))
    if (check_image(1, n, 1, false)) return 1;
  if (check_image(1, 3 * ubi::PIXEL_BLOCK + 1, 1, false) || check_image(1, 1, ubi::PIXEL_BLOCK, false)) return 1;
  // what the plan refuses: no pixel, and 2^31 pixels or more
  ubi::Plan p;
  if (ubi::make_plan(0, 4, 4, &p) || ubi::make_plan(1, -1, 4, &p) || ubi::make_plan(1, 4, 0, &p) || ubi::make_plan(2, 32768, 32768, &p) ||
      ubi::make_plan(1, 1 << 30, 1 << 30, &p) || !ubi::make_plan(1, 2147483647, 1, &p) || p.tiles != 67108864 ||
      !ubi::make_plan(3, 1008, 3456, &p))
    return fail("what make_plan refuses", 0, 0, 0, -1);
  if (p.tiles_y != 32 || p.tiles_x != 54 || p.tiles != 5184 || p.blocks != 10206 || p.scan_trips != 10 || p.scratch_bytes != 4 * 10208)
    return fail("the plan of the full event", 3, 1008, 3456, -1);
  if (ubi::stride_grid(0) != 0 || ubi::stride_grid(1) != 1 || ubi::stride_grid(ubi::LANES + 1) != 2 ||
      ubi::stride_grid((int64_t)ubi::MAX_GRID * ubi::LANES + 1) != ubi::MAX_GRID)
    return fail("stride_grid", 0, 0, 0, -1);
  for (int round = 0; round < 24; ++round) {
    const int32_t n = round < 4 ? round + 1 : 40 + 37 * round;
    if (check_unions(n, 3 * n, 1234u + (uint32_t)round, false) || check_unions(n, 3 * n, 99u + (uint32_t)round, true)) return 1;
  }
  std::printf("G %d %d %d %d %d %d %d\n", ubi::TILE_H, ubi::TILE_W, ubi::LANES, ubi::BORDER_LANES, ubi::PIXEL_BLOCK, ubi::SCAN_WIDTH,
              ubi::MAX_GRID);
  return 0;
}
