// The launch plan, the key, the hash and the probe sequence of libubresnet_overlap.so (ubresnet_amd/csrc/ubr_overlap_plan.h and
// ubr_scan_plan.h, plain C++ for a host compiler) as a stand-alone program, so that tests/test_cpu_overlap.py can run it under
// the host sanitizers:
//   overlap_host P rows cols slots [P rows cols slots ...]
// For every image given, and for a ladder of 1 x 1 x n images, it checks that the plan's walk is ubr_walk_plan.h's (that the walk
// tiles the pixels, and the scales it accepts, are tests/walk_host.cpp's to check), that the pixel blocks of launches 3 to 5 tile
// the pixels (in a buffer of exactly `pixels` bytes), the clear grid and the scratch layout.  Then what the plan refuses, the key of a pair, the default slots, and a sequential model of
// insert-then-look-up over shuffled insertion orders: the (key -> sums) content and the set of occupied slots are the same for
// every order, and with a table too small every key is found by every later look-up or by none.  It prints one line per image,
// `I P rows cols pixels trips span grid clear_grid blocks scratch_bytes`, then `G lanes trip_pixels max_grid lds_slots lds_probes
// flush_above columns slot_words max_probes min_slots`, and exits 1 at the first disagreement.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>
#include "ubr_overlap_plan.h"
#include "ubr_scan_plan.h"

static int fail(const char* what, int64_t P, int64_t rows, int64_t cols) {
  std::fprintf(stderr, "overlap_host: %s (%lld x %lld x %lld)\n", what, (long long)P, (long long)rows, (long long)cols);
  return 1;
}

static int check_image(int64_t P, int64_t rows, int64_t cols, int64_t slots, bool print) {
  ubh::Plan p;
  if (!ubh::make_plan(P, rows, cols, slots, &p)) return fail("make_plan refused", P, rows, cols);
  const int64_t n = P * rows * cols;
  const walk::Walk w = walk::make_walk(n);
  if (p.pixels != n || p.trips != w.trips || p.span != w.span || p.grid != w.grid) return fail("the walk is not the walk plan's", P, rows, cols);
  if (p.clear_grid < 1 || p.clear_grid > ubh::MAX_GRID || (p.clear_grid < ubh::MAX_GRID && p.clear_grid * ubh::LANES < slots))
    return fail("clear grid", P, rows, cols);
  scanplan::BlockPlan b;
  if (!scanplan::make_block_plan(P, rows, cols, &b) || b.blocks != p.blocks.blocks || b.scan_trips != p.blocks.scan_trips ||
      b.scratch_bytes != p.blocks.scratch_bytes)
    return fail("the block plan is not the scan plan's", P, rows, cols);
  if (p.slot_bytes != slots * ubh::SLOT_WORDS * 8 || p.slot_bytes % 16 || p.scratch_bytes != p.slot_bytes + b.scratch_bytes ||
      ((int64_t)1 << p.log2_slots) != slots || p.probes != (slots < ubh::MAX_PROBES ? slots : ubh::MAX_PROBES))
    return fail("scratch layout, log2 or probes", P, rows, cols);
  if (print)
    std::printf("I %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)P, (long long)rows, (long long)cols, (long long)p.pixels,
                (long long)p.trips, (long long)p.span, (long long)p.grid, (long long)p.clear_grid, (long long)b.blocks,
                (long long)p.scratch_bytes);
  // the count and number passes: block b, lane l, pixel j; a pixel at or past `pixels` is not touched
  std::vector<uint8_t> seen((size_t)n, 0);                         // exactly the pixels: a step outside is the sanitizer's
  for (int64_t blk = 0; blk < b.blocks; ++blk)
    for (int l = 0; l < scanplan::LANES; ++l)
      for (int j = 0; j < scanplan::LANE_PIXELS; ++j) {
        const int64_t q = scanplan::lane_pixel(blk, l, j);
        if (q < n && seen[(size_t)q]++) return fail("the blocks do not tile the pixels", P, rows, cols);
      }
  for (int64_t q = 0; q < n; ++q)
    if (seen[(size_t)q] != 1) return fail("a pixel is in no block", P, rows, cols);
  return 0;
}

struct Sums {
  uint64_t first, pixels, q;
  bool operator==(const Sums& o) const { return first == o.first && pixels == o.pixels && q == o.q; }
};

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rng() {                                            // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

// `groups`: (key, first, pixels, q) contributions, several per key; inserted in `orders` shuffled orders into a table of `slots`.
// With room for every key: the content and the occupied set are those of the first order.  Without: a key is found by every
// look-up after its first insert attempt or by none of them, its sums are complete if it is found, and the dropped pixels plus
// the stored pixels are all the pixels.
static int check_orders(int64_t slots, int64_t nkeys, int per_key, int orders, bool must_fit) {
  struct Group { uint64_t key; Sums s; };
  std::vector<Group> groups;
  std::map<uint64_t, Sums> truth;
  uint64_t all_pixels = 0;
  for (int64_t i = 0; i < nkeys; ++i) {
    const int32_t a = (int32_t)(rng() % 3 == 0 ? -1 - (int32_t)(rng() % 5) : (int32_t)(rng() % 2000000000u));
    const int32_t b = (int32_t)(a < 0 || rng() % 4 ? (int32_t)(rng() % 70000u) : -1);
    const uint64_t key = ubh::pair_key(a, b);
    if (key == ubh::EMPTY_KEY) return fail("a pair that takes part has key 0", a, b, 0);
    if (ubh::key_a(key) != (a < 0 ? -1 : a) || ubh::key_b(key) != (b < 0 ? -1 : b)) return fail("key_a / key_b", a, b, 0);
    if (truth.count(key)) continue;
    Sums t = {ubh::NO_FIRST, 0, 0};
    for (int g = 0; g < per_key; ++g) {
      const Sums s = {rng() % 2147483647u, 1 + rng() % 256, rng() % (256 * 65535u)};
      groups.push_back({key, s});
      t.first = s.first < t.first ? s.first : t.first;
      t.pixels += s.pixels;
      t.q += s.q;
      all_pixels += s.pixels;
    }
    truth[key] = t;
  }
  std::set<int64_t> occupied0;
  std::map<uint64_t, Sums> content0;
  for (int o = 0; o < orders; ++o) {
    for (size_t i = groups.size(); i > 1; --i) std::swap(groups[i - 1], groups[(size_t)(rng() % i)]);
    std::vector<uint64_t> keys((size_t)slots, ubh::EMPTY_KEY);
    std::vector<Sums> sums((size_t)slots, Sums{ubh::NO_FIRST, 0, 0});
    std::map<uint64_t, int> fate;                                  // 1: found so far, -1: dropped so far
    uint64_t dropped = 0;
    for (const Group& g : groups) {
      const int64_t s = ubh::host_insert(keys.data(), slots, g.key);
      const int now = s >= 0 ? 1 : -1;
      if (fate.count(g.key) && fate[g.key] != now) return fail("a pair partly in the table and partly dropped", slots, nkeys, o);
      fate[g.key] = now;
      if (ubh::host_lookup(keys.data(), slots, g.key) != s) return fail("the look-up does not find what the insert found", slots, nkeys, o);
      if (s < 0) { dropped += g.s.pixels; continue; }
      Sums& t = sums[(size_t)s];
      t.first = g.s.first < t.first ? g.s.first : t.first;
      t.pixels += g.s.pixels;
      t.q += g.s.q;
    }
    std::set<int64_t> occupied;
    std::map<uint64_t, Sums> content;
    uint64_t stored = 0;
    for (int64_t s = 0; s < slots; ++s)
      if (keys[(size_t)s] != ubh::EMPTY_KEY) {
        occupied.insert(s);
        if (content.count(keys[(size_t)s])) return fail("a key in two slots", slots, nkeys, o);
        content[keys[(size_t)s]] = sums[(size_t)s];
        stored += sums[(size_t)s].pixels;
      }
    for (const auto& kv : fate) {                                  // every later look-up agrees with the inserts
      const int64_t s = ubh::host_lookup(keys.data(), slots, kv.first);
      if ((s >= 0) != (kv.second > 0)) return fail("a later look-up disagrees with the inserts", slots, nkeys, o);
      if (s >= 0 && !(content[kv.first] == truth[kv.first])) return fail("the sums of a stored pair are not complete", slots, nkeys, o);
    }
    if (stored + dropped != all_pixels) return fail("stored + dropped pixels", slots, nkeys, o);
    if (must_fit) {
      if (dropped != 0 || content.size() != truth.size()) return fail("a key found no slot in a table with room", slots, nkeys, o);
      if (o == 0) { occupied0 = occupied; content0 = content; }
      else if (occupied != occupied0 || !(content == content0)) return fail("content or occupied slots depend on the order", slots, nkeys, o);
    } else if (dropped == 0) {
      return fail("the small table dropped nothing: the case checks nothing", slots, nkeys, o);
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if ((argc - 1) % 4) {
    std::fprintf(stderr, "usage: overlap_host [P rows cols slots]...\n");
    return 2;
  }
  for (int a = 1; a + 3 < argc; a += 4)
    if (check_image(std::atoll(argv[a]), std::atoll(argv[a + 1]), std::atoll(argv[a + 2]), std::atoll(argv[a + 3]), true)) return 1;
  for (int64_t n = 1; n <= 3 * ubh::TRIP_PIXELS + 1; n += (n < 70 ? 1 : 127))
    if (check_image(1, 1, n, (int64_t)64 << (n % 5), false)) return 1;
  if (check_image(1, 3, ubh::TRIP_PIXELS + 1, 64, false) || check_image(3, 1008, 3456, 262144, false)) return 1;
  // what the plan refuses
  ubh::Plan p;
  const char* why;
  if (ubh::make_plan(0, 4, 4, 64, &p) || ubh::make_plan(1, -1, 4, 64, &p) || ubh::make_plan(1, 4, 0, 64, &p) ||
      ubh::make_plan(512, 1024, 4096, 64, &p) || ubh::make_plan(1, 46341, 46341, 64, &p) || ubh::make_plan(1, 4, 4, 0, &p) ||
      ubh::make_plan(1, 4, 4, 32, &p) || ubh::make_plan(1, 4, 4, 96, &p) || ubh::make_plan(1, 4, 4, -64, &p) ||
      ubh::make_plan(1, 4, 4, ubh::MAX_SLOTS * 2, &p) || !ubh::make_plan(1, 4, 4, ubh::MAX_SLOTS, &p) ||
      !ubh::make_plan(1, 1, 2147483647, 64, &p) || !ubh::make_plan(3, 1008, 3456, 262144, &p))
    return fail("what make_plan refuses", 0, 0, 0);
  if (p.trips != 5103 || p.span != 5 || p.grid != 1021 || p.clear_grid != ubh::MAX_GRID || p.log2_slots != 18 || p.probes != 128)
    return fail("the plan of the full event", 3, 1008, 3456);
  if (ubh::valid_image(1 << 20, 1 << 20, 1 << 20, &why) || !ubh::valid_image(3, 1008, 3456, &why) || *why != 0) return fail("valid_image", 0, 0, 0);
  // the key: never 0 for a pair that takes part, 0 for two nones, every negative id is none, the largest ids fit
  if (ubh::pair_key(-1, -1) != 0 || ubh::pair_key(-7, INT32_MIN) != 0 || ubh::pair_key(0, -1) != ((uint64_t)1 << 32) || ubh::pair_key(-1, 0) != 1 ||
      ubh::pair_key(-5, 3) != ubh::pair_key(-1, 3) || ubh::pair_key(INT32_MAX, INT32_MAX) != (((uint64_t)1 << 31) << 32 | ((uint64_t)1 << 31)) ||
      ubh::key_a(ubh::pair_key(INT32_MAX, -2)) != INT32_MAX || ubh::key_b(ubh::pair_key(INT32_MAX, -2)) != -1)
    return fail("pair_key", 0, 0, 0);
  // the home slot is below the slots for every table size; the default slots are a power of two at a load of at most 0.5
  for (int l = 6; l <= 30; ++l)
    for (int i = 0; i < 1000; ++i)
      if (ubh::home_slot(rng() | 1, l) >= ((uint64_t)1 << l)) return fail("home_slot", l, 0, 0);
  for (int64_t c = 1; c <= ubh::MAX_SLOTS / 2; c = c < 5000 ? c + 1 : c * 2 - 1 + (c % 3)) {
    const int64_t s = ubh::default_slots(c);
    if (!ubh::valid_slots(s) || s < 1024 || s < 2 * c || (s > 1024 && s / 2 >= 2 * c)) return fail("default_slots", c, s, 0);
  }
  if (ubh::default_slots(0) != 0 || ubh::default_slots(-3) != 0 || ubh::default_slots(ubh::MAX_SLOTS / 2 + 1) != 0 ||
      ubh::default_slots(131072) != 262144 || ubh::default_slots(512) != 1024 || ubh::default_slots(513) != 2048)
    return fail("default_slots at its edges", 0, 0, 0);
  // insert then look-up over shuffled orders: tables with room (load 0.5 and a nearly full small one), and tables too small
  if (check_orders(1024, 512, 3, 6, true) || check_orders(64, 60, 4, 8, true) || check_orders(64, 64, 2, 4, true) ||
      check_orders(4096, 2048, 2, 4, true) || check_orders(64, 500, 3, 6, false) || check_orders(256, 2000, 2, 4, false))
    return 1;
  std::printf("G %d %d %d %d %d %d %d %d %d %lld\n", ubh::LANES, ubh::TRIP_PIXELS, ubh::MAX_GRID, ubh::LDS_SLOTS, ubh::LDS_PROBES,
              ubh::FLUSH_ABOVE, ubh::COLUMNS, ubh::SLOT_WORDS, ubh::MAX_PROBES, (long long)ubh::MIN_SLOTS);
  return 0;
}
