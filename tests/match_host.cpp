// The launch plan of libubresnet_match.so (ubresnet_amd/csrc/ubr_match_plan.h, plain C++ for a host compiler) as a stand-alone
// program, so that tests/test_cpu_match.py can run it under the host sanitizers:
//   match_host P rows cols time_bin slots capacity [P rows cols time_bin slots capacity ...]
// For every geometry given, and for a ladder of others, it checks that the plan's walk is ubr_walk_plan.h's, the time bins and
// chunks (every row falls into a bin below T and every bin into a chunk below `chunks`, marked in buffers of exactly that size),
// the trips of the select, the grids, the scratch layout (three parts that do not overlap, each large enough and aligned) and
// the bound of a 32-bit bin.  Then the tile enumeration for every number of tiles: tile_of visits every pair ti <= tj < nt once,
// in row order, marked in a buffer of exactly nt * nt bytes.  Then what the plan refuses.  It prints one line per geometry,
// `I P rows cols time_bin slots capacity T chunks select_trips clear_grid summary_grid match_grid scratch_bytes`, then
// `G lanes trip_pixels max_grid tile chunk_bins min_slots max_slots max_time_bin max_shift max_bin_pixels`, and exits 1 at the first
// disagreement.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ubr_match_plan.h"

static int fail(const char* what, int64_t a, int64_t b, int64_t c) {
  std::fprintf(stderr, "match_host: %s (%lld, %lld, %lld)\n", what, (long long)a, (long long)b, (long long)c);
  return 1;
}

static int check_plan(int64_t P, int64_t rows, int64_t cols, int64_t bin, int64_t slots, int64_t capacity, bool print) {
  ubu::Plan p;
  const char* why;
  if (!ubu::make_plan(P, rows, cols, bin, slots, capacity, &p, &why) || *why != 0) return fail("make_plan refused", P, rows, cols);
  const int64_t n = P * rows * cols;
  const walk::Walk w = walk::make_walk(n);
  if (p.pixels != n || p.trips != w.trips || p.span != w.span || p.grid != w.grid) return fail("the walk is not the walk plan's", P, rows, cols);
  if (((int64_t)1 << p.log2_bin) != bin || p.T != (rows + bin - 1) / bin || p.chunks != (p.T + ubu::CHUNK_BINS - 1) / ubu::CHUNK_BINS)
    return fail("time bins or chunks", rows, bin, p.T);
  std::vector<uint8_t> bins((size_t)p.T, 0), chunk((size_t)p.chunks, 0);   // exactly T and chunks: a step outside is the sanitizer's
  for (int64_t r = 0; r < rows; ++r) bins[(size_t)(r >> p.log2_bin)] = 1;
  for (int64_t t = 0; t < p.T; ++t) {
    if (!bins[(size_t)t]) return fail("a bin without a row", rows, bin, t);
    chunk[(size_t)(t / ubu::CHUNK_BINS)] = 1;
  }
  for (int64_t c = 0; c < p.chunks; ++c)
    if (!chunk[(size_t)c]) return fail("a chunk without a bin", rows, bin, c);
  if (ubu::bin_bound(bin, cols) >= ((uint64_t)1 << 32)) return fail("a bin can pass 32 bits", bin, cols, 0);
  if (p.rows_max != (capacity < n ? capacity : n) || p.select_trips * ubu::LANES < p.rows_max || (p.select_trips - 1) * ubu::LANES >= p.rows_max)
    return fail("select trips", capacity, p.rows_max, p.select_trips);
  if (p.clear_grid < 1 || p.clear_grid > ubu::MAX_GRID || (p.clear_grid < ubu::MAX_GRID && p.clear_grid * ubu::LANES < slots * p.T))
    return fail("clear grid", slots, p.T, p.clear_grid);
  if (p.summary_grid * ubu::WAVES != slots || p.tiles * ubu::TILE != slots || p.match_grid != ubu::tile_count(p.tiles))
    return fail("summary or match grid", slots, p.summary_grid, p.match_grid);
  if (p.mask_bytes != 8 * slots * p.chunks || p.occ_offset != p.mask_bytes || p.occ_offset % 8 || p.occ_bytes < 4 * slots * p.T ||
      p.slot_offset != p.occ_offset + p.occ_bytes || p.slot_offset % 16 || p.slot_bytes < 4 * p.rows_max ||
      p.scratch_bytes != p.slot_offset + p.slot_bytes || p.scratch_bytes % 16)
    return fail("scratch layout", p.mask_bytes, p.occ_bytes, p.slot_bytes);
  if (print)
    std::printf("I %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)P, (long long)rows, (long long)cols, (long long)bin,
                (long long)slots, (long long)capacity, (long long)p.T, (long long)p.chunks, (long long)p.select_trips, (long long)p.clear_grid,
                (long long)p.summary_grid, (long long)p.match_grid, (long long)p.scratch_bytes);
  return 0;
}

static int check_tiles(int nt) {
  std::vector<uint8_t> seen((size_t)nt * nt, 0);
  int want_i = 0, want_j = 0;
  for (int b = 0; b < (int)ubu::tile_count(nt); ++b) {
    int ti, tj;
    ubu::tile_of(b, nt, &ti, &tj);
    if (ti != want_i || tj != want_j) return fail("tile_of is not the row order of the upper triangle", nt, b, ti);
    if (seen[(size_t)ti * nt + tj]++) return fail("a tile twice", nt, ti, tj);
    if (++want_j == nt) { ++want_i; want_j = want_i; }
  }
  for (int i = 0; i < nt; ++i)
    for (int j = 0; j < nt; ++j)
      if (seen[(size_t)i * nt + j] != (i <= j ? 1 : 0)) return fail("the tiles are not the upper triangle", nt, i, j);
  return 0;
}

int main(int argc, char** argv) {
  if ((argc - 1) % 6) {
    std::fprintf(stderr, "usage: match_host [P rows cols time_bin slots capacity]...\n");
    return 2;
  }
  for (int a = 1; a + 5 < argc; a += 6)
    if (check_plan(std::atoll(argv[a]), std::atoll(argv[a + 1]), std::atoll(argv[a + 2]), std::atoll(argv[a + 3]), std::atoll(argv[a + 4]),
                   std::atoll(argv[a + 5]), true))
      return 1;
  for (int64_t rows = 1; rows <= 4096; rows += (rows < 140 ? 1 : 389))
    for (int64_t bin = 1; bin <= ubu::MAX_TIME_BIN; bin *= 2)
      if (check_plan(2 + rows % 3, rows, 1 + (rows * 7) % 1024, bin, 64 * (1 + rows % 64), 1 + rows * 31, false)) return 1;
  if (check_plan(3, 1008, 3456, 1, 512, 65536, false) || check_plan(4, 1024, 4096, 16, 4096, (int64_t)1 << 40, false) ||
      check_plan(2, 4096, 1024, 64, 64, 1, false))
    return 1;
  for (int nt = 1; nt <= (int)(ubu::MAX_SLOTS / ubu::TILE); ++nt)
    if (check_tiles(nt)) return 1;
  // what the plan refuses, and the edges it admits
  ubu::Plan p;
  const char* why;
  if (ubu::make_plan(1, 4, 4, 1, 64, 8, &p, &why) || ubu::make_plan(5, 4, 4, 1, 64, 8, &p, &why) || ubu::make_plan(2, 0, 4, 1, 64, 8, &p, &why) ||
      ubu::make_plan(2, 4, -1, 1, 64, 8, &p, &why) || ubu::make_plan(2, 4097, 4, 1, 64, 8, &p, &why) || ubu::make_plan(2, 4, 4097, 1, 64, 8, &p, &why) ||
      ubu::make_plan(2, 2048, 4096, 1, 64, 8, &p, &why) || ubu::make_plan(2, 4, 4, 0, 64, 8, &p, &why) || ubu::make_plan(2, 4, 4, 3, 64, 8, &p, &why) ||
      ubu::make_plan(2, 4, 4, 128, 64, 8, &p, &why) || ubu::make_plan(2, 64, 4096, 32, 64, 8, &p, &why) || ubu::make_plan(2, 64, 1025, 64, 64, 8, &p, &why) ||
      ubu::make_plan(2, 4, 4, 1, 0, 8, &p, &why) || ubu::make_plan(2, 4, 4, 1, 32, 8, &p, &why) || ubu::make_plan(2, 4, 4, 1, 96, 8, &p, &why) ||
      ubu::make_plan(2, 4, 4, 1, 4160, 8, &p, &why) || ubu::make_plan(2, 4, 4, 1, -64, 8, &p, &why) || ubu::make_plan(2, 4, 4, 1, 64, 0, &p, &why) ||
      *why == 0)
    return fail("what make_plan refuses", 0, 0, 0);
  if (!ubu::make_plan(2, 64, 4096, 16, 64, 8, &p, &why) || !ubu::make_plan(4, 1024, 4096, 1, 4096, 1, &p, &why) || *why != 0 ||
      !ubu::make_plan(3, 1008, 3456, 1, 512, 65536, &p, &why))
    return fail("what make_plan admits", 0, 0, 0);
  if (p.T != 1008 || p.chunks != 16 || p.select_trips != 256 || p.trips != 5103 || p.span != 5 || p.grid != 1021 || p.match_grid != 36 ||
      p.summary_grid != 128 || p.clear_grid != ubu::MAX_GRID)
    return fail("the plan of the full event", p.T, p.chunks, p.match_grid);
  if (ubu::bin_bound(16, 4096) != 4294901760ull || ubu::log2_time_bin(64) != 6 || ubu::log2_time_bin(1) != 0 || ubu::log2_time_bin(48) != -1)
    return fail("bin_bound or log2_time_bin", 0, 0, 0);
  std::printf("G %d %d %d %d %d %lld %lld %d %d %lld\n", ubu::LANES, ubu::TRIP_PIXELS, ubu::MAX_GRID, ubu::TILE, ubu::CHUNK_BINS, (long long)ubu::MIN_SLOTS,
              (long long)ubu::MAX_SLOTS, ubu::MAX_TIME_BIN, ubu::MAX_SHIFT, (long long)ubu::MAX_BIN_PIXELS);
  return 0;
}
