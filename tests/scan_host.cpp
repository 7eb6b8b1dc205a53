// The pixel-block compaction the event-product libraries share (ubresnet_amd/csrc/ubr_scan_plan.h, plain C++ for a host compiler)
// as a stand-alone program, so that tests/test_cpu_sparse.py can run it under the host sanitizers:
//   scan_host
// At 1, B - 1, B, B + 1 pixels and at S and S + 1 blocks (B the pixel block, S the scan width), then at every size up to three
// blocks and one pixel, it checks that the plan tiles the pixels, the blocks and the scratch, then runs host_count / host_scan /
// host_rank over four occupancies and holds them against brute force, in a scratch buffer of exactly the planned words.  Then
// stride_grid at 0, 1, lanes + 1 and past the cap, and what the plan refuses.  It prints one line for each of the six sizes
// named first, `I pixels blocks scan_trips scratch_bytes`, then `G lanes lane_pixels pixel_block scan_width`, and exits 1 at the
// first disagreement.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "ubr_scan_plan.h"

namespace sp = scanplan;

static int fail(const char* what, int64_t n, int occ) {
  std::fprintf(stderr, "scan_host: %s (%lld pixels, occupancy %d)\n", what, (long long)n, occ);
  return 1;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int check_size(int64_t n, bool print) {
  sp::BlockPlan p;
  if (!sp::make_block_plan(1, n, 1, &p)) return fail("make_block_plan refused", n, -1);
  if (p.pixels != n || p.blocks < 1 || (p.blocks - 1) * sp::PIXEL_BLOCK >= n || p.blocks * sp::PIXEL_BLOCK < n)
    return fail("blocks do not tile the pixels", n, -1);
  if (p.scan_trips < 1 || (p.scan_trips - 1) * sp::SCAN_WIDTH >= p.blocks || p.scan_trips * sp::SCAN_WIDTH < p.blocks)
    return fail("scan trips do not tile the blocks", n, -1);
  if (p.scratch_words < p.blocks || p.scratch_words % sp::SCAN_LANE_COUNTS || p.scratch_words - p.blocks >= sp::SCAN_LANE_COUNTS ||
      p.scratch_bytes != 4 * p.scratch_words)
    return fail("scratch layout", n, -1);
  if (sp::lane_pixel(0, 0, 0) != 0 || sp::lane_pixel(p.blocks - 1, sp::LANES - 1, sp::LANE_PIXELS - 1) != p.blocks * sp::PIXEL_BLOCK - 1)
    return fail("lane_pixel", n, -1);
  if (print) std::printf("I %lld %lld %lld %lld\n", (long long)p.pixels, (long long)p.blocks, (long long)p.scan_trips, (long long)p.scratch_bytes);
  std::vector<uint8_t> named((size_t)n);
  std::vector<uint32_t> scratch((size_t)p.scratch_words);        // exactly the planned words: a step outside is the sanitizer's
  uint32_t seed = (uint32_t)(n * 2654435761u) + 41u;
  for (int occ = 0; occ < 4; ++occ) {                             // none, all, every other block, about 30 %
    for (int64_t q = 0; q < n; ++q)
      named[(size_t)q] = occ == 0 ? 0 : occ == 1 ? 1 : occ == 2 ? (uint8_t)((q / sp::PIXEL_BLOCK) % 2 == 0) : (uint8_t)((lcg(seed) >> 24) < 77);
    const auto is_named = [&named](int64_t q) { return named[(size_t)q] != 0; };
    std::vector<int64_t> brute;
    for (int64_t q = 0; q < n; ++q)
      if (named[(size_t)q]) brute.push_back(q);
    const int64_t total = (int64_t)brute.size();
    for (auto& w : scratch) w = 0xDEADBEEFu;                      // the pass must write every word it later reads
    sp::host_count(p, is_named, scratch.data());
    for (int64_t b = 0; b < p.blocks; ++b) {
      uint32_t want = 0;
      for (int64_t q = b * sp::PIXEL_BLOCK; q < (b + 1) * sp::PIXEL_BLOCK && q < n; ++q) want += named[(size_t)q];
      if (scratch[(size_t)b] != want) return fail("a block's count", n, occ);
    }
    if ((int64_t)sp::host_scan(p, scratch.data()) != total) return fail("the scan's total", n, occ);
    uint32_t run = 0;
    for (int64_t b = 0; b < p.blocks; ++b) {
      if (scratch[(size_t)b] != run) return fail("the scan is not the exclusive prefix", n, occ);
      for (int64_t q = b * sp::PIXEL_BLOCK; q < (b + 1) * sp::PIXEL_BLOCK && q < n; ++q) run += named[(size_t)q];
    }
    int64_t calls = 0;
    bool ok = true;
    sp::host_rank(p, is_named, scratch.data(), [&](int64_t q, int64_t k) {
      ok = ok && k == calls && k < total && brute[(size_t)k] == q;
      ++calls;
    });
    if (!ok || calls != total) return fail("the ranks are not the ascending order of the named pixels", n, occ);
  }
  return 0;
}

int main() {
  const int64_t B = sp::PIXEL_BLOCK, S = sp::SCAN_WIDTH;
  for (int64_t n : {(int64_t)1, B - 1, B, B + 1, S * B, S * B + 1})
    if (check_size(n, true)) return 1;
  for (int64_t n = 2; n <= 3 * B + 1; ++n)                        // and every size up to three blocks and one
    if (check_size(n, false)) return 1;
  // what the plan refuses: no pixel, and 2^31 pixels or more
  sp::BlockPlan p;
  if (sp::make_block_plan(0, 4, 4, &p) || sp::make_block_plan(1, -1, 4, &p) || sp::make_block_plan(1, 4, 0, &p) ||
      sp::make_block_plan(2, 32768, 32768, &p) || sp::make_block_plan(1, 1 << 30, 1 << 30, &p) || !sp::make_block_plan(1, 2147483647, 1, &p) ||
      !sp::make_block_plan(3, 1008, 3456, &p))
    return fail("what make_block_plan refuses", 0, -1);
  if (p.blocks != 10206 || p.scan_trips != 10 || p.scratch_bytes != 4 * 10208) return fail("the plan of the full event", 3 * 1008 * 3456, -1);
  const int64_t lanes = 256, cap = 4096;
  if (sp::stride_grid(0, lanes, cap) != 0 || sp::stride_grid(1, lanes, cap) != 1 || sp::stride_grid(lanes + 1, lanes, cap) != 2 ||
      sp::stride_grid(cap * lanes, lanes, cap) != cap || sp::stride_grid(cap * lanes + 1, lanes, cap) != cap || sp::stride_grid(65, 64, 3) != 2 ||
      sp::stride_grid(1000, 64, 3) != 3)
    return fail("stride_grid", 0, -1);
  std::printf("G %d %d %d %d\n", sp::LANES, sp::LANE_PIXELS, sp::PIXEL_BLOCK, sp::SCAN_WIDTH);
  return 0;
}
