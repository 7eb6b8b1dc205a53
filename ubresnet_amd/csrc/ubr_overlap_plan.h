// The launch plan, the pair key, the hash and the probe sequence of libubresnet_overlap.so (include/ubresnet_overlap.h) as plain
// C++: no HIP, so tests/overlap_host.cpp compiles it into a stand-alone program with the host sanitizers on.  The clear grid, the
// scratch layout, what is refused, the key of a pair, its home slot and how far it probes are decided here and nowhere else;
// host_insert / host_lookup restate the device's insert and look-up one key at a time, for the host program to hold against every
// insertion order.  The trip, the grid and the span of trips of a workgroup of the insert are the pixel walk of ubr_walk_plan.h,
// which libubresnet_moment.so shares; the pixel-block compaction of launches 3 to 5 is ubr_scan_plan.h, unchanged.
//
// The overflow bound.  An image has fewer than 2^31 pixels, so `first` and `pixels` are below 2^31 and so is `weighted`.  A weight
// is at most MAX_WEIGHT = 2^16 - 1, so Q is below 2^31 * 2^16 = 2^47.  No column of a row, no word of a slot and no partial sum
// in a lane, a wave or the LDS table -- each a sum over a subset of the same pixels -- can overflow 64 bits.  Within one wave round
// a lane holds at most LANE_PIXELS pixels and a wave WAVE * LANE_PIXELS = 256: the two pixel counts (two fields of COUNT_BITS bits
// in one word, each at most 256) and the charge (at most 256 * MAX_WEIGHT < 2^24) are summed in 32 bits.
//
// The key of the pair (a, b), a and b >= -1 and not both -1, is (a + 1) << 32 | (b + 1): never 0, which marks an empty slot.
#ifndef UBR_OVERLAP_PLAN_H
#define UBR_OVERLAP_PLAN_H

#include "ubr_scan_plan.h"                            // the block plan of launches 3 to 5, and MAX_PIXELS
#include "ubr_walk_plan.h"

namespace ubh {

using walk::WAVE; using walk::LANES; using walk::LANE_PIXELS; using walk::TRIP_LOADS; using walk::TRIP_PIXELS;
using walk::MAX_GRID;                                 // workgroups of the insert and of the clear
using walk::COUNT_BITS;                               // pixels | weighted << 10 within one wave round
using walk::MAX_WEIGHT; using walk::MAX_SCALE; using walk::valid_scale;
constexpr int LDS_SLOTS = 64;                         // pairs of the LDS table of a workgroup
constexpr int LDS_PROBES = 4;                         // LDS slots a pair tries before it goes to memory directly
constexpr int FLUSH_ABOVE = LDS_SLOTS / 2;            // the LDS table is sent and emptied at the end of a trip that leaves more taken
constexpr int COLUMNS = 6;                            // a, b, first, pixels, weighted, Q
constexpr int SLOT_WORDS = 5;                         // uint64 words of a slot in scratch: key, first, pixels, weighted, Q
constexpr int MAX_PROBES = 128;
constexpr int64_t MIN_SLOTS = 64;
constexpr int64_t MAX_SLOTS = (int64_t)1 << 30;
constexpr int64_t DEFAULT_MIN_SLOTS = 1024;
constexpr int64_t MAX_CAPACITY = (int64_t)1 << 31;    // pairs are no more than pixels; a larger table is never filled
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;    // 2^64 / the golden ratio, odd: multiplying by it permutes the keys
constexpr uint64_t EMPTY_KEY = 0;
constexpr uint64_t NO_FIRST = ~(uint64_t)0;           // `first` of a slot nobody has added to: above every pixel index
using scanplan::MAX_PIXELS;
static_assert((LDS_SLOTS & (LDS_SLOTS - 1)) == 0 && LDS_SLOTS <= WAVE && LDS_PROBES <= LDS_SLOTS, "one lane of a wave flushes one LDS slot");
static_assert((uint64_t)MAX_PIXELS * MAX_WEIGHT < ((uint64_t)1 << 47), "Q < 2^47");
static_assert(TRIP_PIXELS == 2 * scanplan::PIXEL_BLOCK && LANES == scanplan::LANES, "launches 3 to 5 use the workgroup of the scan plan");

// ---- key, home slot, probe limit ----
inline bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

inline int log2_of(int64_t pow2) {
  int l = 0;
  while (((int64_t)1 << l) < pow2) ++l;
  return l;
}

// a, b: any int32; a negative value is "none".  0 for the pair of two nones, which does not take part.
inline uint64_t pair_key(int32_t a, int32_t b) {
  const uint64_t ka = a < 0 ? 0u : (uint64_t)(uint32_t)a + 1u, kb = b < 0 ? 0u : (uint64_t)(uint32_t)b + 1u;
  return ka << 32 | kb;
}
inline int64_t key_a(uint64_t key) { return (int64_t)(key >> 32) - 1; }
inline int64_t key_b(uint64_t key) { return (int64_t)(key & 0xFFFFFFFFull) - 1; }

// the home slot of a key in a table of 2^log2_slots slots, 1 <= log2_slots <= 63
inline uint64_t home_slot(uint64_t key, int log2_slots) { return (key * GOLDEN) >> (64 - log2_slots); }

// UBH_PROBES: slots a key tries, from its home slot on, cyclically
inline int64_t probes(int64_t slots) { return slots < MAX_PROBES ? slots : MAX_PROBES; }

inline bool valid_slots(int64_t slots) { return slots >= MIN_SLOTS && slots <= MAX_SLOTS && is_pow2(slots); }

// ubh_default_slots: the smallest power of two >= 2 * capacity and at least DEFAULT_MIN_SLOTS: a load of at most 0.5 with a table
// of `capacity` pairs; 0 for a capacity below 1 or one whose slots would pass MAX_SLOTS
inline int64_t default_slots(int64_t capacity) {
  if (capacity < 1 || capacity > MAX_SLOTS / 2) return 0;
  int64_t s = DEFAULT_MIN_SLOTS;
  while (s < 2 * capacity) s *= 2;
  return s;
}

// ---- the plan ----
struct Plan : walk::Walk {   // pixels = P * rows * cols, and the trips, span and grid of the insert
  int64_t clear_grid;     // workgroups of the clear: they stride over `slots` slots, one per lane
  int log2_slots;
  int64_t probes;         // probes(slots)
  scanplan::BlockPlan blocks;   // launches 3 to 5
  int64_t slot_bytes;     // scratch: the slots first, [slots][SLOT_WORDS] uint64 ...
  int64_t scratch_bytes;  // ... then the block counts of the scan plan, uint32 [blocks.scratch_words], 16-byte aligned
};

// what the image may be; the reason it is refused in *why if not
inline bool valid_image(int64_t P, int64_t rows, int64_t cols, const char** why) {
  *why = "P, rows and cols must be positive";
  if (P < 1 || rows < 1 || cols < 1) return false;
  *why = "P * rows * cols must be below 2^31 pixels (int32 pixel index)";
  if (rows > MAX_PIXELS / P || cols > MAX_PIXELS / (P * rows)) return false;
  *why = "";
  return true;
}

// false (and nothing defined in *p) for an image valid_image refuses or slots valid_slots refuses
inline bool make_plan(int64_t P, int64_t rows, int64_t cols, int64_t slots, Plan* p) {
  const char* why;
  if (!valid_image(P, rows, cols, &why) || !valid_slots(slots)) return false;
  if (!scanplan::make_block_plan(P, rows, cols, &p->blocks)) return false;
  static_cast<walk::Walk&>(*p) = walk::make_walk(P * rows * cols);
  p->clear_grid = scanplan::stride_grid(slots, LANES, MAX_GRID);
  p->log2_slots = log2_of(slots);
  p->probes = probes(slots);
  p->slot_bytes = slots * SLOT_WORDS * 8;             // slots >= 64: a multiple of 16
  p->scratch_bytes = p->slot_bytes + p->blocks.scratch_bytes;
  return true;
}

// ---- the insert and the look-up, one key at a time: keys[slots], EMPTY_KEY where free ----

// the slot that belongs to `key` after the insert -- one that held it or the first free one of its probe sequence, now taken -- or
// -1 where its `probes` slots all belong to other keys.  A slot is never freed.
inline int64_t host_insert(uint64_t* keys, int64_t slots, uint64_t key) {
  const int l = log2_of(slots);
  const uint64_t h = home_slot(key, l);
  for (int64_t p = 0; p < probes(slots); ++p) {
    const uint64_t s = (h + (uint64_t)p) & (uint64_t)(slots - 1);
    if (keys[s] == EMPTY_KEY) keys[s] = key;
    if (keys[s] == key) return (int64_t)s;
  }
  return -1;
}

// the slot that holds `key`, or -1: the same sequence, read-only, ending at a free slot or at the probe limit
inline int64_t host_lookup(const uint64_t* keys, int64_t slots, uint64_t key) {
  const int l = log2_of(slots);
  const uint64_t h = home_slot(key, l);
  for (int64_t p = 0; p < probes(slots); ++p) {
    const uint64_t s = (h + (uint64_t)p) & (uint64_t)(slots - 1);
    if (keys[s] == key) return (int64_t)s;
    if (keys[s] == EMPTY_KEY) return -1;
  }
  return -1;
}

}  // namespace ubh

#endif
