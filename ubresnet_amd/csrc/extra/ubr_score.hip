// libubresnet_score.so: event products scored against a truth image (include/ubresnet_score.h).  It links against none of the
// other libraries and shares ubr_sat.h with them and ubr_wave.h (the key walk, the wave sum) with the other event-product
// libraries; the launch is a plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include "../../../include/ubresnet_score.h"
#include "../ubr_sat.h"
#include "../ubr_wave.h"

#define UBQ_VERSION 1

SAT_RETURN_CODES(UBQ);
SAT_EXPORTS(ubq, UBQ_VERSION)
using namespace sat;

namespace {

constexpr int TH = UBQ_TILE_H, TW = UBQ_TILE_W, BLOCK = 256;
constexpr int LP = 4;                                         // consecutive pixels of a tile row per lane and slot
constexpr int ROW_LANES = TW / LP;                            // 32 lanes per tile row: a wave takes two rows
constexpr int SLOT_ROWS = BLOCK / ROW_LANES;                  // 8 tile rows per slot
constexpr int SLOTS = TH / SLOT_ROWS;                         // 4
constexpr int GRID_X = 256;                                   // workgroups per plane at most: each walks tiles GRID_X apart
constexpr int STAGE = 8;                                      // truth loads in flight per lane while the tile is staged
constexpr int SH_MAX = TH + 2 * UBQ_MAX_RADIUS, SW_MAX = TW + 2 * UBQ_MAX_RADIUS;
constexpr int MAX_WORDS = 2 * UBQ_MAX_CLASSES * UBQ_MAX_CLASSES + 2 * UBQ_MAX_BINS * 3 + 4;
constexpr unsigned NONE = 255u;                               // a truth that is not a class, or a pixel outside the view
static_assert(TW == 128 && TH % SLOT_ROWS == 0, "the index arithmetic below assumes a 128-wide tile");

struct ScoreK {
  const uint8_t* label;
  const uint16_t* conf;
  const void* truth;
  unsigned long long* table;
  int rows, cols, C, fill, R, lo, bins, tiles_x, tiles;      // tiles: of one plane
  int vlab, vconf;                                            // the 4-byte label / 8-byte confidence load of a lane is aligned
  uint16_t edges[UBQ_MAX_BINS];                               // bins - 1 of them
};

// the class of a truth value, NONE if it is none: compared on the full width of its type, then narrowed
__device__ __forceinline__ unsigned class_of(uint8_t v, int C) { return (int)v < C ? (unsigned)v : NONE; }
__device__ __forceinline__ unsigned class_of(long long v, int C) { return (v >= 0ll && v < (long long)C) ? (unsigned)v : NONE; }

// grid (x: at most GRID_X workgroups that walk the tiles of a plane, row-major, GRID_X apart; y: plane).  The fewer workgroups,
// the fewer global atomics on the same few words at the end (step 4), which is what a launch of one workgroup per tile spent
// its time on.  Per TH x TW tile a workgroup does this:
//   1. it stages the tile's truth with an R-wide halo in LDS, a byte per pixel: the class, or NONE for a value that is no class
//      and for a pixel outside the view -- and notes the set of classes >= lo it met;
//   2. only if that set holds two classes or more can any pixel of the tile have a contact: then the window test runs,
//      separably -- the set of classes >= lo in columns x-R..x+R of every staged row, here; the union over rows y-R..y+R, per
//      scored pixel, below;
//   3. a lane takes LP consecutive pixels of a tile row in each of SLOTS slots (their labels and confidences were loaded first
//      of all, so that these loads and the staging's are in flight together).  A wave without a lit pixel and without dark
//      signal in a slot does nothing more for it.  Scored pixels are counted per wave: the lanes whose (stratum, truth, label,
//      bin) agree with the first remaining lane's are found by ballot, their confidences summed across the wave, and that one
//      lane adds the group to the workgroup's LDS table; so an event whose pixels all agree costs one group per wave and pixel;
//   4. after its last tile, the non-zero words of the LDS table are added to the plane's table with 64-bit integer atomics,
//      the kernel's only global writes.
template <typename T>
__global__ __launch_bounds__(BLOCK) void score_kernel(const ScoreK k) {
  __shared__ unsigned long long tab[MAX_WORDS];
  __shared__ unsigned short rm[SH_MAX * TW];
  __shared__ unsigned char ids[SH_MAX * SW_MAX];
  __shared__ unsigned s_present[2];                           // the classes >= lo of the staged tile; slots alternate by tile
  const int t = threadIdx.x, lane = t & 63;
  const int C = k.C, R = k.R, lo = k.lo, bins = k.bins, rows = k.rows, cols = k.cols;
  const int SW = TW + 2 * R, SH = TH + 2 * R;
  const int conf_words = 2 * C * C, words = conf_words + 6 * bins + 4, tally_at = words - 4;
  const long plane = (long)blockIdx.y * ((long)rows * cols);
  for (int i = t; i < words; i += BLOCK) tab[i] = 0ull;
  if (t < 2) s_present[t] = 0u;
  __syncthreads();
  unsigned long long n_scored = 0ull, n_ignored = 0ull, n_dark = 0ull;       // wave-uniform
  unsigned it = 0u;
  for (unsigned tile = blockIdx.x; tile < (unsigned)k.tiles; tile += gridDim.x, ++it) {      // tiles < 2^31: no wrap
    const int tile_y = (int)(tile / (unsigned)k.tiles_x), tile_x = (int)(tile - (unsigned)tile_y * (unsigned)k.tiles_x);
    const int y0 = tile_y * TH, x0 = tile_x * TW;

    // the lane's labels and confidences of every slot, loaded before anything waits: LP pixels packed in one and two words
    const uint8_t* label = k.label + plane;
    const uint16_t* conf = k.conf + plane;
    const int ry = t / ROW_LANES, x = (t % ROW_LANES) * LP;    // the lane's row within a slot, its first column in the tile
    const unsigned fill4 = (unsigned)k.fill * 0x01010101u;
    unsigned labw[SLOTS];
    uint2 confw[SLOTS];
#pragma unroll
    for (int slot = 0; slot < SLOTS; ++slot) {
      const int gy = y0 + slot * SLOT_ROWS + ry, gx = x0 + x;
      labw[slot] = fill4;                                      // a pixel outside the view: not lit
      confw[slot] = make_uint2(0u, 0u);
      if (gy < rows && gx < cols) {
        const long o = (long)gy * cols + gx;
        if (k.vlab) {                                          // cols % 4 == 0: gx + 3 < cols
          labw[slot] = *reinterpret_cast<const unsigned*>(label + o);
        } else {
#pragma unroll
          for (int q = 0; q < LP; ++q)
            if (gx + q < cols) labw[slot] = (labw[slot] & ~(255u << (8 * q))) | ((unsigned)label[o + q] << (8 * q));
        }
        if (k.vconf) {
          confw[slot] = *reinterpret_cast<const uint2*>(conf + o);
        } else {
          unsigned h[LP] = {0u, 0u, 0u, 0u};
#pragma unroll
          for (int q = 0; q < LP; ++q) if (gx + q < cols) h[q] = conf[o + q];
          confw[slot] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
        }
      }
    }

    const T* truth = reinterpret_cast<const T*>(k.truth) + plane;
    unsigned mine = 0u;
    for (int i0 = t; i0 < SH * SW; i0 += BLOCK * STAGE) {       // STAGE independent loads in flight per lane; SH * SW <= sizeof(ids)
      T raw[STAGE];
#pragma unroll
      for (int u = 0; u < STAGE; ++u) {
        const int i = i0 + u * BLOCK;
        raw[u] = (T)NONE;                                      // 255 is no class
        if (i < SH * SW) {
          const int sy = i / SW, sx = i - sy * SW;
          const int gy = y0 - R + sy, gx = x0 - R + sx;
          if (gy >= 0 && gy < rows && gx >= 0 && gx < cols) raw[u] = truth[(long)gy * cols + gx];
        }
      }
#pragma unroll
      for (int u = 0; u < STAGE; ++u) {
        const int i = i0 + u * BLOCK;
        if (i < SH * SW) {
          const unsigned v = class_of(raw[u], C);
          ids[i] = (unsigned char)v;
          if (v != NONE && (int)v >= lo) mine |= 1u << v;
        }
      }
    }
    if (mine != 0u) atomicOr(&s_present[it & 1u], mine);
    __syncthreads();
    const unsigned present = s_present[it & 1u];
    if (t == 0) s_present[(it + 1u) & 1u] = 0u;                // the next tile's slot: last read before the barrier that ended the tile before
    const bool window = R > 0 && (present & (present - 1u)) != 0u;     // the same for the whole workgroup
    if (window) {
      for (int i = t; i < SH * TW; i += BLOCK) {
        const unsigned char* row = ids + (i >> 7) * SW + (i & (TW - 1));   // staged columns x .. x+2R are tile columns x-R .. x+R
        unsigned m = 0u;
        for (int d = 0; d <= 2 * R; ++d) {
          const unsigned v = row[d];
          if (v != NONE && (int)v >= lo) m |= 1u << v;
        }
        rm[i] = (unsigned short)m;
      }
      __syncthreads();
    }

#pragma unroll
    for (int slot = 0; slot < SLOTS; ++slot) {
      const int y = slot * SLOT_ROWS + ry;
      unsigned lab[LP], hb[LP];
#pragma unroll
      for (int q = 0; q < LP; ++q) lab[q] = (labw[slot] >> (8 * q)) & 255u;
      hb[0] = confw[slot].x & 0xFFFFu; hb[1] = confw[slot].x >> 16; hb[2] = confw[slot].y & 0xFFFFu; hb[3] = confw[slot].y >> 16;
      unsigned tr[LP];
      bool lit[LP], busy = false;
#pragma unroll
      for (int q = 0; q < LP; ++q) {
        tr[q] = ids[(y + R) * SW + (x + q + R)];
        lit[q] = lab[q] != (unsigned)k.fill;
        busy |= lit[q] || (tr[q] != NONE && tr[q] >= 1u);
      }
      if (__ballot(busy) == 0ull) continue;                    // wave-uniform
#pragma unroll
      for (int q = 0; q < LP; ++q) {
        const bool dark = !lit[q] && tr[q] != NONE && tr[q] >= 1u;
        const bool ignored = lit[q] && (tr[q] == NONE || (int)lab[q] >= C);
        const bool scored = lit[q] && !ignored;
        n_dark += (unsigned)__popcll(__ballot(dark));
        n_ignored += (unsigned)__popcll(__ballot(ignored));
        unsigned long long rem = __ballot(scored);
        if (rem == 0ull) continue;                             // wave-uniform
        n_scored += (unsigned)__popcll(rem);
        unsigned key = 0xFFFFFFFFu;
        unsigned long long fx = 0ull;
        if (scored) {
          unsigned s = 0u;
          if (window && (int)tr[q] >= lo) {
            unsigned m = 0u;
            for (int d = 0; d <= 2 * R; ++d) m |= rm[(y + d) * TW + x + q];
            s = (m & ~(1u << tr[q])) != 0u ? 1u : 0u;
          }
          const unsigned h = hb[q] == 0x8000u ? 0u : hb[q];
          unsigned b = (unsigned)bins;                         // bins: not binned
          if ((h & 0x8000u) == 0u && (h & 0x7C00u) != 0x7C00u) {
            b = 0u;
            for (int e = 0; e < bins - 1; ++e) b += (unsigned)k.edges[e] <= h ? 1u : 0u;
            const unsigned ex = h >> 10, m = h & 1023u;
            fx = ex == 0u ? (unsigned long long)m : (unsigned long long)(1024u + m) << (ex - 1u);
          }
          key = (s << 14) | (tr[q] << 10) | (lab[q] << 6) | b;  // tr, lab < 16; b <= 32
        }
        while (rem != 0ull) {                                   // wave-uniform: one trip per distinct key among the scored lanes
          const wv::KeyGroup<unsigned> g = wv::next_key_group(rem, key, scored);
          const unsigned n = (unsigned)__popcll(g.lanes);
          unsigned long long sum = g.member ? fx : 0ull;
          if (n > 1u) sum = wv::sum_all(sum);
          if (lane == g.leader) {
            const unsigned kk = g.key, s = kk >> 14, tt = (kk >> 10) & 15u, ll = (kk >> 6) & 15u, b = kk & 63u;
            atomicAdd(&tab[(s * C + tt) * C + ll], (unsigned long long)n);
            if ((int)b < bins) {
              unsigned long long* r = tab + conf_words + (s * bins + b) * 3;
              atomicAdd(r, (unsigned long long)n);
              if (tt == ll) atomicAdd(r + 1, (unsigned long long)n);
              if (sum != 0ull) atomicAdd(r + 2, sum);
            } else {
              atomicAdd(&tab[tally_at + 3], (unsigned long long)n);
            }
          }
        }
      }
    }
    __syncthreads();                                           // ids and rm are free for the next tile
  }
  if (lane == 0) {
    if (n_scored != 0ull) atomicAdd(&tab[tally_at + 0], n_scored);
    if (n_ignored != 0ull) atomicAdd(&tab[tally_at + 1], n_ignored);
    if (n_dark != 0ull) atomicAdd(&tab[tally_at + 2], n_dark);
  }
  __syncthreads();
  unsigned long long* out = k.table + (long)blockIdx.y * words;
  for (int i = t; i < words; i += BLOCK) {
    const unsigned long long v = tab[i];
    if (v != 0ull) atomicAdd(out + i, v);
  }
}

inline long long table_words(int P, int C, int bins) { return (long long)P * (2 * C * C + 6 * bins + 4); }

}  // namespace

extern "C" int ubq_table_words(int P, int C, int bins) {
  SAT_CHECK(P >= 1, "ubq_table_words: P=%d must be >= 1", P);
  SAT_CHECK(C >= 1 && C <= UBQ_MAX_CLASSES, "ubq_table_words: C=%d must be 1..%d", C, UBQ_MAX_CLASSES);
  SAT_CHECK(bins >= 1 && bins <= UBQ_MAX_BINS, "ubq_table_words: bins=%d must be 1..%d", bins, UBQ_MAX_BINS);
  const long long w = table_words(P, C, bins);
  SAT_CHECK(w <= 0x7FFFFFFFll, "ubq_table_words: %lld words do not fit an int", w);
  return (int)w;
}

extern "C" int ubq_score_event(const uint8_t* label, const uint16_t* confidence, const void* truth, int truth_kind,
                               int C, int fill_label, int radius, int interface_from,
                               const uint16_t* edges_host, int bins,
                               unsigned long long* table, int P, int rows, int cols, void* stream) {
  // the scalar arguments first, the pointers last: a refusal names the first thing that is wrong with the call
  SAT_CHECK(truth_kind == UBQ_TRUTH_U8 || truth_kind == UBQ_TRUTH_I64, "ubq_score_event: truth_kind=%d must be %d (uint8) or %d (int64)",
            truth_kind, UBQ_TRUTH_U8, UBQ_TRUTH_I64);
  SAT_CHECK(C >= 1 && C <= UBQ_MAX_CLASSES, "ubq_score_event: C=%d must be 1..%d", C, UBQ_MAX_CLASSES);
  SAT_CHECK(fill_label >= 0 && fill_label <= 255, "ubq_score_event: fill_label=%d must be 0..255", fill_label);
  SAT_CHECK(radius >= 0 && radius <= UBQ_MAX_RADIUS, "ubq_score_event: radius=%d must be 0..%d", radius, UBQ_MAX_RADIUS);
  SAT_CHECK(interface_from >= 0 && interface_from <= C, "ubq_score_event: interface_from=%d must be 0..C=%d", interface_from, C);
  SAT_CHECK(bins >= 1 && bins <= UBQ_MAX_BINS, "ubq_score_event: bins=%d must be 1..%d", bins, UBQ_MAX_BINS);
  SAT_CHECK(P >= 1 && P <= 65535 && rows >= 1 && cols >= 1, "ubq_score_event: P=%d must be 1..65535, rows=%d and cols=%d >= 1", P, rows, cols);
  SAT_CHECK(bins == 1 || edges_host, "ubq_score_event: edges_host is null with bins=%d", bins);
  ScoreK k{};
  for (int e = 0; e < bins - 1; ++e) {
    const unsigned h = edges_host[e];
    SAT_CHECK(h >= 0x0001u && h <= 0x7BFFu, "ubq_score_event: edge %d (0x%04X) is not a positive finite half", e, h);
    SAT_CHECK(e == 0 || h > edges_host[e - 1], "ubq_score_event: edges not strictly ascending at %d (0x%04X after 0x%04X)", e, h,
              (unsigned)edges_host[e - 1]);
    k.edges[e] = (uint16_t)h;
  }
  const long long tiles_x = ((long long)cols + TW - 1) / TW, tiles_y = ((long long)rows + TH - 1) / TH;
  SAT_CHECK(tiles_x * tiles_y <= 0x7FFFFFFFll, "ubq_score_event: %lld x %lld tiles exceed the grid", tiles_y, tiles_x);
  SAT_CHECK(table_words(P, C, bins) <= 0x7FFFFFFFll, "ubq_score_event: the table does not fit an int of words");
  SAT_CHECK(label && confidence && truth && table, "ubq_score_event: null pointer (label %p, confidence %p, truth %p, table %p)",
            (const void*)label, (const void*)confidence, truth, (void*)table);
  SAT_CHECK(aligned(confidence, 2) && aligned(table, 8) && (truth_kind == UBQ_TRUTH_U8 || aligned(truth, 8)),
            "ubq_score_event: a pointer lacks its natural alignment (2 bytes for a half, 8 for a 64-bit integer)");
  k.label = label; k.conf = confidence; k.truth = truth; k.table = table;
  k.rows = rows; k.cols = cols; k.C = C; k.fill = fill_label; k.R = radius; k.lo = interface_from; k.bins = bins;
  k.tiles_x = (int)tiles_x;
  k.tiles = (int)(tiles_x * tiles_y);
  k.vlab = cols % LP == 0 && aligned(label, 4);
  k.vconf = cols % LP == 0 && aligned(confidence, 8);
  const long long gx = tiles_x * tiles_y < GRID_X ? tiles_x * tiles_y : GRID_X;
  const dim3 grid((unsigned)gx, (unsigned)P), block(BLOCK);
  if (truth_kind == UBQ_TRUTH_U8)
    score_kernel<uint8_t><<<grid, block, 0, (hipStream_t)stream>>>(k);
  else
    score_kernel<long long><<<grid, block, 0, (hipStream_t)stream>>>(k);
  SAT_LAUNCH_CHECK("ubq_score_event");
  return UBQ_OK;
}
