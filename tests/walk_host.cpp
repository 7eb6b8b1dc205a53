// The pixel walk and the weight rule that libubresnet_moment.so and libubresnet_overlap.so share (ubresnet_amd/csrc/ubr_walk_plan.h
// and ubr_adc_rule.h, plain C++ for a host compiler) as a stand-alone program, so that tests/test_cpu_moment.py can run it under
// the host sanitizers:
//   walk_host stride [bits-of-an-ADC-value-in-hex ...]
// (a) For 1 .. a few trips of pixels, for the pixel counts around MAX_GRID * TRIP_PIXELS up to a few trips past it, and for the
// full event it checks that the spans of the workgroups tile the trips and that the trips tile the pixels, marking every pixel of
// every lane slot of every trip in a buffer of exactly `pixels` bytes; it prints `W pixels trips span grid` for the named ones.
// (b) It checks the scales valid_scale accepts; for every valid scale it prints `E scale bits weight class` for each ADC value given, then `S scale stride` and one line of
// `weight * 4 + class` in hex for the floats of bits 0, stride, 2 stride, ... below 2^32.  It exits 1 at the first disagreement.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ubr_adc_rule.h"
#include "ubr_walk_plan.h"

static int fail(const char* what, int64_t n) {
  std::fprintf(stderr, "walk_host: %s (%lld pixels)\n", what, (long long)n);
  return 1;
}

static int check_walk(int64_t n, bool print) {
  const walk::Walk p = walk::make_walk(n);
  if (p.pixels != n || p.trips < 1 || (p.trips - 1) * walk::TRIP_PIXELS >= n || p.trips * walk::TRIP_PIXELS < n)
    return fail("trips do not tile the pixels", n);
  if (p.grid < 1 || p.grid > walk::MAX_GRID || p.span < 1 || (p.grid - 1) * p.span >= p.trips || p.grid * p.span < p.trips)
    return fail("spans do not tile the trips", n);
  if (print) std::printf("W %lld %lld %lld %lld\n", (long long)n, (long long)p.trips, (long long)p.span, (long long)p.grid);
  // the kernels' walk: workgroup g, trip t of its span, load u, lane l, pixel j; a pixel at or past `pixels` is not touched
  std::vector<uint8_t> seen((size_t)n, 0);                         // exactly the pixels: a step outside is the sanitizer's
  for (int64_t g = 0; g < p.grid; ++g) {
    const int64_t t0 = g * p.span, t1 = (t0 + p.span < p.trips) ? t0 + p.span : p.trips;
    if (t0 >= t1) return fail("a workgroup without a trip", n);
    for (int64_t t = t0; t < t1; ++t)
      for (int u = 0; u < walk::TRIP_LOADS; ++u)
        for (int l = 0; l < walk::LANES; ++l) {
          const int64_t q = t * walk::TRIP_PIXELS + (int64_t)u * walk::LANES * walk::LANE_PIXELS + (int64_t)l * walk::LANE_PIXELS;
          if (q % walk::LANE_PIXELS) return fail("a lane's first pixel is not a multiple of four", n);
          for (int j = 0; j < walk::LANE_PIXELS; ++j)
            if (q + j < n && seen[(size_t)(q + j)]++) return fail("a pixel is visited twice", n);
        }
  }
  for (int64_t q = 0; q < n; ++q)
    if (seen[(size_t)q] != 1) return fail("a pixel is not visited", n);
  return 0;
}

static float from_bits(uint32_t bits) {
  float v;
  std::memcpy(&v, &bits, 4);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2 || std::atoll(argv[1]) < 1) {
    std::fprintf(stderr, "usage: walk_host stride [adc-bits-in-hex]...\n");
    return 2;
  }
  // (a)
  const int64_t full = (int64_t)walk::MAX_GRID * walk::TRIP_PIXELS, event = (int64_t)3 * 1008 * 3456;
  for (int64_t n = 1; n <= 3 * walk::TRIP_PIXELS + 1; n += (n < 70 ? 1 : 127))
    if (check_walk(n, n == 1)) return 1;
  for (int64_t n : {(int64_t)3 * walk::TRIP_PIXELS + 1, full - walk::TRIP_PIXELS, full - 1, full, full + 1, full + walk::TRIP_PIXELS, 2 * full, 2 * full + 1,
                    full + 3 * walk::TRIP_PIXELS + 5, event})
    if (check_walk(n, true)) return 1;
  const walk::Walk e = walk::make_walk(event);
  if (e.trips != 5103 || e.span != 5 || e.grid != 1021) return fail("the walk of the full event", event);
  // (b)
  for (int s = -2; s <= 600; ++s) {
    const bool want = s == 1 || s == 2 || s == 4 || s == 8 || s == 16 || s == 32 || s == 64 || s == 128 || s == 256;
    if (walk::valid_scale((float)s) != want || walk::valid_scale((float)s + 0.5f)) return fail("valid_scale", s);
  }
  if (walk::valid_scale(0.5f) || walk::valid_scale(1.0f / 0.0f) || walk::valid_scale(0.0f / 0.0f)) return fail("valid_scale", 0);
  const uint64_t stride = (uint64_t)std::atoll(argv[1]);
  for (int scale = 1; scale <= walk::MAX_SCALE; scale *= 2) {
    if (!walk::valid_scale((float)scale)) return fail("valid_scale", scale);
    for (int a = 2; a < argc; ++a) {
      const uint32_t bits = (uint32_t)std::strtoul(argv[a], nullptr, 16);
      const adc::Weight r = adc::weight_of(from_bits(bits), (float)scale);
      std::printf("E %d %08x %u %d\n", scale, bits, r.w, (int)r.cls);
    }
    std::printf("S %d %llu\n", scale, (unsigned long long)stride);
    for (uint64_t bits = 0; bits < ((uint64_t)1 << 32); bits += stride) {
      const adc::Weight r = adc::weight_of(from_bits((uint32_t)bits), (float)scale);
      if (r.w > (uint32_t)walk::MAX_WEIGHT || (r.cls == adc::ODD && r.w != 0) || (r.cls == adc::CLIPPED && r.w != (uint32_t)walk::MAX_WEIGHT))
        return fail("a weight outside its class", (int64_t)bits);
      std::printf("%x ", r.w * 4u + (unsigned)r.cls);
    }
    std::printf("\n");
  }
  return 0;
}
