// The rule of libubresnet_det.so (ubresnet_amd/csrc/ubr_det_rule.h, plain C++ for a host compiler) as a stand-alone program,
// so that tests/test_cpu_det.py can run it under the host sanitizers:
//   det_host
// It prints one line per case, every number as a 32-bit pattern in hexadecimal:
//   W seed seq group r plane | w0 w1 w2 w3                              the Philox words of a counter
//   E x dead gain sigma all seed seq group r plane c | y                 ubx::element: x, gain, sigma and y are fp32 bit patterns
#include <cstdint>
#include <cstdio>
#include "ubr_det_rule.h"

int main() {
  const uint32_t keys[][2] = {{0u, 0u}, {1u, 0u}, {0u, 1u}, {0xFFFFFFFFu, 0xFFFFFFFFu}, {0x243F6A88u, 0x85A308D3u}, {7u, 1000u}};
  const uint32_t ctrs[][3] = {{0u, 0u, 0u}, {1u, 0u, 0u}, {0u, 1u, 0u}, {0u, 0u, 1u}, {207u, 511u, 47u},
                              {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, {0x13198A2Eu, 0x03707344u, 0xA4093822u}};
  for (const auto& k : keys)
    for (const auto& c : ctrs) {
      const ubx::Words w = ubx::words(k[0], k[1], c[0], c[1], c[2]);
      std::printf("W %08x %08x %08x %08x %08x | %08x %08x %08x %08x\n", k[0], k[1], c[0], c[1], c[2], w.w[0], w.w[1], w.w[2], w.w[3]);
    }
  // x: zeros of both signs, a subnormal, ordinary values, the largest finite, an infinity, NaNs with a payload
  const uint32_t xs[] = {0x00000000u, 0x80000000u, 0x00012345u, 0x3f800000u, 0xc2c80000u, 0x42f6e979u, 0x7f7fffffu, 0x7f800000u,
                         0x7fc00000u, 0xffc01234u};
  const uint32_t gains[] = {0x3f800000u, 0x3f8ccccdu, 0x3f666666u, 0xbf800000u, 0x00000000u};   // 1, 1.1, 0.9, -1, 0
  const uint32_t sigmas[] = {0x00000000u, 0x3fc00000u, 0x00000001u, 0x41200000u};               // 0, 1.5, the least subnormal, 10
  for (uint32_t xb : xs)
    for (uint32_t gb : gains)
      for (uint32_t sb : sigmas)
        for (int dead = 0; dead < 2; ++dead)
          for (int all = 0; all < 2; ++all)
            for (int c = 0; c < 4; ++c) {
              const uint32_t seed = 7u, seq = 3u + (uint32_t)all, group = 5u + (uint32_t)c, r = xb & 0xffu, plane = gb & 3u;
              const ubx::Words w = ubx::words(seed, seq, group, r, plane);
              const float y = ubx::element(ubx::from_bits(xb), dead != 0, gb, ubx::from_bits(sb), all != 0, w, c);
              std::printf("E %08x %d %08x %08x %d %08x %08x %08x %08x %08x %d | %08x\n", xb, dead, gb, sb, all, seed, seq, group, r, plane, c,
                          ubx::bits(y));
            }
  // the ends of the uniforms: u1 = 2^-24 (the largest radius), u1 = 1 (radius 0), the angles at the quarter turns
  const uint32_t as[] = {0x00000000u, 0x000000ffu, 0xffffff00u, 0xffffffffu, 0x80000000u};
  const uint32_t bs[] = {0x00000000u, 0x20000000u, 0x40000000u, 0x60000000u, 0x80000000u, 0xa0000000u, 0xc0000000u, 0xe0000000u, 0xffffffffu,
                         0x3fffff00u, 0x40000100u};
  for (uint32_t a : as)
    for (uint32_t b : bs) {
      const float rad = ubx::radius(a), ang = ubx::angle(b);
      std::printf("N %08x %08x | %08x %08x\n", a, b, ubx::bits(ubx::normal_even(rad, ang)), ubx::bits(ubx::normal_odd(rad, ang)));
    }
  return 0;
}
