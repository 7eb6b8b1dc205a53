// The rule of libubresnet_det.so (include/ubresnet_det.h states it) as inline functions that a host compiler takes as well:
// the kernel in ubr_det.hip calls them on the device, tests/det_host.cpp compiles them into a stand-alone program with the host
// sanitizers on.  Every statement is one fp32 operation or one library call; build with -ffp-contract=off.
//
// What the host program does and does not cover.  The kernel composes words / radius / angle / normal_even / normal_odd / gained /
// noisy / noised itself, per lane and pair; normal() and element() below are the same composition for ONE element and are called
// by the host program only.  On the host, cospi / sinpi are an fp64 substitute for the device's cospif / sinpif, and logf and
// sqrtf are the host's.  So the host program holds the integer part (Philox, the uniforms), the exact part (dead, gain, which
// pixel is noisy) and the rule's arithmetic as written; the kernel's own control flow and the device's library functions are
// held by tests/test_gpu_det_exact.py alone.
#ifndef UBR_DET_RULE_H
#define UBR_DET_RULE_H

#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../include/ubresnet_det.h"

#if defined(__HIPCC__)
#define UBX_HD __host__ __device__ __forceinline__
#else
#define UBX_HD inline
#endif

namespace ubx {

struct Words {
  uint32_t w[4];
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", 2011)
UBX_HD Words philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t m0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t m1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1;
    c0 = n0;
    c1 = (uint32_t)m1;
    c2 = n2;
    c3 = (uint32_t)m0;
    k0 += 0x9E3779B9u;      // (the bump after the tenth round is never used)
    k1 += 0xBB67AE85u;
  }
  Words r;
  r.w[0] = c0; r.w[1] = c1; r.w[2] = c2; r.w[3] = c3;
  return r;
}

// the words of the four columns 4 * group .. 4 * group + 3 of row r of plane `plane` = b * P + p
UBX_HD Words words(uint32_t seed, uint32_t seq, uint32_t group, uint32_t r, uint32_t plane) {
  return philox(seed, seq, group, r, plane, UBX_PHILOX_TAG);
}

// (0, 1] and [0, 1): a 24-bit integer converts exactly, and so does the product with a power of two
UBX_HD float uniform_open0(uint32_t a) { return (float)((a >> 8) + 1u) * 0x1p-24f; }
UBX_HD float uniform_open1(uint32_t b) { return (float)(b >> 8) * 0x1p-24f; }

#if defined(__HIP_DEVICE_COMPILE__)
UBX_HD float mul(float a, float b) { return __fmul_rn(a, b); }
UBX_HD float add(float a, float b) { return __fadd_rn(a, b); }
UBX_HD float root(float a) { return __fsqrt_rn(a); }
UBX_HD float cospi(float x) { return cospif(x); }
UBX_HD float sinpi(float x) { return sinpif(x); }
#else
UBX_HD float mul(float a, float b) { return a * b; }
UBX_HD float add(float a, float b) { return a + b; }
UBX_HD float root(float a) { return sqrtf(a); }
// a host libm need not have cospif / sinpif: x in [0, 2) is split exactly into a quarter turn count and t in [-1/4, 1/4], the
// rest is fp64 and one rounding
UBX_HD double turn(float x, int* quarter) {
  const double n = nearbyint(2.0 * (double)x);
  *quarter = (int)n & 3;
  return (double)x - 0.5 * n;
}
UBX_HD float cospi(float x) {
  int q;
  const double a = 3.14159265358979323846 * turn(x, &q);
  return (float)(q == 0 ? cos(a) : (q == 1 ? -sin(a) : (q == 2 ? -cos(a) : sin(a))));
}
UBX_HD float sinpi(float x) {
  int q;
  const double a = 3.14159265358979323846 * turn(x, &q);
  return (float)(q == 0 ? sin(a) : (q == 1 ? cos(a) : (q == 2 ? -sin(a) : -cos(a))));
}
#endif

// Box-Muller radius and angle of a pair of words: the even column of the pair takes the cosine, the odd one the sine
UBX_HD float radius(uint32_t a) {
  const float l = logf(uniform_open0(a));
  const float m = mul(-2.0f, l);
  return root(m);
}
UBX_HD float angle(uint32_t b) { return mul(2.0f, uniform_open1(b)); }   // exact: in [0, 2)
UBX_HD float normal_even(float rad, float ang) { return mul(rad, cospi(ang)); }
UBX_HD float normal_odd(float rad, float ang) { return mul(rad, sinpi(ang)); }

// z of column c (its row and plane are in the words): pair (w0, w1) for c & 3 in {0, 1}, (w2, w3) for {2, 3}
UBX_HD float normal(const Words& w, int c) {
  const int pair = (c >> 1) & 1;
  const float rad = radius(w.w[2 * pair]), ang = angle(w.w[2 * pair + 1]);
  return (c & 1) ? normal_odd(rad, ang) : normal_even(rad, ang);
}

UBX_HD uint32_t bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}
UBX_HD float from_bits(uint32_t u) {
  float x;
  memcpy(&x, &u, 4);
  return x;
}

#define UBX_ONE_BITS 0x3f800000u

// steps 1 and 2: a dead wire reads +0.0f; a gain whose bits are those of 1.0f multiplies nothing
UBX_HD float gained(float x, bool dead, uint32_t gain_bits) {
  if (dead) return 0.0f;
  return gain_bits == UBX_ONE_BITS ? x : mul(x, from_bits(gain_bits));
}

// whether step 3 applies to a live pixel that held x (sigma > 0 is the caller's): a NaN is lit
UBX_HD bool noisy(float x, bool noise_all) { return noise_all || x != 0.0f; }

// step 3
UBX_HD float noised(float y, float sigma, float z) { return add(y, mul(sigma, z)); }

// the whole rule for one element
UBX_HD float element(float x, bool dead, uint32_t gain_bits, float sigma, bool noise_all, const Words& w, int c) {
  const float y = gained(x, dead, gain_bits);
  if (dead || !(sigma > 0.0f) || !noisy(x, noise_all)) return y;
  return noised(y, sigma, normal(w, c));
}

}  // namespace ubx

#endif
