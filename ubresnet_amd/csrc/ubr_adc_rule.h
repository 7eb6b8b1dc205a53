// The weight of an ADC value (include/ubresnet_moment.h states the rule; libubresnet_overlap.so weighs a pixel the same way) as one
// inline function that a host compiler takes as well: moment_kernel and insert_kernel call it on the device, tests/walk_host.cpp
// compiles it into a stand-alone program with the host sanitizers on and prints what tests/moment_ref.py is compared with.  One
// fp32 multiply by a power of two and one rint; build with -ffp-contract=off.
#ifndef UBR_ADC_RULE_H
#define UBR_ADC_RULE_H

#include <stdint.h>
#include <string.h>
#include "ubr_walk_plan.h"

#if defined(__HIPCC__)
#define UBW_HD __host__ __device__ __forceinline__
#else
#define UBW_HD inline
#endif

namespace adc {

enum Class { PLAIN = 0, CLIPPED = 1, ODD = 2 };   // ODD: NaN or below zero, weight 0; CLIPPED: above MAX_WEIGHT, weight MAX_WEIGHT

struct Weight {
  uint32_t w;
  Class cls;
};

// scale: a power of two in 1..MAX_SCALE (walk::valid_scale).  The sign and NaN tests read the bits, so that they do not depend on
// how the float unit treats a subnormal; scale > 0, so t < 0 iff v < 0.
UBW_HD Weight weight_of(float v, float scale) {
  uint32_t bits;
  memcpy(&bits, &v, 4);
  const uint32_t mag = bits & 0x7FFFFFFFu;
  if (mag > 0x7F800000u || ((bits >> 31) != 0u && mag != 0u)) return {0u, ODD};
  const float t = v * scale;                                      // exact: scale is a power of two
  if (t > (float)walk::MAX_WEIGHT) return {(uint32_t)walk::MAX_WEIGHT, CLIPPED};
  return {(uint32_t)__builtin_rintf(t), PLAIN};                   // ties to even
}

}  // namespace adc

#endif
