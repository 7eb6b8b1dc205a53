// The decay schedule of libubresnet_ema.so (ube_advance of include/ubresnet_ema.h) as one inline function that a host
// compiler takes as well: the kernel in ubr_ema.hip calls it on the device, tests/ema_host.cpp compiles it into a stand-alone
// program with the host sanitizers on.
#ifndef UBR_EMA_SCHED_H
#define UBR_EMA_SCHED_H

#include <stdint.h>

#if defined(__HIPCC__)
#define UBE_HD __host__ __device__ __forceinline__
#else
#define UBE_HD inline
#endif

namespace ube {

struct Weight {
  float w;  // (float)(1 - d): what (param - shadow) is multiplied by
  float d;  // (float)d
};

// The update that follows `updates` applied ones.  Everything is fp64 until the two conversions at the end: the integers are
// exact in fp64 (below 2^53), the sum 1.0 + u and the quotient are rounded once each, 1.0 - d once.
UBE_HD Weight schedule(float decay, int64_t warmup, int64_t updates) {
  double d = (double)decay;
  if (warmup >= 2) {
    const double ramp = (1.0 + (double)updates) / (double)(warmup + updates);
    if (ramp < d) d = ramp;
  }
  Weight r;
  r.w = (float)(1.0 - d);
  r.d = (float)d;
  return r;
}

}  // namespace ube

#endif
