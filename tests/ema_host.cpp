// The decay schedule of libubresnet_ema.so (ubresnet_amd/csrc/ubr_ema_sched.h, plain C++ for a host compiler) as a stand-alone
// program, so that tests/test_cpu_ema.py can run it under the host sanitizers:
//   ema_host DECAY_BITS WARMUP U0 U1
// DECAY_BITS is the fp32 bit pattern of the decay in hex.  Prints, for u = U0 .. U1 - 1, one line `u w_bits d_bits` with the bit
// patterns of the two floats of ube::schedule(decay, WARMUP, u) in hex.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ubr_ema_sched.h"

static uint32_t bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, sizeof b);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: %s DECAY_BITS WARMUP U0 U1\n", argv[0]);
    return 2;
  }
  const uint32_t db = (uint32_t)std::strtoul(argv[1], nullptr, 16);
  float decay;
  std::memcpy(&decay, &db, sizeof decay);
  const long long warmup = std::atoll(argv[2]), u0 = std::atoll(argv[3]), u1 = std::atoll(argv[4]);
  for (long long u = u0; u < u1; ++u) {
    const ube::Weight s = ube::schedule(decay, (int64_t)warmup, (int64_t)u);
    std::printf("%lld %08x %08x\n", u, bits(s.w), bits(s.d));
  }
  return 0;
}
