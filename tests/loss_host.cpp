// The arithmetic of libubresnet_loss.so (ubresnet_amd/csrc/ubr_loss_term.h, plain C++ for a host compiler) as a stand-alone
// program, so that tests/test_cpu_loss.py can run it under the host sanitizers:
//   loss_host
// It walks the edge cases of the per-pixel term and of the finish rule and prints one line per case, every float as a C99
// hexadecimal literal (%a; nan, inf and -inf as such):
//   T lp gamma w_c pw s | q m term d g            the term, its derivative and the gradient g = grad(s, pw, w_c, d)
//   M mode loss_sum weight_sum valid total | denom inv_denom loss
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include "ubr_loss_term.h"

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const float lps[] = {0.f, -0.0f, -1e-30f, -1e-45f, -104.f, -110.f, -inf, 1e-3f, std::numeric_limits<float>::quiet_NaN(),
                       -1e-3f, -0.6931472f, -5.f, -87.f};
  const float gammas[] = {0.f, 0.01f, 0.5f, 1.f, 2.f, 5.f};
  const float w_c = 2.f, pw = 0.5f, s = 0.25f;
  for (float gamma : gammas)
    for (float lp : lps) {
      const float q = ubl::miss(lp), m = ubl::modulator(q, gamma);
      const float t = ubl::term(lp, gamma, w_c, pw), d = ubl::deriv(lp, gamma), g = ubl::grad(s, pw, w_c, d);
      std::printf("T %a %a %a %a %a | %a %a %a %a %a\n", (double)lp, (double)gamma, (double)w_c, (double)pw, (double)s, (double)q, (double)m,
                  (double)t, (double)d, (double)g);
    }
  struct Case { double loss_sum, weight_sum; uint64_t valid, total; };
  const Case cases[] = {
      {12.5, 3.75, 7, 72},          // an ordinary batch
      {0.0, 0.0, 0, 72},            // nothing contributed: valid and weights have a zero denominator
      {1e-41, 1e-40, 3, 16},        // a weight sum that is an fp32 subnormal: no fp32 reciprocal
      {3.0, 0x1p-126, 1, 16},       // the smallest normal weight sum
      {5.0, 1.0 / 3.0, 16777217, 16777217},   // a pixel count that fp32 rounds
  };
  for (const Case& c : cases)
    for (int mode = UBL_MEAN_PIXELS; mode <= UBL_MEAN_WEIGHTS; ++mode) {
      const ubl::Mean r = ubl::mean(mode, c.loss_sum, c.weight_sum, c.valid, c.total);
      std::printf("M %d %a %a %llu %llu | %a %a %a\n", mode, c.loss_sum, c.weight_sum, (unsigned long long)c.valid, (unsigned long long)c.total,
                  r.denom, (double)r.inv_denom, (double)r.loss);
    }
  return 0;
}
