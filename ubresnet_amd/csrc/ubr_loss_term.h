// The arithmetic of libubresnet_loss.so (include/ubresnet_loss.h states it) as inline functions that a host compiler takes as
// well: the kernels in ubr_loss.hip call them on the device, tests/loss_host.cpp compiles them into a stand-alone program with the
// host sanitizers on.  Every statement is one fp32 operation or one library call; build with -ffp-contract=off.
#ifndef UBR_LOSS_TERM_H
#define UBR_LOSS_TERM_H

#include <math.h>
#include <stdint.h>
#include "../../include/ubresnet_loss.h"

#if defined(__HIPCC__)
#define UBL_HD __host__ __device__ __forceinline__
#else
#define UBL_HD inline
#endif

namespace ubl {

// q = 1 - p, from expm1f (no cancellation near lp = 0), clamped to [0, 1] by comparisons: a NaN passes through
UBL_HD float miss(float lp) {
  const float x = -expm1f(lp);
  return x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
}

// m = q^gamma
UBL_HD float modulator(float q, float gamma) {
  if (gamma == 0.f) return 1.f;
  if (gamma == 1.f) return q;
  if (gamma == 2.f) return q * q;
  if (q == 0.f) return 0.f;
  const float e = gamma * log2f(q);
  return exp2f(e);
}

// the per-pixel term of the loss sum; at gamma == 0: (-lp * w_c) * pw
UBL_HD float term(float lp, float gamma, float w_c, float pw) {
  const float m = modulator(miss(lp), gamma);
  const float lm = lp * m;
  const float t = -lm * w_c;
  return t * pw;
}

// d term / d lp / (w_c * pw); at gamma == 0 exactly -1 (NaN for a NaN lp)
UBL_HD float deriv(float lp, float gamma) {
  const float q = miss(lp);
  const float m = modulator(q, gamma);
  if (q == 0.f) return -m;
  const float p = expf(lp);
  const float a = gamma * p;
  const float b = lp / q;
  const float c = p == 0.f ? 0.f : a * b;
  const float e = c - 1.f;
  return m * e;
}

// s = g_loss * inv_denom, once per launch; then the products in nll_bwd_kernel's order
UBL_HD float grad(float s, float pw, float w_c, float d) {
  const float a = s * pw;
  const float b = a * w_c;
  return b * d;
}

struct Mean {
  double denom;
  float inv_denom;
  float loss;
};

// the finish rule: total = N*H*W; a zero denominator gives a zero loss and a zero gradient
UBL_HD Mean mean(int mode, double loss_sum, double weight_sum, uint64_t valid, uint64_t total) {
  Mean r;
  r.denom = mode == UBL_MEAN_PIXELS ? (double)total : (mode == UBL_MEAN_VALID ? (double)valid : weight_sum);
  if (r.denom == 0.0) {
    r.inv_denom = 0.f;
    r.loss = 0.f;
    return r;
  }
  const float df = (float)r.denom;
  r.inv_denom = 1.0f / df;
  const double inv = 1.0 / r.denom;
  r.loss = (float)(loss_sum * inv);
  return r;
}

}  // namespace ubl

#endif
