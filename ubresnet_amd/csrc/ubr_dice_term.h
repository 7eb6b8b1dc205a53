// The arithmetic of libubresnet_dice.so (include/ubresnet_dice.h states it) as inline functions that a host compiler takes as
// well: the kernels in ubr_dice.hip call them on the device, tests/dice_host.cpp compiles them into a stand-alone program.  Every
// fp32 statement is one operation or one library call; build with -ffp-contract=off.
#ifndef UBR_DICE_TERM_H
#define UBR_DICE_TERM_H

#include <math.h>
#include <stdint.h>
#include "../../include/ubresnet_dice.h"

#if defined(__HIPCC__)
#define UBK_HD __host__ __device__ __forceinline__
#else
#define UBK_HD inline
#endif

namespace ubk {

// q = 1 - p, from expm1f (no cancellation near lp = 0), clamped to [0, 1] by comparisons: a NaN passes through
UBK_HD float miss(float lp) {
  const float x = -expm1f(lp);
  return x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
}

// pw * p_c: the addend of TP_t (c == t) or FP_c (c != t)
UBK_HD float hit(float lp, float pw) {
  const float p = expf(lp);
  return pw * p;
}

// pw * q: the addend of FN_t
UBK_HD float lost(float lp_t, float pw) {
  const float q = miss(lp_t);
  return pw * q;
}

// s = g_loss * pw, once per pixel; then times p_c, times the coefficient of the channel
UBK_HD float grad(float s, float lp, float k) {
  const float p = expf(lp);
  const float a = s * p;
  return a * k;
}

struct Class {
  double T;       // the Tversky index
  double term;    // a (1 - T)
  float k1, k0;   // the backward's coefficients
};

// the finish of one class, the sums in fp64: a = classw * present / S; live = S != 0 (otherwise the loss and every coefficient are
// 0 whatever the sums hold)
UBK_HD Class finish_class(bool live, double a, double tp, double fp, double fn, double alpha, double beta, double eps) {
  Class r;
  const double nn = tp + eps;
  const double m = alpha * fp + beta * fn;
  const double dn = tp + m + eps;
  if (dn == 0.0 || !live) {
    r.T = dn == 0.0 ? 1.0 : nn / dn;
    r.term = 0.0;
    r.k1 = 0.f;
    r.k0 = 0.f;
    return r;
  }
  const double d2 = dn * dn;
  r.T = nn / dn;
  r.term = a * (m / dn);
  r.k1 = (float)(-(a * (beta * nn + m)) / d2);
  r.k0 = (float)((a * (alpha * nn)) / d2);
  return r;
}

}  // namespace ubk

#endif
