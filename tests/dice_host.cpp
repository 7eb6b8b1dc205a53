// The arithmetic of libubresnet_dice.so (ubresnet_amd/csrc/ubr_dice_term.h, plain C++ for a host compiler) as a stand-alone
// program, so that tests/test_cpu_dice.py can compare it with tests/dice_ref.py without a device:
//   dice_host
// It walks the edge cases of the per-pixel addends and of the finish rule and prints one line per case, every float as a C99
// hexadecimal literal (%a; nan, inf and -inf as such):
//   P lp pw s k | hit lost grad                          hit = pw * expf(lp), lost = pw * q, grad = (s * expf(lp)) * k
//   F live a tp fp fn alpha beta eps | T term k1 k0      ubk::finish_class
#include <cmath>
#include <cstdio>
#include <limits>
#include "ubr_dice_term.h"

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const float lps[] = {0.f, -0.0f, -1e-30f, -1e-45f, -104.f, -110.f, -inf, std::numeric_limits<float>::quiet_NaN(),
                       -1e-3f, -0.6931472f, -5.f, -87.f, -88.5f};
  const float pws[] = {0.5f, 2.f, 1e-40f, 0.f};
  const float s = 0.25f, k = -3.f;
  for (float pw : pws)
    for (float lp : lps)
      std::printf("P %a %a %a %a | %a %a %a\n", (double)lp, (double)pw, (double)s, (double)k, (double)ubk::hit(lp, pw),
                  (double)ubk::lost(lp, pw), (double)ubk::grad(s, lp, k));
  struct Case { int live; double a, tp, fp, fn; float alpha, beta, eps; };
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const Case cases[] = {
      {1, 0.25, 120.5, 30.25, 17.75, 0.5f, 0.5f, 1.f},      // soft Dice
      {1, 0.5, 120.5, 30.25, 17.75, 0.3f, 0.7f, 1e-6f},     // Tversky
      {1, 1.0, 3.0, 2.0, 1.0, 0.f, 1.f, 0.f},
      {1, 1.0, 3.0, 2.0, 1.0, 1.f, 0.f, 0.f},
      {1, 1.0, 3.0, 2.0, 1.0, 0.f, 0.f, 0.f},               // alpha = beta = 0: T = 1, coefficients 0
      {1, 0.5, 0.0, 7.5, 0.0, 0.f, 1.f, 0.f},               // an absent class, alpha = 0, eps = 0: Dn == 0
      {1, 0.5, 0.0, 7.5, 0.0, 0.5f, 0.5f, 0.f},             // an absent class, eps = 0: T = 0
      {1, 0.0, 0.0, 7.5, 0.0, 0.5f, 0.5f, 1.f},             // a = 0: an absent class under present_only, or a zero class weight
      {0, 0.0, 12.0, 7.5, 3.0, 0.5f, 0.5f, 1.f},            // S == 0
      {0, 0.0, nan, 7.5, 3.0, 0.5f, 0.5f, 1.f},             // S == 0 and a NaN sum: still a zero loss
      {1, 0.25, nan, 30.25, 17.75, 0.5f, 0.5f, 1.f},        // a NaN sum
      {1, 0.0, 120.5, nan, 17.75, 0.5f, 0.5f, 1.f},         // a NaN sum in a class of no weight: NaN all the same
      {1, 1.0, 1e-30, 1e-32, 1e-31, 0.5f, 0.5f, 0.f},       // tiny sums without eps: the coefficients are large, not NaN
  };
  for (const Case& c : cases) {
    const ubk::Class r = ubk::finish_class(c.live != 0, c.a, c.tp, c.fp, c.fn, (double)c.alpha, (double)c.beta, (double)c.eps);
    std::printf("F %d %a %a %a %a %a %a %a | %a %a %a %a\n", c.live, c.a, c.tp, c.fp, c.fn, (double)c.alpha, (double)c.beta, (double)c.eps,
                r.T, r.term, (double)r.k1, (double)r.k0);
  }
  return 0;
}
