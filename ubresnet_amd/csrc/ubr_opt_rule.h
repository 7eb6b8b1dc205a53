// The arithmetic of the guarded optimizer step, written once for libubresnet_opt.so (ubr_opt.hip) and libubresnet_group.so
// (ubr_group.hip): the sum of squares, the norm / scale / apply / clipped decision and its record in a control block's head,
// the bias-correction row, and the Adam and SGD updates of one element.  Inline functions that a host compiler takes as well:
// the kernels call them on the device, tests/opt_rule_host.cpp compiles them into a stand-alone program with the host
// sanitizers on.  The order of the floating-point operations is the contract (the sources are compiled with
// -ffp-contract=off): the element updates are adam_kernel and sgd_kernel of libubresnet_hip.so (csrc/ubr_head.hip, which keeps
// its own) operation for operation.  No other header of the project is included here.
#ifndef UBR_OPT_RULE_H
#define UBR_OPT_RULE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define UBO_RULE_HD __host__ __device__ __forceinline__
#else
#define UBO_RULE_HD inline
#endif

namespace optrule {

// Four more squares into a lane's fp64 sum, in this order.  The square of an fp32 value is exact in fp64 (48 bits of product),
// so fma(x, x, acc) rounds once, as x * x + acc does.
UBO_RULE_HD double sumsq4(double acc, float x, float y, float z, float w) {
  acc = fma((double)x, (double)x, acc);
  acc = fma((double)y, (double)y, acc);
  acc = fma((double)z, (double)z, acc);
  acc = fma((double)w, (double)w, acc);
  return acc;
}

#if defined(__HIPCC__)
// The lanes of a workgroup of BLOCK added in a fixed tree in LDS: the sum depends on the addends, never on timing.  Every lane
// of the workgroup calls it; s[0] holds the sum afterwards.
template <int BLOCK>
__device__ __forceinline__ void block_tree_sum(double* s, double acc) {
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
}
#endif

struct Decision {
  float norm, scale, gscale;
  int apply, clipped;
};

// max_norm < 0: no clipping.  fminf: a NaN quotient gives 1.0f.  skip_nonfinite 0: a step with a NaN or infinite sum applies.
UBO_RULE_HD Decision decide(double sumsq, float grad_scale, float max_norm, int skip_nonfinite) {
  const float norm = (float)(fabs((double)grad_scale) * sqrt(sumsq));
  const float scale = max_norm < 0.f ? 1.0f : fminf(max_norm / (norm + 1e-6f), 1.0f);
  const int apply = !(skip_nonfinite && !isfinite(sumsq));
  const int clipped = apply && scale < 1.0f;
  return Decision{norm, scale, grad_scale * scale, apply, clipped};
}

// the decision into a control block's head (ubo_ctl or ubg_ctl: the same fields at the same offsets); each counter moves once
template <typename Head>
UBO_RULE_HD void record(Head& h, double sumsq, const Decision& d) {
  h.sumsq = sumsq;
  h.norm = d.norm;
  h.scale = d.scale;
  h.gscale = d.gscale;
  h.apply = d.apply;
  h.clipped = d.clipped;
  if (d.apply) {
    h.applied += 1;
    h.clipped_total += d.clipped;
  } else {
    h.skipped += 1;
  }
  h.row[0] = d.norm;
  h.row[1] = d.scale;
  h.row[2] = d.apply ? 1.0f : 0.0f;
  h.row[3] = d.gscale;
}

// the bias corrections of applied step t >= 1: row t of the table, its last row past the end
UBO_RULE_HD void bc_row(const float* __restrict__ bc_table, long bc_len, long long t, float& bc1, float& sqrt_bc2) {
  const long row = (t < (long long)bc_len ? (long)t : bc_len) - 1;
  bc1 = bc_table[2 * row];
  sqrt_bc2 = bc_table[2 * row + 1];
}

// torch.optim.Adam's single-tensor step of one element; step_size = lr / bc1
UBO_RULE_HD void adam_element(float& p, float g, float& m, float& v, float gscale, float wd, float b1, float b2, float eps,
                              float step_size, float sqrt_bc2) {
  float gr = g * gscale;
  gr = fmaf(wd, p, gr);                                  // grad.add(param, alpha=weight_decay)
  m = m + (1.f - b1) * (gr - m);                         // exp_avg.lerp_(grad, 1 - beta1)
  v = b2 * v + (1.f - b2) * gr * gr;                     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  const float denom = sqrtf(v) / sqrt_bc2 + eps;
  p = p - step_size * (m / denom);                       // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// torch.optim.SGD's; has_buf: there is a momentum buffer (b is it, and is written), first: this is the first applied step
UBO_RULE_HD void sgd_element(float& p, float g, float& b, float gscale, float wd, float lr, float momentum, float dampening,
                             bool has_buf, int first, int nesterov) {
  float gr = fmaf(wd, p, g * gscale);
  if (has_buf) {
    b = first ? gr : momentum * b + (1.f - dampening) * gr;      // torch.optim.SGD: first step clones the gradient
    gr = nesterov ? fmaf(momentum, b, gr) : b;
  }
  p = p - lr * gr;
}

}  // namespace optrule

#endif
