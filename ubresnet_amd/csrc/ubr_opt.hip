// libubresnet_opt.so: the guarded flat optimizer step (include/ubresnet_opt.h).  It links against none of the other libraries;
// it shares ubr_sat.h with every satellite source and ubr_opt_rule.h, the step's arithmetic, with ubr_group.hip.  The launches
// are plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include "../../include/ubresnet_opt.h"
#include "ubr_opt_rule.h"
#include "ubr_sat.h"

#define UBO_VERSION 1

static_assert(sizeof(ubo_ctl) == UBO_CTL_HEAD_BYTES, "ubo_ctl layout");
static_assert(offsetof(ubo_ctl, norm) == 8 && offsetof(ubo_ctl, apply) == 20 && offsetof(ubo_ctl, bc1) == 28 &&
                  offsetof(ubo_ctl, applied) == 40 && offsetof(ubo_ctl, clipped_total) == 56 && offsetof(ubo_ctl, row) == 64,
              "ubo_ctl layout");

SAT_RETURN_CODES(UBO);
SAT_EXPORTS(ubo, UBO_VERSION)
using namespace sat;

namespace {

// the block as the kernels see it: the header's fields, then the partials
struct Ctl {
  ubo_ctl h;
  double partial[UBO_MAX_GRID];
};
static_assert(sizeof(Ctl) == UBO_CTL_BYTES, "control block size");

__global__ __launch_bounds__(UBO_BLOCK) void ctl_init_kernel(Ctl* ctl, long long applied) {
  double* w = reinterpret_cast<double*>(ctl);
  for (int i = threadIdx.x; i < (int)(UBO_CTL_BYTES / 8); i += UBO_BLOCK)
    w[i] = i == (int)(offsetof(ubo_ctl, applied) / 8) ? __longlong_as_double(applied) : 0.0;
}

// Sum of squares, first launch.  Lane `l` of the grid (l = block * UBO_BLOCK + thread) takes the units l + k * lanes, k = 0, 1,
// ..; UBO_UNROLL of them are loaded before any is used, so a trip of the grid has grid * UBO_BLOCK * UBO_UNROLL * 16 bytes in
// flight.  The lanes of a workgroup are added in a fixed tree in LDS: the partial depends on the data and on n, never on timing.
__global__ __launch_bounds__(UBO_BLOCK) void grad_sumsq_kernel(const float4* __restrict__ g, long n4, Ctl* __restrict__ ctl) {
  __shared__ double s[UBO_BLOCK];
  const long lanes = (long)gridDim.x * UBO_BLOCK;
  double acc = 0.0;
  for (long base = (long)blockIdx.x * UBO_BLOCK + threadIdx.x; base < n4; base += lanes * UBO_UNROLL) {
    float4 v[UBO_UNROLL];
#pragma unroll
    for (int u = 0; u < UBO_UNROLL; ++u) {
      const long i = base + u * lanes;
      v[u] = i < n4 ? g[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < UBO_UNROLL; ++u) acc = optrule::sumsq4(acc, v[u].x, v[u].y, v[u].z, v[u].w);
  }
  optrule::block_tree_sum<UBO_BLOCK>(s, acc);
  if (threadIdx.x == 0) ctl->partial[blockIdx.x] = s[0];
}

// Second launch, one workgroup: the partials come into LDS in parallel, lane 0 adds them in index order and decides.
__global__ __launch_bounds__(UBO_BLOCK) void grad_decide_kernel(Ctl* __restrict__ ctl, int grid, float grad_scale, float max_norm,
                                                                 int skip_nonfinite, const float* __restrict__ bc_table, long bc_len) {
  __shared__ double s[UBO_MAX_GRID];
  for (int i = threadIdx.x; i < grid; i += UBO_BLOCK) s[i] = ctl->partial[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sumsq = 0.0;
  for (int i = 0; i < grid; ++i) sumsq += s[i];
  const optrule::Decision d = optrule::decide(sumsq, grad_scale, max_norm, skip_nonfinite);
  ubo_ctl& h = ctl->h;
  const long long t = h.applied + 1;                         // the count of this step if it applies
  optrule::record(h, sumsq, d);
  if (d.apply) optrule::bc_row(bc_table, bc_len, t, h.bc1, h.sqrt_bc2);
}

// The two step kernels are adam_kernel and sgd_kernel of libubresnet_hip.so (csrc/ubr_head.hip) operation for operation, by the
// element rule of ubr_opt_rule.h; what those take as launch arguments from the host's step count comes from the control block here.
__global__ __launch_bounds__(256) void guarded_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, long n4, float lr, float b1, float b2, float eps,
                                                           float wd, const ubo_ctl* __restrict__ ctl) {
  if (ctl->apply == 0) return;
  const float bc1 = ctl->bc1, sqrt_bc2 = ctl->sqrt_bc2, gscale = ctl->gscale;
  const float step_size = lr / bc1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 P = reinterpret_cast<float4*>(p)[i], G = reinterpret_cast<const float4*>(g)[i];
    float4 M = reinterpret_cast<float4*>(m)[i], V = reinterpret_cast<float4*>(v)[i];
    float pp[4] = {P.x, P.y, P.z, P.w}, gg[4] = {G.x, G.y, G.z, G.w}, mm[4] = {M.x, M.y, M.z, M.w}, vv[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) optrule::adam_element(pp[e], gg[e], mm[e], vv[e], gscale, wd, b1, b2, eps, step_size, sqrt_bc2);
    reinterpret_cast<float4*>(p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
    reinterpret_cast<float4*>(m)[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
    reinterpret_cast<float4*>(v)[i] = make_float4(vv[0], vv[1], vv[2], vv[3]);
  }
}

// This kernel keeps the SGD element written out: with the call to optrule::sgd_element the compiler schedules two independent
// multiplies of the momentum branch the other way round, and no benchmark of tools/ times ubo_sgd_step to show that the same.
// group_sgd_kernel calls the rule and compiles to what it compiled to before; tests/test_gpu_group_exact.py holds the two to
// the same bits.
__global__ __launch_bounds__(256) void guarded_sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                          long n4, float lr, float momentum, float dampening, float wd, int nesterov,
                                                          const ubo_ctl* __restrict__ ctl) {
  if (ctl->apply == 0) return;
  const float gscale = ctl->gscale;
  const int first = ctl->applied == 1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 P = reinterpret_cast<float4*>(p)[i], G = reinterpret_cast<const float4*>(g)[i];
    float4 B = make_float4(0.f, 0.f, 0.f, 0.f);
    if (buf != nullptr && !first) B = reinterpret_cast<float4*>(buf)[i];
    float pp[4] = {P.x, P.y, P.z, P.w}, gg[4] = {G.x, G.y, G.z, G.w}, bb[4] = {B.x, B.y, B.z, B.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {                               // optrule::sgd_element, written out: see the note above
      float gr = fmaf(wd, pp[e], gg[e] * gscale);
      if (buf != nullptr) {
        bb[e] = first ? gr : momentum * bb[e] + (1.f - dampening) * gr;   // torch.optim.SGD: first step clones the gradient
        gr = nesterov ? fmaf(momentum, bb[e], gr) : bb[e];
      }
      pp[e] = pp[e] - lr * gr;
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
    if (buf != nullptr) reinterpret_cast<float4*>(buf)[i] = make_float4(bb[0], bb[1], bb[2], bb[3]);
  }
}

inline int step_blocks(long n4) {
  long b = (n4 + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" int ubo_ctl_init(void* ctl, int64_t applied, void* stream) {
  SAT_CHECK(ctl, "ubo_ctl_init: null ctl");
  SAT_CHECK(aligned16(ctl), "ubo_ctl_init: ctl must be 16-byte aligned");
  SAT_CHECK(applied >= 0, "ubo_ctl_init: applied=%lld must be >= 0", (long long)applied);
  ctl_init_kernel<<<dim3(1), dim3(UBO_BLOCK), 0, (hipStream_t)stream>>>((Ctl*)ctl, (long long)applied);
  SAT_LAUNCH_CHECK("ubo_ctl_init");
  return UBO_OK;
}

extern "C" int ubo_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, int skip_nonfinite,
                             const float* bc_table, int64_t bc_len, void* ctl, void* stream) {
  SAT_CHECK(grad && bc_table && ctl, "ubo_grad_norm: null pointer (grad, bc_table, ctl)");
  SAT_CHECK(n > 0 && n % 4 == 0, "ubo_grad_norm: n=%lld must be positive and a multiple of 4", (long long)n);
  SAT_CHECK(aligned16(grad) && aligned16(ctl), "ubo_grad_norm: grad and ctl must be 16-byte aligned");
  SAT_CHECK(((uintptr_t)bc_table & 7) == 0, "ubo_grad_norm: bc_table must be 8-byte aligned");
  SAT_CHECK(max_norm == max_norm, "ubo_grad_norm: max_norm is NaN");
  SAT_CHECK(bc_len >= 1, "ubo_grad_norm: bc_len=%lld must be >= 1", (long long)bc_len);
  SAT_CHECK(!overlap(ctl, UBO_CTL_BYTES, grad, 4ull * (unsigned long long)n), "ubo_grad_norm: ctl overlaps grad");
  SAT_CHECK(!overlap(ctl, UBO_CTL_BYTES, bc_table, 8ull * (unsigned long long)bc_len), "ubo_grad_norm: ctl overlaps bc_table");
  const long n4 = (long)(n / 4);
  long grid = (n4 + UBO_BLOCK * UBO_UNROLL - 1) / (UBO_BLOCK * UBO_UNROLL);
  if (grid > UBO_MAX_GRID) grid = UBO_MAX_GRID;
  grad_sumsq_kernel<<<dim3((unsigned)grid), dim3(UBO_BLOCK), 0, (hipStream_t)stream>>>((const float4*)grad, n4, (Ctl*)ctl);
  SAT_LAUNCH_CHECK("ubo_grad_norm");
  grad_decide_kernel<<<dim3(1), dim3(UBO_BLOCK), 0, (hipStream_t)stream>>>((Ctl*)ctl, (int)grid, grad_scale, max_norm,
                                                                            skip_nonfinite ? 1 : 0, bc_table, (long)bc_len);
  SAT_LAUNCH_CHECK("ubo_grad_norm");
  return UBO_OK;
}

extern "C" int ubo_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, const void* ctl, void* stream) {
  SAT_CHECK(param && grad && exp_avg && exp_avg_sq && ctl, "ubo_adam_step: null pointer (param, grad, exp_avg, exp_avg_sq, ctl)");
  SAT_CHECK(n > 0 && n % 4 == 0, "ubo_adam_step: n=%lld must be positive and a multiple of 4", (long long)n);
  SAT_CHECK(aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned16(ctl),
            "ubo_adam_step: buffers and ctl must be 16-byte aligned");
  const unsigned long long bytes = 4ull * (unsigned long long)n;
  const void* bufs[4] = {param, grad, exp_avg, exp_avg_sq};
  const char* names[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
  for (int i = 0; i < 4; ++i) SAT_CHECK(!overlap(ctl, UBO_CTL_BYTES, bufs[i], bytes), "ubo_adam_step: ctl overlaps %s", names[i]);
  guarded_adam_kernel<<<dim3(step_blocks((long)(n / 4))), dim3(256), 0, (hipStream_t)stream>>>(
      param, grad, exp_avg, exp_avg_sq, (long)(n / 4), lr, beta1, beta2, eps, weight_decay, (const ubo_ctl*)ctl);
  SAT_LAUNCH_CHECK("ubo_adam_step");
  return UBO_OK;
}

extern "C" int ubo_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                            float weight_decay, int nesterov, const void* ctl, void* stream) {
  SAT_CHECK(param && grad && ctl, "ubo_sgd_step: null pointer (param, grad, ctl)");
  SAT_CHECK(n > 0 && n % 4 == 0, "ubo_sgd_step: n=%lld must be positive and a multiple of 4", (long long)n);
  SAT_CHECK((momentum == 0.f) == (momentum_buf == nullptr), "ubo_sgd_step: momentum buffer iff momentum != 0");
  SAT_CHECK(aligned16(param) && aligned16(grad) && aligned16(momentum_buf) && aligned16(ctl),
            "ubo_sgd_step: buffers and ctl must be 16-byte aligned");
  const unsigned long long bytes = 4ull * (unsigned long long)n;
  const void* bufs[3] = {param, grad, momentum_buf};
  const char* names[3] = {"param", "grad", "momentum_buf"};
  for (int i = 0; i < 3; ++i) SAT_CHECK(!overlap(ctl, UBO_CTL_BYTES, bufs[i], bytes), "ubo_sgd_step: ctl overlaps %s", names[i]);
  guarded_sgd_kernel<<<dim3(step_blocks((long)(n / 4))), dim3(256), 0, (hipStream_t)stream>>>(
      param, grad, momentum_buf, (long)(n / 4), lr, momentum, dampening, weight_decay, nesterov, (const ubo_ctl*)ctl);
  SAT_LAUNCH_CHECK("ubo_sgd_step");
  return UBO_OK;
}
