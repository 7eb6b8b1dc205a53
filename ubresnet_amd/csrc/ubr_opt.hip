// libubresnet_opt.so: the guarded flat optimizer step (include/ubresnet_opt.h).  Self-contained: nothing of the other four
// libraries is linked or included, the launches are plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include "../../include/ubresnet_opt.h"

#define UBO_VERSION 1

static_assert(sizeof(ubo_ctl) == UBO_CTL_HEAD_BYTES, "ubo_ctl layout");
static_assert(offsetof(ubo_ctl, norm) == 8 && offsetof(ubo_ctl, apply) == 20 && offsetof(ubo_ctl, bc1) == 28 &&
                  offsetof(ubo_ctl, applied) == 40 && offsetof(ubo_ctl, clipped_total) == 56 && offsetof(ubo_ctl, row) == 64,
              "ubo_ctl layout");

static thread_local char g_ubo_err[512] = "";

static void ubo_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_ubo_err, sizeof(g_ubo_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* ubo_last_error(void) { return g_ubo_err; }
extern "C" int ubo_version(void) { return UBO_VERSION; }

#define UBO_CHECK(cond, ...)     \
  do {                           \
    if (!(cond)) {               \
      ubo_set_error(__VA_ARGS__);\
      return UBO_EINVAL;         \
    }                            \
  } while (0)

#define UBO_LAUNCH_CHECK(name)                                              \
  do {                                                                      \
    hipError_t e_ = hipGetLastError();                                      \
    if (e_ != hipSuccess) {                                                 \
      ubo_set_error(name ": launch failed: %s", hipGetErrorString(e_));     \
      return UBO_ELAUNCH;                                                   \
    }                                                                       \
  } while (0)

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
// flight.  The square of an fp32 value is exact in fp64 (48 bits of product), so fma(x, x, acc) rounds once, as x * x + acc
// does.  The lanes of a workgroup are added in a fixed tree in LDS: the partial depends on the data and on n, never on timing.
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
    for (int u = 0; u < UBO_UNROLL; ++u) {
      acc = fma((double)v[u].x, (double)v[u].x, acc);
      acc = fma((double)v[u].y, (double)v[u].y, acc);
      acc = fma((double)v[u].z, (double)v[u].z, acc);
      acc = fma((double)v[u].w, (double)v[u].w, acc);
    }
  }
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = UBO_BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
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
  const float norm = (float)(fabs((double)grad_scale) * sqrt(sumsq));
  const float scale = max_norm < 0.f ? 1.0f : fminf(max_norm / (norm + 1e-6f), 1.0f);
  const int apply = !(skip_nonfinite && !isfinite(sumsq));
  const int clipped = apply && scale < 1.0f;
  ubo_ctl& h = ctl->h;
  h.sumsq = sumsq;
  h.norm = norm;
  h.scale = scale;
  h.gscale = grad_scale * scale;
  h.apply = apply;
  h.clipped = clipped;
  if (apply) {
    const long long t = h.applied + 1;
    h.applied = t;
    h.clipped_total += clipped;
    const long row = (t < (long long)bc_len ? (long)t : bc_len) - 1;
    h.bc1 = bc_table[2 * row];
    h.sqrt_bc2 = bc_table[2 * row + 1];
  } else {
    h.skipped += 1;
  }
  h.row[0] = norm;
  h.row[1] = scale;
  h.row[2] = apply ? 1.0f : 0.0f;
  h.row[3] = grad_scale * scale;
}

// The two step kernels are adam_kernel and sgd_kernel of libubresnet_hip.so (csrc/ubr_head.hip) operation for operation; what
// those take as launch arguments from the host's step count comes from the control block here.
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
    for (int e = 0; e < 4; ++e) {
      float gr = gg[e] * gscale;
      gr = fmaf(wd, pp[e], gr);                                  // grad.add(param, alpha=weight_decay)
      mm[e] = mm[e] + (1.f - b1) * (gr - mm[e]);                 // exp_avg.lerp_(grad, 1 - beta1)
      vv[e] = b2 * vv[e] + (1.f - b2) * gr * gr;                 // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
      const float denom = sqrtf(vv[e]) / sqrt_bc2 + eps;
      pp[e] = pp[e] - step_size * (mm[e] / denom);               // param.addcdiv_(exp_avg, denom, value=-step_size)
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
    reinterpret_cast<float4*>(m)[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
    reinterpret_cast<float4*>(v)[i] = make_float4(vv[0], vv[1], vv[2], vv[3]);
  }
}

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
    for (int e = 0; e < 4; ++e) {
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

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline bool overlap(const void* a, unsigned long long abytes, const void* b, unsigned long long bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x != 0 && y != 0 && x < y + bbytes && y < x + abytes;
}

inline int step_blocks(long n4) {
  long b = (n4 + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" int ubo_ctl_init(void* ctl, int64_t applied, void* stream) {
  UBO_CHECK(ctl, "ubo_ctl_init: null ctl");
  UBO_CHECK(aligned16(ctl), "ubo_ctl_init: ctl must be 16-byte aligned");
  UBO_CHECK(applied >= 0, "ubo_ctl_init: applied=%lld must be >= 0", (long long)applied);
  ctl_init_kernel<<<dim3(1), dim3(UBO_BLOCK), 0, (hipStream_t)stream>>>((Ctl*)ctl, (long long)applied);
  UBO_LAUNCH_CHECK("ubo_ctl_init");
  return UBO_OK;
}

extern "C" int ubo_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, int skip_nonfinite,
                             const float* bc_table, int64_t bc_len, void* ctl, void* stream) {
  UBO_CHECK(grad && bc_table && ctl, "ubo_grad_norm: null pointer (grad, bc_table, ctl)");
  UBO_CHECK(n > 0 && n % 4 == 0, "ubo_grad_norm: n=%lld must be positive and a multiple of 4", (long long)n);
  UBO_CHECK(aligned16(grad) && aligned16(ctl), "ubo_grad_norm: grad and ctl must be 16-byte aligned");
  UBO_CHECK(((uintptr_t)bc_table & 7) == 0, "ubo_grad_norm: bc_table must be 8-byte aligned");
  UBO_CHECK(max_norm == max_norm, "ubo_grad_norm: max_norm is NaN");
  UBO_CHECK(bc_len >= 1, "ubo_grad_norm: bc_len=%lld must be >= 1", (long long)bc_len);
  UBO_CHECK(!overlap(ctl, UBO_CTL_BYTES, grad, 4ull * (unsigned long long)n), "ubo_grad_norm: ctl overlaps grad");
  UBO_CHECK(!overlap(ctl, UBO_CTL_BYTES, bc_table, 8ull * (unsigned long long)bc_len), "ubo_grad_norm: ctl overlaps bc_table");
  const long n4 = (long)(n / 4);
  long grid = (n4 + UBO_BLOCK * UBO_UNROLL - 1) / (UBO_BLOCK * UBO_UNROLL);
  if (grid > UBO_MAX_GRID) grid = UBO_MAX_GRID;
  grad_sumsq_kernel<<<dim3((unsigned)grid), dim3(UBO_BLOCK), 0, (hipStream_t)stream>>>((const float4*)grad, n4, (Ctl*)ctl);
  UBO_LAUNCH_CHECK("ubo_grad_norm");
  grad_decide_kernel<<<dim3(1), dim3(UBO_BLOCK), 0, (hipStream_t)stream>>>((Ctl*)ctl, (int)grid, grad_scale, max_norm,
                                                                            skip_nonfinite ? 1 : 0, bc_table, (long)bc_len);
  UBO_LAUNCH_CHECK("ubo_grad_norm");
  return UBO_OK;
}

extern "C" int ubo_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, const void* ctl, void* stream) {
  UBO_CHECK(param && grad && exp_avg && exp_avg_sq && ctl, "ubo_adam_step: null pointer (param, grad, exp_avg, exp_avg_sq, ctl)");
  UBO_CHECK(n > 0 && n % 4 == 0, "ubo_adam_step: n=%lld must be positive and a multiple of 4", (long long)n);
  UBO_CHECK(aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned16(ctl),
            "ubo_adam_step: buffers and ctl must be 16-byte aligned");
  const unsigned long long bytes = 4ull * (unsigned long long)n;
  const void* bufs[4] = {param, grad, exp_avg, exp_avg_sq};
  const char* names[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
  for (int i = 0; i < 4; ++i) UBO_CHECK(!overlap(ctl, UBO_CTL_BYTES, bufs[i], bytes), "ubo_adam_step: ctl overlaps %s", names[i]);
  guarded_adam_kernel<<<dim3(step_blocks((long)(n / 4))), dim3(256), 0, (hipStream_t)stream>>>(
      param, grad, exp_avg, exp_avg_sq, (long)(n / 4), lr, beta1, beta2, eps, weight_decay, (const ubo_ctl*)ctl);
  UBO_LAUNCH_CHECK("ubo_adam_step");
  return UBO_OK;
}

extern "C" int ubo_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                            float weight_decay, int nesterov, const void* ctl, void* stream) {
  UBO_CHECK(param && grad && ctl, "ubo_sgd_step: null pointer (param, grad, ctl)");
  UBO_CHECK(n > 0 && n % 4 == 0, "ubo_sgd_step: n=%lld must be positive and a multiple of 4", (long long)n);
  UBO_CHECK((momentum == 0.f) == (momentum_buf == nullptr), "ubo_sgd_step: momentum buffer iff momentum != 0");
  UBO_CHECK(aligned16(param) && aligned16(grad) && aligned16(momentum_buf) && aligned16(ctl),
            "ubo_sgd_step: buffers and ctl must be 16-byte aligned");
  const unsigned long long bytes = 4ull * (unsigned long long)n;
  const void* bufs[3] = {param, grad, momentum_buf};
  const char* names[3] = {"param", "grad", "momentum_buf"};
  for (int i = 0; i < 3; ++i) UBO_CHECK(!overlap(ctl, UBO_CTL_BYTES, bufs[i], bytes), "ubo_sgd_step: ctl overlaps %s", names[i]);
  guarded_sgd_kernel<<<dim3(step_blocks((long)(n / 4))), dim3(256), 0, (hipStream_t)stream>>>(
      param, grad, momentum_buf, (long)(n / 4), lr, momentum, dampening, weight_decay, nesterov, (const ubo_ctl*)ctl);
  UBO_LAUNCH_CHECK("ubo_sgd_step");
  return UBO_OK;
}
