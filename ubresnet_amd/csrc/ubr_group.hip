// libubresnet_group.so: flat optimizer steps with parameter groups and frozen parameters (include/ubresnet_group.h).  It links
// against none of the other libraries; it shares ubr_sat.h with every satellite source and ubr_opt_rule.h, the step's arithmetic,
// with ubr_opt.hip.  The launches are plain <<<>>> on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include "../../include/ubresnet_group.h"
#include "ubr_group_plan.h"
#include "ubr_opt_rule.h"
#include "ubr_sat.h"

#define UBG_VERSION 1

static_assert(sizeof(ubg_ctl) == UBG_CTL_HEAD_BYTES, "ubg_ctl layout");
static_assert(offsetof(ubg_ctl, norm) == 8 && offsetof(ubg_ctl, apply) == 20 && offsetof(ubg_ctl, bc1) == 28 &&
                  offsetof(ubg_ctl, applied) == 40 && offsetof(ubg_ctl, clipped_total) == 56 && offsetof(ubg_ctl, row) == 64,
              "ubg_ctl layout");
static_assert(sizeof(ubg_tile) == 16 && sizeof(ubg_hyper) == 16 && sizeof(ubg_state) == 16, "16-byte records");
static_assert(UBG_TILE_UNITS == 4 * UBG_BLOCK, "a lane takes four units of a tile");

SAT_RETURN_CODES(UBG);
SAT_EXPORTS(ubg, UBG_VERSION)
using namespace sat;

namespace {

// the block as the kernels see it: the header's fields, then the partials
struct Ctl {
  ubg_ctl h;
  double partial[UBG_MAX_GRID];
};
static_assert(sizeof(Ctl) == UBG_CTL_BYTES, "control block size");

// a tile the kernels may follow: inside the n4 units and of a segment that exists (a table is device memory: the host cannot
// look at it, so the kernels do)
__device__ inline bool tile_ok(const ubg_tile& t, long n4, int nseg) {
  return t.seg >= 0 && t.seg < nseg && t.units >= 1 && t.units <= UBG_TILE_UNITS && t.unit0 >= 0 && t.unit0 <= n4 - t.units;
}

__global__ __launch_bounds__(UBG_BLOCK) void group_state_set_kernel(ubg_state* __restrict__ state, long seg0, long count,
                                                                    const long long* __restrict__ applied,
                                                                    const float* __restrict__ bc_table, long bc_len) {
  for (long i = (long)blockIdx.x * UBG_BLOCK + threadIdx.x; i < count; i += (long)gridDim.x * UBG_BLOCK) {
    const long long a = applied[i] < 0 ? 0 : applied[i];
    ubg_state st;
    st.applied = a;
    st.bc1 = 0.f;
    st.sqrt_bc2 = 0.f;
    if (a > 0) optrule::bc_row(bc_table, bc_len, a, st.bc1, st.sqrt_bc2);
    state[seg0 + i] = st;
  }
}

// Sum of squares of the active segments, first launch: the order is the one include/ubresnet_group.h states.  The tile record
// and the segment's switch are the same for the whole workgroup (uniform reads); the four units of a lane are loaded before
// any is used.  A unit past the tile's end counts as zeros: acc + 0.0 is acc (acc is never -0.0).
__global__ __launch_bounds__(UBG_BLOCK) void group_sumsq_kernel(const float4* __restrict__ g, long n4, const ubg_tile* __restrict__ tiles,
                                                                int ntiles, const ubg_hyper* __restrict__ hyper, int nseg,
                                                                Ctl* __restrict__ ctl) {
  __shared__ double s[UBG_BLOCK];
  double acc = 0.0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const ubg_tile tl = tiles[t];
    if (!tile_ok(tl, n4, nseg)) continue;
    if (hyper[tl.seg].active == 0) continue;
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = (int)threadIdx.x + u * UBG_BLOCK;
      v[u] = i < tl.units ? g[tl.unit0 + i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = optrule::sumsq4(acc, v[u].x, v[u].y, v[u].z, v[u].w);
  }
  optrule::block_tree_sum<UBG_BLOCK>(s, acc);
  if (threadIdx.x == 0) ctl->partial[blockIdx.x] = s[0];
}

// Second launch, one workgroup: lane 0 adds the partials in index order and decides by ubo_grad_norm's rule; if the step
// applies, the lanes then advance the active segments, one segment per lane at a time.  grid == 0 is ubg_advance.
__global__ __launch_bounds__(UBG_BLOCK) void group_decide_kernel(Ctl* __restrict__ ctl, int grid, float grad_scale, float max_norm,
                                                                 int skip_nonfinite, const ubg_hyper* __restrict__ hyper,
                                                                 ubg_state* __restrict__ state, int nseg,
                                                                 const float* __restrict__ bc_table, long bc_len) {
  __shared__ double s[UBG_MAX_GRID];
  __shared__ int s_apply;
  for (int i = threadIdx.x; i < grid; i += UBG_BLOCK) s[i] = ctl->partial[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    double sumsq = 0.0;
    for (int i = 0; i < grid; ++i) sumsq += s[i];
    const optrule::Decision d = optrule::decide(sumsq, grad_scale, max_norm, skip_nonfinite);
    optrule::record(ctl->h, sumsq, d);
    s_apply = d.apply;
  }
  __syncthreads();
  if (!s_apply) return;
  for (int seg = threadIdx.x; seg < nseg; seg += UBG_BLOCK) {
    if (hyper[seg].active == 0) continue;
    ubg_state st = state[seg];
    st.applied += 1;
    optrule::bc_row(bc_table, bc_len, st.applied, st.bc1, st.sqrt_bc2);
    state[seg] = st;
  }
}

// The two step kernels apply the rule of guarded_adam_kernel and guarded_sgd_kernel of libubresnet_opt.so (ubr_opt_rule.h, one
// text for both); what those take as launch arguments or from the control block's head comes from the tile's segment here.  A
// workgroup takes whole tiles; lane l the units l, l + 256, l + 512, l + 768 of a tile, all loaded before the arithmetic.  A
// segment that was never advanced (applied < 1: its bias corrections are zero) is passed over like an inactive one.
__global__ __launch_bounds__(UBG_BLOCK) void group_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, long n4, const ubg_tile* __restrict__ tiles,
                                                               int ntiles, const ubg_hyper* __restrict__ hyper,
                                                               const ubg_state* __restrict__ state, int nseg, float b1, float b2,
                                                               float eps, const ubg_ctl* __restrict__ ctl) {
  if (ctl->apply == 0) return;
  const float gscale = ctl->gscale;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const ubg_tile tl = tiles[t];
    if (!tile_ok(tl, n4, nseg)) continue;
    const ubg_hyper hy = hyper[tl.seg];
    if (hy.active == 0) continue;
    const ubg_state st = state[tl.seg];
    if (st.applied < 1) continue;
    const float lr = hy.lr, wd = hy.weight_decay, sqrt_bc2 = st.sqrt_bc2;
    const float step_size = lr / st.bc1;
    float4 P[4], G[4], M[4], V[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = (int)threadIdx.x + u * UBG_BLOCK;
      if (i < tl.units) {
        const long j = tl.unit0 + i;
        P[u] = reinterpret_cast<float4*>(p)[j];
        G[u] = reinterpret_cast<const float4*>(g)[j];
        M[u] = reinterpret_cast<float4*>(m)[j];
        V[u] = reinterpret_cast<float4*>(v)[j];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = (int)threadIdx.x + u * UBG_BLOCK;
      if (i < tl.units) {
        const long j = tl.unit0 + i;
        float pp[4] = {P[u].x, P[u].y, P[u].z, P[u].w}, gg[4] = {G[u].x, G[u].y, G[u].z, G[u].w};
        float mm[4] = {M[u].x, M[u].y, M[u].z, M[u].w}, vv[4] = {V[u].x, V[u].y, V[u].z, V[u].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) optrule::adam_element(pp[e], gg[e], mm[e], vv[e], gscale, wd, b1, b2, eps, step_size, sqrt_bc2);
        reinterpret_cast<float4*>(p)[j] = make_float4(pp[0], pp[1], pp[2], pp[3]);
        reinterpret_cast<float4*>(m)[j] = make_float4(mm[0], mm[1], mm[2], mm[3]);
        reinterpret_cast<float4*>(v)[j] = make_float4(vv[0], vv[1], vv[2], vv[3]);
      }
    }
  }
}

__global__ __launch_bounds__(UBG_BLOCK) void group_sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                              long n4, const ubg_tile* __restrict__ tiles, int ntiles,
                                                              const ubg_hyper* __restrict__ hyper, const ubg_state* __restrict__ state,
                                                              int nseg, float momentum, float dampening, int nesterov,
                                                              const ubg_ctl* __restrict__ ctl) {
  if (ctl->apply == 0) return;
  const float gscale = ctl->gscale;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const ubg_tile tl = tiles[t];
    if (!tile_ok(tl, n4, nseg)) continue;
    const ubg_hyper hy = hyper[tl.seg];
    if (hy.active == 0) continue;
    const long long applied = state[tl.seg].applied;
    if (applied < 1) continue;
    const int first = applied == 1;
    const float lr = hy.lr, wd = hy.weight_decay;
    float4 P[4], G[4], B[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = (int)threadIdx.x + u * UBG_BLOCK;
      B[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < tl.units) {
        const long j = tl.unit0 + i;
        P[u] = reinterpret_cast<float4*>(p)[j];
        G[u] = reinterpret_cast<const float4*>(g)[j];
        if (buf != nullptr && !first) B[u] = reinterpret_cast<float4*>(buf)[j];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = (int)threadIdx.x + u * UBG_BLOCK;
      if (i < tl.units) {
        const long j = tl.unit0 + i;
        float pp[4] = {P[u].x, P[u].y, P[u].z, P[u].w}, gg[4] = {G[u].x, G[u].y, G[u].z, G[u].w}, bb[4] = {B[u].x, B[u].y, B[u].z, B[u].w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          optrule::sgd_element(pp[e], gg[e], bb[e], gscale, wd, lr, momentum, dampening, buf != nullptr, first, nesterov);
        reinterpret_cast<float4*>(p)[j] = make_float4(pp[0], pp[1], pp[2], pp[3]);
        if (buf != nullptr) reinterpret_cast<float4*>(buf)[j] = make_float4(bb[0], bb[1], bb[2], bb[3]);
      }
    }
  }
}

// the checks every call with segment records and a control block shares; 0 or UBG_EINVAL with the message set
int check_segments(const char* fn, const void* hyper, const void* state, int64_t nseg, const void* ctl) {
  SAT_CHECK(hyper && state && ctl, "%s: null pointer (hyper, state, ctl)", fn);
  SAT_CHECK(nseg >= 1 && nseg <= INT32_MAX, "%s: nseg=%lld must be in [1, 2^31)", fn, (long long)nseg);
  SAT_CHECK(aligned16(hyper) && aligned16(state) && aligned16(ctl), "%s: hyper, state and ctl must be 16-byte aligned", fn);
  const unsigned long long segbytes = 16ull * (unsigned long long)nseg;
  SAT_CHECK(!overlap(ctl, UBG_CTL_BYTES, hyper, segbytes), "%s: ctl overlaps hyper", fn);
  SAT_CHECK(!overlap(ctl, UBG_CTL_BYTES, state, segbytes), "%s: ctl overlaps state", fn);
  SAT_CHECK(!overlap(hyper, segbytes, state, segbytes), "%s: hyper overlaps state", fn);
  return UBG_OK;
}

// and those of a call that also takes a tile table (after check_segments)
int check_tiles(const char* fn, const void* tiles, int64_t ntiles, const void* state, int64_t nseg, const void* ctl) {
  SAT_CHECK(tiles, "%s: null pointer (tiles)", fn);
  SAT_CHECK(ntiles >= 1 && ntiles <= INT32_MAX, "%s: tile table empty or too long (ntiles=%lld)", fn, (long long)ntiles);
  SAT_CHECK(aligned16(tiles), "%s: tiles must be 16-byte aligned", fn);
  SAT_CHECK(!overlap(ctl, UBG_CTL_BYTES, tiles, 16ull * (unsigned long long)ntiles), "%s: ctl overlaps tiles", fn);
  SAT_CHECK(!overlap(state, 16ull * (unsigned long long)nseg, tiles, 16ull * (unsigned long long)ntiles), "%s: state overlaps tiles", fn);
  return UBG_OK;
}

int check_table(const char* fn, const float* bc_table, int64_t bc_len, const void* ctl) {
  SAT_CHECK(bc_table, "%s: null pointer (bc_table)", fn);
  SAT_CHECK(((uintptr_t)bc_table & 7) == 0, "%s: bc_table must be 8-byte aligned", fn);
  SAT_CHECK(bc_len >= 1, "%s: bc_len=%lld must be >= 1", fn, (long long)bc_len);
  SAT_CHECK(!overlap(ctl, UBG_CTL_BYTES, bc_table, 8ull * (unsigned long long)bc_len), "%s: ctl overlaps bc_table", fn);
  return UBG_OK;
}

int check_buffers(const char* fn, int64_t n, const void* const* bufs, const char* const* names, int nbufs, const void* tiles,
                  int64_t ntiles, const void* hyper, const void* state, int64_t nseg, const void* ctl) {
  SAT_CHECK(n > 0 && n % 4 == 0, "%s: n=%lld must be positive and a multiple of 4", fn, (long long)n);
  const unsigned long long bytes = 4ull * (unsigned long long)n;
  for (int i = 0; i < nbufs; ++i) {
    SAT_CHECK(aligned16(bufs[i]), "%s: %s must be 16-byte aligned", fn, names[i]);
    SAT_CHECK(!overlap(ctl, UBG_CTL_BYTES, bufs[i], bytes), "%s: ctl overlaps %s", fn, names[i]);
    SAT_CHECK(!overlap(state, 16ull * (unsigned long long)nseg, bufs[i], bytes), "%s: state overlaps %s", fn, names[i]);
    SAT_CHECK(!overlap(hyper, 16ull * (unsigned long long)nseg, bufs[i], bytes), "%s: hyper overlaps %s", fn, names[i]);
    SAT_CHECK(!overlap(tiles, 16ull * (unsigned long long)ntiles, bufs[i], bytes), "%s: tiles overlap %s", fn, names[i]);
  }
  return UBG_OK;
}

inline unsigned step_grid(int64_t ntiles) { return (unsigned)(ntiles < UBG_STEP_GRID ? ntiles : UBG_STEP_GRID); }

}  // namespace

extern "C" int64_t ubg_plan_tiles(const int64_t* seg_unit0, const int64_t* seg_units, int64_t nseg, ubg_tile* tiles, int64_t cap) {
  int err = 0;
  int64_t bad = -1;
  const int64_t nt = ubg::plan_tiles(seg_unit0, seg_units, nseg, tiles, cap < 0 ? 0 : cap, &err, &bad);
  switch (err) {
    case ubg::PLAN_OK: return nt;
    case ubg::PLAN_NULL: set_error("ubg_plan_tiles: null pointer (seg_unit0, seg_units, tiles)"); break;
    case ubg::PLAN_NSEG: set_error("ubg_plan_tiles: nseg=%lld must be in [1, 2^31)", (long long)nseg); break;
    case ubg::PLAN_UNITS: set_error("ubg_plan_tiles: segment %lld has %lld units; must be >= 1", (long long)bad, (long long)seg_units[bad]); break;
    case ubg::PLAN_ORDER: set_error("ubg_plan_tiles: segment %lld starts at unit %lld, inside or before the segment in front of it", (long long)bad, (long long)seg_unit0[bad]); break;
    default: set_error("ubg_plan_tiles: cap=%lld is too small for %lld tiles", (long long)cap, (long long)nt); break;
  }
  return UBG_EINVAL;
}

extern "C" int ubg_state_set(void* state, int64_t nseg, int64_t seg0, int64_t count, const int64_t* applied, const float* bc_table,
                             int64_t bc_len, void* stream) {
  SAT_CHECK(state && applied, "ubg_state_set: null pointer (state, applied)");
  SAT_CHECK(nseg >= 1 && nseg <= INT32_MAX, "ubg_state_set: nseg=%lld must be in [1, 2^31)", (long long)nseg);
  SAT_CHECK(seg0 >= 0 && count >= 1 && seg0 <= nseg - count, "ubg_state_set: seg out of range: segments %lld .. %lld of %lld",
            (long long)seg0, (long long)(seg0 + count - 1), (long long)nseg);
  SAT_CHECK(aligned16(state) && ((uintptr_t)applied & 7) == 0, "ubg_state_set: state must be 16-byte and applied 8-byte aligned");
  SAT_CHECK(bc_table, "ubg_state_set: null pointer (bc_table)");
  SAT_CHECK(((uintptr_t)bc_table & 7) == 0, "ubg_state_set: bc_table must be 8-byte aligned");
  SAT_CHECK(bc_len >= 1, "ubg_state_set: bc_len=%lld must be >= 1", (long long)bc_len);
  SAT_CHECK(!overlap(state, 16ull * (unsigned long long)nseg, applied, 8ull * (unsigned long long)count), "ubg_state_set: state overlaps applied");
  SAT_CHECK(!overlap(state, 16ull * (unsigned long long)nseg, bc_table, 8ull * (unsigned long long)bc_len), "ubg_state_set: state overlaps bc_table");
  const int64_t blocks = (count + UBG_BLOCK - 1) / UBG_BLOCK;
  group_state_set_kernel<<<dim3((unsigned)(blocks < 64 ? blocks : 64)), dim3(UBG_BLOCK), 0, (hipStream_t)stream>>>(
      (ubg_state*)state, (long)seg0, (long)count, (const long long*)applied, bc_table, (long)bc_len);
  SAT_LAUNCH_CHECK("ubg_state_set");
  return UBG_OK;
}

extern "C" int ubg_state_get(const void* state, int64_t nseg, ubg_state* out, void* stream) {
  SAT_CHECK(state && out, "ubg_state_get: null pointer (state, out)");
  SAT_CHECK(nseg >= 1 && nseg <= INT32_MAX, "ubg_state_get: nseg=%lld must be in [1, 2^31)", (long long)nseg);
  SAT_CHECK(aligned16(state) && ((uintptr_t)out & 7) == 0, "ubg_state_get: state must be 16-byte and out 8-byte aligned");
  hipError_t e = hipMemcpyAsync(out, state, 16ull * (unsigned long long)nseg, hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) {
    set_error("ubg_state_get: copy failed: %s", hipGetErrorString(e));
    return UBG_ELAUNCH;
  }
  return UBG_OK;
}

extern "C" int ubg_grad_norm(const float* grad, int64_t n, const void* tiles, int64_t ntiles, const void* hyper, void* state,
                             int64_t nseg, float grad_scale, float max_norm, int skip_nonfinite, const float* bc_table,
                             int64_t bc_len, void* ctl, void* stream) {
  const char* fn = "ubg_grad_norm";
  SAT_CHECK(grad, "%s: null pointer (grad)", fn);
  if (check_segments(fn, hyper, state, nseg, ctl) || check_tiles(fn, tiles, ntiles, state, nseg, ctl)) return UBG_EINVAL;
  const void* bufs[1] = {grad};
  const char* names[1] = {"grad"};
  if (check_buffers(fn, n, bufs, names, 1, tiles, ntiles, hyper, state, nseg, ctl)) return UBG_EINVAL;
  SAT_CHECK(max_norm == max_norm, "%s: max_norm is NaN", fn);
  if (check_table(fn, bc_table, bc_len, ctl)) return UBG_EINVAL;
  const int grid = (int)(ntiles < UBG_MAX_GRID ? ntiles : UBG_MAX_GRID);
  group_sumsq_kernel<<<dim3((unsigned)grid), dim3(UBG_BLOCK), 0, (hipStream_t)stream>>>(
      (const float4*)grad, (long)(n / 4), (const ubg_tile*)tiles, (int)ntiles, (const ubg_hyper*)hyper, (int)nseg, (Ctl*)ctl);
  SAT_LAUNCH_CHECK("ubg_grad_norm");
  group_decide_kernel<<<dim3(1), dim3(UBG_BLOCK), 0, (hipStream_t)stream>>>((Ctl*)ctl, grid, grad_scale, max_norm, skip_nonfinite ? 1 : 0,
                                                                             (const ubg_hyper*)hyper, (ubg_state*)state, (int)nseg,
                                                                             bc_table, (long)bc_len);
  SAT_LAUNCH_CHECK("ubg_grad_norm");
  return UBG_OK;
}

extern "C" int ubg_advance(const void* hyper, void* state, int64_t nseg, float grad_scale, const float* bc_table, int64_t bc_len,
                           void* ctl, void* stream) {
  const char* fn = "ubg_advance";
  if (check_segments(fn, hyper, state, nseg, ctl)) return UBG_EINVAL;
  if (check_table(fn, bc_table, bc_len, ctl)) return UBG_EINVAL;
  group_decide_kernel<<<dim3(1), dim3(UBG_BLOCK), 0, (hipStream_t)stream>>>((Ctl*)ctl, 0, grad_scale, -1.0f, 0, (const ubg_hyper*)hyper,
                                                                             (ubg_state*)state, (int)nseg, bc_table, (long)bc_len);
  SAT_LAUNCH_CHECK("ubg_advance");
  return UBG_OK;
}

extern "C" int ubg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const void* tiles,
                             int64_t ntiles, const void* hyper, const void* state, int64_t nseg, float beta1, float beta2, float eps,
                             const void* ctl, void* stream) {
  const char* fn = "ubg_adam_step";
  SAT_CHECK(param && grad && exp_avg && exp_avg_sq, "%s: null pointer (param, grad, exp_avg, exp_avg_sq)", fn);
  if (check_segments(fn, hyper, state, nseg, ctl) || check_tiles(fn, tiles, ntiles, state, nseg, ctl)) return UBG_EINVAL;
  const void* bufs[4] = {param, grad, exp_avg, exp_avg_sq};
  const char* names[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
  if (check_buffers(fn, n, bufs, names, 4, tiles, ntiles, hyper, state, nseg, ctl)) return UBG_EINVAL;
  group_adam_kernel<<<dim3(step_grid(ntiles)), dim3(UBG_BLOCK), 0, (hipStream_t)stream>>>(
      param, grad, exp_avg, exp_avg_sq, (long)(n / 4), (const ubg_tile*)tiles, (int)ntiles, (const ubg_hyper*)hyper,
      (const ubg_state*)state, (int)nseg, beta1, beta2, eps, (const ubg_ctl*)ctl);
  SAT_LAUNCH_CHECK("ubg_adam_step");
  return UBG_OK;
}

extern "C" int ubg_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, const void* tiles, int64_t ntiles,
                            const void* hyper, const void* state, int64_t nseg, float momentum, float dampening, int nesterov,
                            const void* ctl, void* stream) {
  const char* fn = "ubg_sgd_step";
  SAT_CHECK(param && grad, "%s: null pointer (param, grad)", fn);
  SAT_CHECK((momentum == 0.f) == (momentum_buf == nullptr), "%s: momentum buffer iff momentum != 0", fn);
  if (check_segments(fn, hyper, state, nseg, ctl) || check_tiles(fn, tiles, ntiles, state, nseg, ctl)) return UBG_EINVAL;
  const void* bufs[3] = {param, grad, momentum_buf};
  const char* names[3] = {"param", "grad", "momentum_buf"};
  if (check_buffers(fn, n, bufs, names, 3, tiles, ntiles, hyper, state, nseg, ctl)) return UBG_EINVAL;
  group_sgd_kernel<<<dim3(step_grid(ntiles)), dim3(UBG_BLOCK), 0, (hipStream_t)stream>>>(
      param, grad, momentum_buf, (long)(n / 4), (const ubg_tile*)tiles, (int)ntiles, (const ubg_hyper*)hyper,
      (const ubg_state*)state, (int)nseg, momentum, dampening, nesterov, (const ubg_ctl*)ctl);
  SAT_LAUNCH_CHECK("ubg_sgd_step");
  return UBG_OK;
}
