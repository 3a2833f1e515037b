// gbnf_image_boost.hip -- boosting for IMAGE components on the device (gfx950): the image counterparts of gbnf_mixture_rho_step and
// gbnf_boosted_nll_step (gbnf_boost.hip).
//
//   gbnf_image_mixture_rho_step   one iteration of update_rho (models/boosted_flow.py:119-207, approximate branch): the components'
//                                 forwards one after another on the caller's stream, then the rho update shared with the tabular call
//   gbnf_image_mixture_rho_step_y the same over class-conditional components: every forward under its prior of each row's y
//   g_partial_kernel              per-workgroup sums of -max(ll_G, g_floor) and the count of rows below the floor or non-finite
//   g_finalize_kernel             G_nll = their mean (image_experiment.py:252-254), the count
//   boosted_stat_kernel           stats[5] = stats[0] - stats[4]: the reference's nll = g_nll - G_nll (:256)
//
// Launch-latency sized like the kernels of gbnf_boost.hip: no matrix pipe, no LDS opt-in.  The reductions run in f64 in an order that
// depends on the sizes alone -- no atomics --, so the statistics are bit-identical from run to run for the same log-likelihoods.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gbnf.h"
#include "gbnf_image_train.h"
#include "gbnf_internal.h"
#include "gbnf_opt.h"

namespace gbnf {

constexpr int G_THREADS = 256;
constexpr int G_MAX_PARTIALS = 256;
static_assert(G_MAX_PARTIALS <= G_THREADS, "the finalise kernel re-adds the partial sums one per thread");

static int64_t iboost_align256(int64_t b) { return (b + 255) / 256 * 256; }

// the workgroup's 256 values added up in a fixed tree order; every thread gets the sum
__device__ __forceinline__ double g_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = G_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

// part_sum[b] = sum over this workgroup's rows of -max(ll_i, g_floor) with torch.max's semantics (a NaN ll stays NaN; g_floor = -inf:
// no clamp);  part_bad[b] = rows with ll_i < g_floor or a non-finite ll_i
__global__ void __launch_bounds__(G_THREADS) g_partial_kernel(const float* __restrict__ ll, int64_t n, float g_floor,
                                                              double* __restrict__ part_sum, double* __restrict__ part_bad) {
  __shared__ double lds[G_THREADS];
  const int64_t stride = (int64_t)gridDim.x * G_THREADS;
  double acc = 0.0, bad = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * G_THREADS + threadIdx.x; i < n; i += stride) {
    const float v = ll[i];
    const float m = v < g_floor ? g_floor : v;       // (a NaN compares false: it is kept)
    acc -= (double)m;
    if (v < g_floor || !(fabsf(v) < INFINITY)) bad += 1.0;
  }
  const double s = g_block_sum(acc, lds);
  const double b = g_block_sum(bad, lds);
  if (threadIdx.x == 0) { part_sum[blockIdx.x] = s; part_bad[blockIdx.x] = b; }
}

// stats[4] = G_nll = mean_i(-max(ll_i, g_floor)), stats[6] = the row count, stats[7] = 0
__global__ void __launch_bounds__(G_THREADS) g_finalize_kernel(const double* __restrict__ part_sum, const double* __restrict__ part_bad,
                                                               int n_partial, int64_t n, float* __restrict__ stats) {
  __shared__ double lds[G_THREADS];
  const int tid = threadIdx.x;
  const double s = g_block_sum(tid < n_partial ? part_sum[tid] : 0.0, lds);
  const double b = g_block_sum(tid < n_partial ? part_bad[tid] : 0.0, lds);
  if (tid != 0) return;
  stats[4] = (float)(s / (double)n);
  stats[6] = (float)b;
  stats[7] = 0.0f;
}

// behind the trained component's step: the reference's nll = g_nll - G_nll (unscaled, in nats)
// (g: where the G term's three floats start: 4, or 8 in the class-conditional call's 12-float layout)
__global__ void boosted_stat_kernel(float* __restrict__ stats, int g) {
  if (threadIdx.x == 0 && blockIdx.x == 0) stats[g + 1] = stats[0] - stats[g];
}

// the caller's workspace of one boosted image step, in 256-byte aligned pieces
struct ImageBoostLayout {
  int64_t step, step_bytes, flow, flow_bytes, ldj, ll, part, total;
};

static int image_boost_layout(const gbnf_image_flow* fixed, const gbnf_image_trainer* t, int64_t n, ImageBoostLayout* L) {
  int64_t step_bytes = 0, flow_bytes = 0;
  if (const int rc = gbnf_image_trainer_step_workspace_bytes(t, n, &step_bytes)) return rc;
  if (const int rc = gbnf_image_flow_workspace_bytes(fixed, n, &flow_bytes)) return rc;
  const int64_t nn = iboost_align256(n * 4);
  int64_t off = 0;
  L->step = off; L->step_bytes = step_bytes; off += iboost_align256(step_bytes);
  L->flow = off; L->flow_bytes = flow_bytes; off += iboost_align256(flow_bytes);
  L->ldj = off; off += nn;
  L->ll = off; off += nn;
  L->part = off; off += iboost_align256(2 * G_MAX_PARTIALS * (int64_t)sizeof(double));
  L->total = off;
  return GBNF_OK;
}

// the fixed component and the trainer must see the same images
static int check_fixed_image(const char* fn, const gbnf_image_flow* fixed, const gbnf_image_trainer* t) {
  if (!fixed) return fail(GBNF_ERR_INVALID, "%s: fixed is null", fn);
  if (!t) return fail(GBNF_ERR_INVALID, "%s: trainer is null", fn);
  int C = 0, H = 0, W = 0;
  if (const int rc = image_flow_input_shape(fixed, &C, &H, &W)) return rc;
  if (C != t->C || H != t->Hi || W != t->Wi)
    return fail(GBNF_ERR_INVALID, "%s: the fixed component takes %d x %d x %d images, the trainer %d x %d x %d", fn, C, H, W, t->C, t->Hi,
                t->Wi);
  return GBNF_OK;
}

// handles [0, n_flows) are non-null and take images of one shape  (gbnf_internal.h: shared with gbnf_eval.hip)
int check_image_flows(const char* fn, const gbnf_image_flow* const* flows, int n_flows) {
  int C0 = 0, H0 = 0, W0 = 0;
  for (int c = 0; c < n_flows; ++c) {
    if (!flows[c]) return fail(GBNF_ERR_INVALID, "%s: flows[%d] is null", fn, c);
    int C = 0, H = 0, W = 0;
    if (const int rc = image_flow_input_shape(flows[c], &C, &H, &W)) return rc;
    if (c == 0) { C0 = C; H0 = H; W0 = W; }
    else if (C != C0 || H != H0 || W != W0)
      return fail(GBNF_ERR_INVALID, "%s: flows[%d] takes %d x %d x %d images, flows[0] %d x %d x %d", fn, c, C, H, W, C0, H0, W0);
  }
  return GBNF_OK;
}

// with_y false: every handle is plain;  true: every handle is conditioned, all on one class count (*y_classes_out, may be null)
// (gbnf_internal.h: shared with gbnf_eval.hip)
int check_image_flows_y(const char* fn, const gbnf_image_flow* const* flows, int n_flows, bool with_y, int32_t* y_classes_out) {
  int32_t Y0 = 0;
  for (int c = 0; c < n_flows; ++c) {
    int32_t y_classes = 0;
    if (const int rc = gbnf_image_flow_y_classes(flows[c], &y_classes)) return rc;
    if (!with_y) {
      if (y_classes != 0)
        return fail(GBNF_ERR_INVALID, "%s: flows[%d] is class-conditional (%d classes) and needs y: this call takes none (the _y call does)", fn,
                    c, (int)y_classes);
      continue;
    }
    if (y_classes == 0) return fail(GBNF_ERR_INVALID, "%s: flows[%d] has no conditioning set (gbnf_image_flow_set_ycond)", fn, c);
    if (c == 0) Y0 = y_classes;
    else if (y_classes != Y0)
      return fail(GBNF_ERR_INVALID, "%s: flows[%d] has %d classes, flows[0] %d: y has one width", fn, c, (int)y_classes, (int)Y0);
  }
  if (y_classes_out) *y_classes_out = Y0;
  return GBNF_OK;
}

static int image_rho_layout(const gbnf_image_flow* const* flows, int n_flows, int64_t n, int64_t* flow_bytes, int64_t* total) {
  int64_t worst = 0;
  for (int c = 0; c < n_flows; ++c) {
    int64_t b = 0;
    if (const int rc = gbnf_image_flow_workspace_bytes(flows[c], n, &b)) return rc;
    if (b > worst) worst = b;
  }
  *flow_bytes = iboost_align256(worst);
  *total = *flow_bytes + iboost_align256(n * 4);
  return GBNF_OK;
}

}  // namespace gbnf

using namespace gbnf;

extern "C" {

int gbnf_image_rho_step_workspace_bytes(const gbnf_image_flow* const* flows, int32_t n_flows, int64_t n, int64_t* bytes) {
  const char* fn = "gbnf_image_rho_step_workspace_bytes";
  if (!flows || !bytes) return fail(GBNF_ERR_INVALID, "%s: flows / bytes is null", fn);
  if (n_flows < 1 || n < 1) return fail(GBNF_ERR_INVALID, "%s: n_flows = %d, n = %lld (both must be >= 1)", fn, (int)n_flows, (long long)n);
  if (const int rc = check_image_flows(fn, flows, n_flows)) return rc;
  int64_t flow_bytes = 0;
  return image_rho_layout(flows, n_flows, n, &flow_bytes, bytes);
}

// gbnf_image_mixture_rho_step (y null: every handle plain) and gbnf_image_mixture_rho_step_y (y (n, Y): every handle conditioned, one Y)
static int image_rho_step(const char* fn, const gbnf_image_flow* const* flows, int32_t component, const float* x, const float* noise,
                          const float* y, bool with_y, int64_t n, float* rho_dev, float step_size, float* ll_workspace, float* stats_dev,
                          void* workspace, int64_t workspace_bytes, void* stream) {
  if (!flows || !x || !rho_dev || !ll_workspace || !stats_dev || !workspace || (with_y && !y))
    return fail(GBNF_ERR_INVALID, "%s: flows / x / %srho_dev / ll_workspace / stats_dev / workspace is null", fn, with_y ? "y / " : "");
  if (component < 1) return fail(GBNF_ERR_INVALID, "%s: component = %d (must be >= 1: component 0 has no weight to learn)", fn, (int)component);
  if (n < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld (must be >= 1)", fn, (long long)n);
  const int n_flows = (int)component + 1;
  if (const int rc = check_image_flows(fn, flows, n_flows)) return rc;
  if (const int rc = check_image_flows_y(fn, flows, n_flows, with_y, nullptr)) return rc;    // refused HERE, before the first component's launches
  int64_t flow_bytes = 0, total = 0;
  if (const int rc = image_rho_layout(flows, n_flows, n, &flow_bytes, &total)) return rc;
  if (workspace_bytes < total)
    return fail(GBNF_ERR_INVALID, "%s: workspace of %lld bytes < %lld (gbnf_image_rho_step_workspace_bytes)", fn, (long long)workspace_bytes,
                (long long)total);
  float* ldj = (float*)((char*)workspace + flow_bytes);
  for (int c = 0; c < n_flows; ++c) {    // one chain after the other on the caller's stream: they share the workspace
    float* ll = ll_workspace + (int64_t)c * n;
    const int rc = with_y ? gbnf_image_flow_forward_y(flows[c], x, noise, y, n, nullptr, ldj, ll, nullptr, workspace, flow_bytes, stream)
                          : gbnf_image_flow_forward(flows[c], x, noise, n, nullptr, ldj, ll, workspace, flow_bytes, stream);
    if (rc) return rc;
  }
  return rho_update_launch(fn, ll_workspace, n, (int)component, rho_dev, step_size, stats_dev, (hipStream_t)stream);
}

int gbnf_image_mixture_rho_step(const gbnf_image_flow* const* flows, int32_t component, const float* x, const float* noise, int64_t n,
                                float* rho_dev, float step_size, float* ll_workspace, float* stats_dev, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  return image_rho_step("gbnf_image_mixture_rho_step", flows, component, x, noise, nullptr, false, n, rho_dev, step_size, ll_workspace,
                        stats_dev, workspace, workspace_bytes, stream);
}

int gbnf_image_mixture_rho_step_y(const gbnf_image_flow* const* flows, int32_t component, const float* x, const float* noise, const float* y,
                                  int64_t n, float* rho_dev, float step_size, float* ll_workspace, float* stats_dev, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  return image_rho_step("gbnf_image_mixture_rho_step_y", flows, component, x, noise, y, true, n, rho_dev, step_size, ll_workspace,
                        stats_dev, workspace, workspace_bytes, stream);
}

int gbnf_image_boosted_step_workspace_bytes(const gbnf_image_flow* fixed, const gbnf_image_trainer* trainer, int64_t n, int64_t* bytes) {
  const char* fn = "gbnf_image_boosted_step_workspace_bytes";
  if (!bytes || n < 1) return fail(GBNF_ERR_INVALID, "%s: bad argument", fn);
  if (const int rc = check_fixed_image(fn, fixed, trainer)) return rc;
  ImageBoostLayout L;
  if (const int rc = image_boost_layout(fixed, trainer, n, &L)) return rc;
  *bytes = L.total;
  return GBNF_OK;
}

// the plain call (y null) and the class-conditional one (y (n, Y): the fixed component through gbnf_image_flow_forward_y, the step
// through gbnf_image_trainer_nll_step_y, the G term's floats at stats[8..10])
static int image_boosted_step(const char* fn, const gbnf_image_flow* fixed, float g_floor, gbnf_image_trainer* trainer, const float* x,
                              const float* noise, const float* y, bool want_y, int64_t n, float loss_scale, float y_weight, float* grads,
                              float* exp_avg, float* exp_avg_sq, const gbnf_opt_hyper* hyper, float* stats_dev, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  // everything gbnf_image_trainer_nll_step refuses is refused HERE, before the fixed component's launches
  if (!trainer || !x || !grads || !stats_dev || !workspace)
    return fail(GBNF_ERR_INVALID, "%s: trainer / x / grads / stats_dev / workspace is null", fn);
  if (want_y && !y) return fail(GBNF_ERR_INVALID, "%s: y is null", fn);
  if (n < 1 || n > 65535) return fail(GBNF_ERR_INVALID, "%s: n = %lld (1 to 65535 images per call)", fn, (long long)n);
  int64_t step_floats = 0;
  if (const int rc = gbnf_image_trainer_step_grad_floats(trainer, &step_floats)) return rc;      // (a failed bind call)
  int32_t y_trainer = 0, y_fixed = 0;
  if (const int rc = gbnf_image_trainer_y_classes(trainer, &y_trainer)) return rc;
  if (const int rc = fixed ? gbnf_image_flow_y_classes(fixed, &y_fixed) : GBNF_OK) return rc;
  if (want_y ? (y_trainer < 1 || y_fixed != y_trainer) : (y_trainer != 0 || y_fixed != 0))
    return fail(GBNF_ERR_INVALID, "%s: the trainer has %d classes bound, the fixed component %d: %s", fn, (int)y_trainer, (int)y_fixed,
                want_y ? "both must be conditioned on the same classes" : "class-conditional components need y (the _y call)");
  if (const int rc = check_hyper(fn, hyper, exp_avg, exp_avg_sq)) return rc;
  if (const int rc = check_fixed_image(fn, fixed, trainer)) return rc;
  ImageBoostLayout L;
  if (const int rc = image_boost_layout(fixed, trainer, n, &L)) return rc;
  if (workspace_bytes < L.total)
    return fail(GBNF_ERR_INVALID, "%s: workspace too small: %lld bytes < %lld (gbnf_image_boosted_step_workspace_bytes)", fn,
                (long long)workspace_bytes, (long long)L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* ldj = (float*)(ws + L.ldj);
  float* ll = (float*)(ws + L.ll);
  double* part_sum = (double*)(ws + L.part);
  double* part_bad = part_sum + G_MAX_PARTIALS;
  int rc = want_y ? gbnf_image_flow_forward_y(fixed, x, noise, y, n, nullptr, ldj, ll, nullptr, ws + L.flow, L.flow_bytes, stream)
                  : gbnf_image_flow_forward(fixed, x, noise, n, nullptr, ldj, ll, ws + L.flow, L.flow_bytes, stream);
  if (rc) return rc;
  const int g_at = want_y ? 8 : 4;
  int64_t nb = (n + 4 * G_THREADS - 1) / (4 * G_THREADS);
  if (nb > G_MAX_PARTIALS) nb = G_MAX_PARTIALS;
  hipLaunchKernelGGL(g_partial_kernel, dim3((unsigned)nb), dim3(G_THREADS), 0, s, (const float*)ll, n, g_floor, part_sum, part_bad);
  hipLaunchKernelGGL(g_finalize_kernel, dim3(1), dim3(G_THREADS), 0, s, (const double*)part_sum, (const double*)part_bad, (int)nb, n,
                     stats_dev + (g_at - 4));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  rc = want_y ? gbnf_image_trainer_nll_step_y(trainer, x, noise, y, n, loss_scale, y_weight, grads, exp_avg, exp_avg_sq, hyper, stats_dev,
                                              ws + L.step, L.step_bytes, stream)
              : gbnf_image_trainer_nll_step(trainer, x, noise, n, loss_scale, grads, exp_avg, exp_avg_sq, hyper, stats_dev, ws + L.step,
                                            L.step_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(boosted_stat_kernel, dim3(1), dim3(64), 0, s, stats_dev, g_at);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

int gbnf_image_boosted_nll_step(const gbnf_image_flow* fixed, float g_floor, gbnf_image_trainer* trainer, const float* x, const float* noise,
                                int64_t n, float loss_scale, float* grads, float* exp_avg, float* exp_avg_sq, const gbnf_opt_hyper* hyper,
                                float* stats_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  return image_boosted_step("gbnf_image_boosted_nll_step", fixed, g_floor, trainer, x, noise, nullptr, false, n, loss_scale, 0.0f, grads,
                            exp_avg, exp_avg_sq, hyper, stats_dev, workspace, workspace_bytes, stream);
}

int gbnf_image_boosted_step_workspace_bytes_y(const gbnf_image_flow* fixed, const gbnf_image_trainer* trainer, int64_t n, int64_t* bytes) {
  const char* fn = "gbnf_image_boosted_step_workspace_bytes_y";
  if (!bytes || n < 1) return fail(GBNF_ERR_INVALID, "%s: bad argument", fn);
  if (const int rc = check_fixed_image(fn, fixed, trainer)) return rc;
  int32_t y_trainer = 0, y_fixed = 0;
  if (const int rc = gbnf_image_trainer_y_classes(trainer, &y_trainer)) return rc;
  if (const int rc = gbnf_image_flow_y_classes(fixed, &y_fixed)) return rc;
  if (y_trainer < 1 || y_fixed != y_trainer)
    return fail(GBNF_ERR_INVALID, "%s: the trainer has %d classes bound, the fixed component %d", fn, (int)y_trainer, (int)y_fixed);
  ImageBoostLayout L;
  if (const int rc = image_boost_layout(fixed, trainer, n, &L)) return rc;
  *bytes = L.total;
  return GBNF_OK;
}

int gbnf_image_boosted_nll_step_y(const gbnf_image_flow* fixed, float g_floor, gbnf_image_trainer* trainer, const float* x, const float* noise,
                                  const float* y, int64_t n, float loss_scale, float y_weight, float* grads, float* exp_avg,
                                  float* exp_avg_sq, const gbnf_opt_hyper* hyper, float* stats_dev, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  return image_boosted_step("gbnf_image_boosted_nll_step_y", fixed, g_floor, trainer, x, noise, y, true, n, loss_scale, y_weight, grads,
                            exp_avg, exp_avg_sq, hyper, stats_dev, workspace, workspace_bytes, stream);
}

}  // extern "C"
