// gbnf_eval.hip -- the validation pass of both training drivers on the device (gfx950): what `evaluate(model, loader, args)` of
// density_experiment.py:544-603 and image_experiment.py:296-337 does in eager PyTorch with a host read per batch (or a cat over the
// whole set), as running sums in a caller-owned DEVICE state that is read once after the last batch.
//
//   eval_partial_kernel        per-workgroup sums over a (n_used, n) log-likelihood table: G_ll (the recursion of mixture_lse_kernel,
//                              bit for bit), g_ll = ll[component], G_ll - g_ll, E_ll = sum_c w_c ll_c, and the non-finite rows
//   eval_finalize_kernel       the partials re-added in index order and ADDED into the 16 doubles of the state
//   class_loss_partial_kernel  per-workgroup sums of one component's cross-entropy and correct predictions (image_experiment.py:236)
//   class_loss_finalize_kernel those, weighted with the component's w_c, added into entries 10 - 12 of the state
//
// Launch-latency sized like the kernels of gbnf_boost.hip: no matrix pipe, no LDS opt-in.  Every sum runs in f64 in an order that
// depends on the sizes alone -- an LDS tree per workgroup, then the partials in index order, no atomics --, so the state is
// bit-identical from run to run for the same tables.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gbnf.h"
#include "gbnf_internal.h"

namespace gbnf {

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_ROWS_PER_WG = 4 * EVAL_THREADS;     // rows a workgroup takes before the grid-stride loop wraps (as rho_update_launch)
constexpr int EVAL_MAX_PARTIALS = 256;
constexpr int EVAL_SUMS = 5;                            // G, g, G - g, E, non-finite rows  (the class loss uses the first two)
constexpr int64_t EVAL_WORKSPACE_BYTES = (int64_t)EVAL_SUMS * EVAL_MAX_PARTIALS * sizeof(double);
static_assert(GBNF_EVAL_STATE_DOUBLES >= 13, "the finalise kernels write entries 0 - 12 of the state");
static_assert(EVAL_WORKSPACE_BYTES % 256 == 0, "the image call lays its pieces out in 256-byte steps");

static int64_t eval_align256(int64_t b) { return (b + 255) / 256 * 256; }

// the workgroup's 256 values added up in a fixed tree order; every thread gets the sum
__device__ __forceinline__ double eval_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = EVAL_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

// sum_{k < n_used} rho[k] in double, in index order: the denominator of w_c
__device__ __forceinline__ double rho_total(const float* __restrict__ rho, int n_used) {
  double t = 0.0;
  for (int k = 0; k < n_used; ++k) t = __dadd_rn(t, (double)rho[k]);
  return t;
}

// Row i of the table:  G = the mixture recursion (float32, mixture_lse_kernel's operations);  g = ll[component][i];  G - g in float32, as
// the reference forms g_nll - G_nll (density_experiment.py:588);  E = sum_c (rho[c] / sum rho) * ll[c][i] in double, index order, every
// product and sum rounded on its own (no fused multiply-add: the value is that of the same expression in any IEEE double arithmetic).
// partial[k * EVAL_MAX_PARTIALS + b] = workgroup b's sum of quantity k;  k = 4 counts the rows where G, g or E is not finite (they are
// still added: a NaN reaches the mean as it does in the reference).
__global__ void __launch_bounds__(EVAL_THREADS) eval_partial_kernel(const float* __restrict__ ll, int64_t stride, int n_used, int64_t n,
                                                                    const float* __restrict__ rho, int component, float* __restrict__ G_out,
                                                                    double* __restrict__ partial) {
  __shared__ double lds[EVAL_THREADS];
  const int64_t step = (int64_t)gridDim.x * EVAL_THREADS;
  const double total = rho_total(rho, n_used);
  double sG = 0.0, sg = 0.0, sd = 0.0, sE = 0.0, bad = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * EVAL_THREADS + threadIdx.x; i < n; i += step) {
    const float G = mixture_lse_row(ll, stride, rho, n_used, i);
    const float g = ll[(int64_t)component * stride + i];
    double E = 0.0;
    for (int c = 0; c < n_used; ++c)
      E = __dadd_rn(E, __dmul_rn((double)rho[c] / total, (double)ll[(int64_t)c * stride + i]));
    if (G_out != nullptr) G_out[i] = G;
    sG += (double)G;
    sg += (double)g;
    sd += (double)(G - g);
    sE += E;
    if (!(fabsf(G) < INFINITY) || !(fabsf(g) < INFINITY) || !(fabs(E) < (double)INFINITY)) bad += 1.0;
  }
  const double v[EVAL_SUMS] = {sG, sg, sd, sE, bad};
#pragma unroll
  for (int k = 0; k < EVAL_SUMS; ++k) {
    const double s = eval_block_sum(v[k], lds);
    if (threadIdx.x == 0) partial[k * EVAL_MAX_PARTIALS + blockIdx.x] = s;
  }
}

// One wave.  Lane k < 5 adds quantity k's partials in index order and adds the result into the state (include/gbnf.h has the layout):
// no two lanes write the same entry.
__global__ void __launch_bounds__(64) eval_finalize_kernel(const double* __restrict__ partial, int n_partial, int64_t n,
                                                           double* __restrict__ state) {
  const int k = threadIdx.x;
  if (k >= EVAL_SUMS) return;
  double s = 0.0;
  for (int b = 0; b < n_partial; ++b) s += partial[k * EVAL_MAX_PARTIALS + b];
  const double rows = (double)n;
  if (k == 0) { state[2] += s; state[6] += s / rows; }             // G_ll
  else if (k == 1) { state[3] += s; state[7] += s / rows; }        // g_ll
  else if (k == 2) { state[4] += s; }                              // G_ll - g_ll
  else if (k == 3) { state[5] += s; state[8] += s / rows; }        // E_ll
  else { state[9] += s; state[0] += rows; state[1] += 1.0; }       // non-finite rows; rows and batches seen
}

// Row i:  t = the first largest entry of y_i, p = the first largest logit (a NaN never wins either; a row of NaNs gives 0);
// CE = LSE(logits_i) - logits_i[t] in double with torch.logsumexp's semantics (an infinite maximum is replaced by 0, a NaN logit makes
// the sum NaN), the exponentials added in index order.  One thread per row: Y <= 256 and a batch of images is a few hundred rows.
// partial[b] = workgroup b's sum of CE, partial[EVAL_MAX_PARTIALS + b] = its rows with p == t.
__global__ void __launch_bounds__(EVAL_THREADS) class_loss_partial_kernel(const float* __restrict__ logits, const float* __restrict__ y,
                                                                          int64_t n, int Y, double* __restrict__ partial) {
  __shared__ double lds[EVAL_THREADS];
  const int64_t step = (int64_t)gridDim.x * EVAL_THREADS;
  double sce = 0.0, hit = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * EVAL_THREADS + threadIdx.x; i < n; i += step) {
    const float* __restrict__ lr = logits + i * Y;
    const float* __restrict__ yr = y + i * Y;
    int t = 0, p = 0;
    float ybest = -INFINITY, lbest = -INFINITY;
    for (int k = 0; k < Y; ++k) {
      if (yr[k] > ybest) { ybest = yr[k]; t = k; }
      if (lr[k] > lbest) { lbest = lr[k]; p = k; }
    }
    double m = (double)lbest;                        // (the largest non-NaN logit, -inf if there is none)
    if (isinf(m)) m = 0.0;
    double s = 0.0;
    for (int k = 0; k < Y; ++k) s = __dadd_rn(s, exp((double)lr[k] - m));
    sce += __dadd_rn(__dadd_rn(m, log(s)), -(double)lr[t]);
    if (p == t) hit += 1.0;
  }
  const double a = eval_block_sum(sce, lds);
  const double b = eval_block_sum(hit, lds);
  if (threadIdx.x == 0) { partial[blockIdx.x] = a; partial[EVAL_MAX_PARTIALS + blockIdx.x] = b; }
}

// One wave.  w = rho[c] / sum_{k < n_used} rho[k];  lane 0: state[10] += w S_CE, state[11] += w (S_CE / n);  lane 1: state[12] += w S_hit
__global__ void __launch_bounds__(64) class_loss_finalize_kernel(const double* __restrict__ partial, int n_partial, int64_t n,
                                                                 const float* __restrict__ rho, int n_used, int c,
                                                                 double* __restrict__ state) {
  const int k = threadIdx.x;
  if (k >= 2) return;
  double s = 0.0;
  for (int b = 0; b < n_partial; ++b) s += partial[k * EVAL_MAX_PARTIALS + b];
  const double w = (double)rho[c] / rho_total(rho, n_used);
  if (k == 0) { state[10] += w * s; state[11] += w * (s / (double)n); }
  else state[12] += w * s;
}

static unsigned eval_grid(int64_t n) {
  int64_t nb = (n + EVAL_ROWS_PER_WG - 1) / EVAL_ROWS_PER_WG;
  if (nb > EVAL_MAX_PARTIALS) nb = EVAL_MAX_PARTIALS;
  return (unsigned)nb;
}

// what gbnf_eval_accumulate refuses, for the one-call forms too (they check before THEIR first launch)
static int check_accumulate(const char* fn, const void* ll, int64_t ll_row_stride, int32_t n_used, int64_t n, const void* rho_dev,
                            int32_t component, const void* state_dev, const void* workspace, int64_t workspace_bytes) {
  if (!ll || !rho_dev || !state_dev || !workspace) return fail(GBNF_ERR_INVALID, "%s: ll / rho_dev / state_dev / workspace is null", fn);
  if (n < 0) return fail(GBNF_ERR_INVALID, "%s: n = %lld (must be >= 0)", fn, (long long)n);
  if (n_used < 1) return fail(GBNF_ERR_INVALID, "%s: n_used = %d (must be >= 1)", fn, (int)n_used);
  if (component < 0 || component >= n_used)
    return fail(GBNF_ERR_INVALID, "%s: component = %d outside [0,%d)", fn, (int)component, (int)n_used);
  if (ll_row_stride < n) return fail(GBNF_ERR_INVALID, "%s: ll_row_stride = %lld < n = %lld", fn, (long long)ll_row_stride, (long long)n);
  if (workspace_bytes < EVAL_WORKSPACE_BYTES)
    return fail(GBNF_ERR_INVALID, "%s: workspace of %lld bytes < %lld (gbnf_eval_workspace_bytes)", fn, (long long)workspace_bytes,
                (long long)EVAL_WORKSPACE_BYTES);
  return GBNF_OK;
}

static int launch_accumulate(const char* fn, const float* ll, int64_t stride, int n_used, int64_t n, const float* rho, int component,
                             float* G_out, double* state, double* partial, hipStream_t s) {
  if (n == 0) return GBNF_OK;
  const unsigned nb = eval_grid(n);
  hipLaunchKernelGGL(eval_partial_kernel, dim3(nb), dim3(EVAL_THREADS), 0, s, ll, stride, n_used, n, rho, component, G_out, partial);
  hipLaunchKernelGGL(eval_finalize_kernel, dim3(1), dim3(64), 0, s, (const double*)partial, (int)nb, n, state);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

static int check_class_loss(const char* fn, const void* y_logits, const void* y, int64_t n, int32_t Y, const void* rho_dev, int32_t n_used,
                            int32_t c, const void* state_dev, const void* workspace, int64_t workspace_bytes) {
  if (!y_logits || !y || !rho_dev || !state_dev || !workspace)
    return fail(GBNF_ERR_INVALID, "%s: y_logits / y / rho_dev / state_dev / workspace is null", fn);
  if (n < 0) return fail(GBNF_ERR_INVALID, "%s: n = %lld (must be >= 0)", fn, (long long)n);
  if (Y < 1 || Y > 256) return fail(GBNF_ERR_INVALID, "%s: Y = %d outside [1,256]", fn, (int)Y);
  if (n_used < 1) return fail(GBNF_ERR_INVALID, "%s: n_used = %d (must be >= 1)", fn, (int)n_used);
  if (c < 0 || c >= n_used) return fail(GBNF_ERR_INVALID, "%s: c = %d outside [0,%d)", fn, (int)c, (int)n_used);
  if (workspace_bytes < EVAL_WORKSPACE_BYTES)
    return fail(GBNF_ERR_INVALID, "%s: workspace of %lld bytes < %lld (gbnf_eval_workspace_bytes)", fn, (long long)workspace_bytes,
                (long long)EVAL_WORKSPACE_BYTES);
  return GBNF_OK;
}

static int launch_class_loss(const char* fn, const float* logits, const float* y, int64_t n, int Y, const float* rho, int n_used, int c,
                             double* state, double* partial, hipStream_t s) {
  if (n == 0) return GBNF_OK;
  const unsigned nb = eval_grid(n);
  hipLaunchKernelGGL(class_loss_partial_kernel, dim3(nb), dim3(EVAL_THREADS), 0, s, logits, y, n, Y, partial);
  hipLaunchKernelGGL(class_loss_finalize_kernel, dim3(1), dim3(64), 0, s, (const double*)partial, (int)nb, n, rho, n_used, c, state);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

// the caller's workspace of one image evaluation call, in 256-byte aligned pieces
struct ImageEvalLayout {
  int64_t flow_bytes, ldj, logits, part, total;
};

static int image_eval_layout(const gbnf_image_flow* const* flows, int n_flows, int64_t n, int32_t y_classes, ImageEvalLayout* L) {
  int64_t worst = 0;
  for (int c = 0; c < n_flows; ++c) {
    int64_t b = 0;
    if (const int rc = gbnf_image_flow_workspace_bytes(flows[c], n, &b)) return rc;
    if (b > worst) worst = b;
  }
  int64_t off = 0;
  L->flow_bytes = eval_align256(worst); off += L->flow_bytes;
  L->ldj = off; off += eval_align256(n * 4);
  L->logits = off; off += eval_align256(n * (int64_t)y_classes * 4);
  L->part = off; off += EVAL_WORKSPACE_BYTES;
  L->total = off;
  return GBNF_OK;
}

// gbnf_image_mixture_evaluate (y null: every handle plain) and gbnf_image_mixture_evaluate_y (y (n, Y): every handle conditioned on one
// Y, every handle with a class head), built as image_rho_step is (gbnf_image_boost.hip)
static int image_evaluate(const char* fn, const gbnf_image_flow* const* flows, int32_t n_used, int32_t component, const float* x,
                          const float* noise, const float* y, bool with_y, int64_t n, const float* rho_dev, float* ll_workspace,
                          float* G_out, double* state_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!flows || !x || !rho_dev || !ll_workspace || !state_dev || !workspace || (with_y && !y))
    return fail(GBNF_ERR_INVALID, "%s: flows / x / %srho_dev / ll_workspace / state_dev / workspace is null", fn, with_y ? "y / " : "");
  if (n < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld (must be >= 1)", fn, (long long)n);
  if (n_used < 1) return fail(GBNF_ERR_INVALID, "%s: n_used = %d (must be >= 1)", fn, (int)n_used);
  if (component < 0 || component >= n_used)
    return fail(GBNF_ERR_INVALID, "%s: component = %d outside [0,%d)", fn, (int)component, (int)n_used);
  if (const int rc = check_image_flows(fn, flows, n_used)) return rc;
  int32_t Y = 0;
  if (const int rc = check_image_flows_y(fn, flows, n_used, with_y, &Y)) return rc;
  for (int c = 0; with_y && c < n_used; ++c)
    if (!image_flow_has_class_head(flows[c]))
      return fail(GBNF_ERR_INVALID, "%s: flows[%d] has no class head (project_class): its share of the class loss cannot be formed", fn, c);
  ImageEvalLayout L;
  if (const int rc = image_eval_layout(flows, n_used, n, Y, &L)) return rc;
  if (workspace_bytes < L.total)
    return fail(GBNF_ERR_INVALID, "%s: workspace of %lld bytes < %lld (gbnf_image_mixture_evaluate_workspace_bytes)", fn,
                (long long)workspace_bytes, (long long)L.total);
  char* ws = (char*)workspace;
  float* ldj = (float*)(ws + L.ldj);
  float* logits = (float*)(ws + L.logits);
  double* partial = (double*)(ws + L.part);
  hipStream_t s = (hipStream_t)stream;
  for (int c = 0; c < n_used; ++c) {     // one chain after the other on the caller's stream: they share the workspace
    float* ll = ll_workspace + (int64_t)c * n;
    if (!with_y) {
      if (const int rc = gbnf_image_flow_forward(flows[c], x, noise, n, nullptr, ldj, ll, workspace, L.flow_bytes, stream)) return rc;
      continue;
    }
    if (const int rc = gbnf_image_flow_forward_y(flows[c], x, noise, y, n, nullptr, ldj, ll, logits, workspace, L.flow_bytes, stream)) return rc;
    if (const int rc = launch_class_loss(fn, logits, y, n, Y, rho_dev, n_used, c, state_dev, partial, s)) return rc;
  }
  return launch_accumulate(fn, ll_workspace, n, n_used, n, rho_dev, component, G_out, state_dev, partial, s);
}

}  // namespace gbnf

using namespace gbnf;

extern "C" {

int gbnf_eval_workspace_bytes(int64_t n, int64_t* bytes) {
  if (!bytes || n < 0) return fail(GBNF_ERR_INVALID, "gbnf_eval_workspace_bytes: bad argument");
  *bytes = EVAL_WORKSPACE_BYTES;
  return GBNF_OK;
}

int gbnf_eval_accumulate(const float* ll, int64_t ll_row_stride, int32_t n_used, int64_t n, const float* rho_dev, int32_t component,
                         float* G_out_or_null, double* state_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "gbnf_eval_accumulate";
  if (const int rc = check_accumulate(fn, ll, ll_row_stride, n_used, n, rho_dev, component, state_dev, workspace, workspace_bytes)) return rc;
  return launch_accumulate(fn, ll, ll_row_stride, n_used, n, rho_dev, component, G_out_or_null, state_dev, (double*)workspace,
                           (hipStream_t)stream);
}

int gbnf_eval_accumulate_class_loss(const float* y_logits, const float* y, int64_t n, int32_t Y, const float* rho_dev, int32_t n_used,
                                    int32_t c, double* state_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "gbnf_eval_accumulate_class_loss";
  if (const int rc = check_class_loss(fn, y_logits, y, n, Y, rho_dev, n_used, c, state_dev, workspace, workspace_bytes)) return rc;
  return launch_class_loss(fn, y_logits, y, n, Y, rho_dev, n_used, c, state_dev, (double*)workspace, (hipStream_t)stream);
}

int gbnf_mixture_evaluate(const gbnf_mixture* mix, const float* x, int64_t n, int32_t n_used, int32_t component, const float* rho_dev,
                          float* ll_workspace, float* G_out_or_null, double* state_dev, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  const char* fn = "gbnf_mixture_evaluate";
  if (!mix) return fail(GBNF_ERR_INVALID, "%s: mix is null", fn);
  if (!x && n > 0) return fail(GBNF_ERR_INVALID, "%s: x is null", fn);
  if (const int rc = check_accumulate(fn, ll_workspace, n, n_used, n, rho_dev, component, state_dev, workspace, workspace_bytes)) return rc;
  int C = 0, d = 0;
  if (const int rc = mixture_shape(mix, &C, &d)) return rc;
  if (n_used > C) return fail(GBNF_ERR_INVALID, "%s: n_used = %d, the mixture holds %d component(s)", fn, (int)n_used, C);
  if (n == 0) return GBNF_OK;
  if (const int rc = gbnf_mixture_component_log_prob(mix, x, n, 0, n_used, ll_workspace, stream)) return rc;
  return launch_accumulate(fn, ll_workspace, n, n_used, n, rho_dev, component, G_out_or_null, state_dev, (double*)workspace,
                           (hipStream_t)stream);
}

int gbnf_image_mixture_evaluate_workspace_bytes(const gbnf_image_flow* const* flows, int32_t n_flows, int64_t n, int64_t* bytes) {
  const char* fn = "gbnf_image_mixture_evaluate_workspace_bytes";
  if (!flows || !bytes) return fail(GBNF_ERR_INVALID, "%s: flows / bytes is null", fn);
  if (n_flows < 1 || n < 1) return fail(GBNF_ERR_INVALID, "%s: n_flows = %d, n = %lld (both must be >= 1)", fn, (int)n_flows, (long long)n);
  if (const int rc = check_image_flows(fn, flows, n_flows)) return rc;
  int32_t Y = 0;                                       // the logits' scratch is sized by the first handle's classes (0: a plain model)
  if (const int rc = gbnf_image_flow_y_classes(flows[0], &Y)) return rc;
  ImageEvalLayout L;
  if (const int rc = image_eval_layout(flows, n_flows, n, Y, &L)) return rc;
  *bytes = L.total;
  return GBNF_OK;
}

int gbnf_image_mixture_evaluate(const gbnf_image_flow* const* flows, int32_t n_used, int32_t component, const float* x, const float* noise,
                                int64_t n, const float* rho_dev, float* ll_workspace, float* G_out_or_null, double* state_dev,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  return image_evaluate("gbnf_image_mixture_evaluate", flows, n_used, component, x, noise, nullptr, false, n, rho_dev, ll_workspace,
                        G_out_or_null, state_dev, workspace, workspace_bytes, stream);
}

int gbnf_image_mixture_evaluate_y(const gbnf_image_flow* const* flows, int32_t n_used, int32_t component, const float* x,
                                  const float* noise, const float* y_dev, int64_t n, const float* rho_dev, float* ll_workspace,
                                  float* G_out_or_null, double* state_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  return image_evaluate("gbnf_image_mixture_evaluate_y", flows, n_used, component, x, noise, y_dev, true, n, rho_dev, ll_workspace,
                        G_out_or_null, state_dev, workspace, workspace_bytes, stream);
}

}  // extern "C"
