// gbnf_image_score.hip -- the score of the image path on the device (gfx950): grad_x log p(x) of one Glow component and of the
// boosted mixture  log p(x) = LSE_c(log_w_c + ll_c(x)),  whose gradient is  sum_c r_c grad_x ll_c  with the responsibilities
// r_c = softmax_c(log_w + ll).
//
//   img_pre_adjoint_kernel        the last adjoint of gbnf_image_trainer_backward_x: the gradient of level 0's input (squeezed logits in
//                                 H/2 x W/2 storage) and g_ldj -> g_x on the Hi x Wi image; v recomputed from x and noise as img_pre_body does
//   img_score_prior_kernel        (mu | logvar) = bias e^{3 logs} of a live learn_top_fn (2 Cz floats; zeros without one)
//   img_score_ll_kernel           ll_i = log_normal_diag(z_i, mu, logvar) + ldj_i + the 1x1 log-dets: one workgroup per image, f64, fixed order
//   img_score_seed_kernel         g_z = -r (z - mu) e^{-logvar}, g_ldj = r: the gradient of that ll scaled per row
//   mix_resp_kernel               r (C, N) and G (N) from ll (C, N) and log_w (C): one thread per column, f64, component order
//
// Everything here is elementwise or a short per-image reduction: no MFMA, no LDS opt-in, no atomics, plain vector stores.  The
// convolutions of the backward are gbnf_image.hip's through gbnf_image_trainer_backward_x (gbnf_image_train.hip).
//
// Reference semantics: models/glow.py:125-179 (dequantisation, logit, log-det), image_experiment.py:227 and
// utils/distributions.py:13-21 (log_normal_diag without the 2 pi term), models/boosted_flow.py:119-207 (the mixture's recursion;
// its closed form is log_w_c = log(rho_c / sum_j rho_j)).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/gbnf.h"
#include "gbnf_internal.h"
#include "gbnf_image_train.h"
#include "gbnf_image_ycond.h"

namespace gbnf {

constexpr int SC_THREADS = 256;

// one thread per pixel of x (n, C, Hi, Wi).  Forward (img_pre_body): u = (255 x + noise) / 256, v = ((2u - 1) b + 1) / 2,
// logit = log v - log(1 - v), ldj += -log v - log(1 - v).  So d logit / dv = 1 / (v (1 - v)), d ldj / dv = (2v - 1) / (v (1 - v)),
// dv / dx = b 255 / 256.  Pixel (c, y, x) lives at channel 4c + 2 (y & 1) + (x & 1), row y / 2, column x / 2 of the squeezed storage.
__global__ void __launch_bounds__(SC_THREADS) img_pre_adjoint_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                                     const float* __restrict__ gs, const float* __restrict__ g_ldj,
                                                                     float* __restrict__ g_x, int C, int H2, int W2, int Hi, int Wi, float bounds,
                                                                     int accumulate, int64_t total /* n C Hi Wi */) {
  const int64_t t = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (t >= total) return;
  const int xchw = C * Hi * Wi;
  const int64_t n = t / xchw;
  const int src = (int)(t - n * xchw);
  const int c = src / (Hi * Wi), rem = src - c * Hi * Wi, y = rem / Wi, xx = rem - y * Wi;
  float v = x[t];
  v = (255.0f * v + (noise ? noise[t] : 0.0f)) / 256.0f;
  v = ((v * 2.0f - 1.0f) * bounds + 1.0f) * 0.5f;
  const int oc = 4 * c + 2 * (y & 1) + (xx & 1);
  const float g_logit = gs[(n * (4 * C) + oc) * (int64_t)(H2 * W2) + (y >> 1) * W2 + (xx >> 1)];
  const float g = (g_logit + g_ldj[n] * (2.0f * v - 1.0f)) / (v * (1.0f - v)) * bounds * (255.0f / 256.0f);
  g_x[t] = accumulate ? g_x[t] + g : g;
}

void img_launch_pre_adjoint(const float* x, const float* noise, const float* gs, const float* g_ldj, float* g_x, int C, int H, int W, int Hi,
                            int Wi, float bounds, int accumulate, int64_t n, hipStream_t s) {
  const int64_t total = n * C * Hi * Wi;
  hipLaunchKernelGGL(img_pre_adjoint_kernel, dim3((unsigned)((total + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, s, x, noise, gs,
                     g_ldj, g_x, C, H / 2, W / 2, Hi, Wi, bounds, accumulate, total);
}

// Conv2dZeros of a zero input (models/layers.py:609-630), f32 as torch computes it; bias null: the zero-mean unit prior
__global__ void __launch_bounds__(SC_THREADS) img_score_prior_kernel(const float* __restrict__ bias, const float* __restrict__ logs, int n2,
                                                                     float* __restrict__ prior) {
  const int j = blockIdx.x * SC_THREADS + threadIdx.x;
  if (j >= n2) return;
  prior[j] = bias != nullptr ? bias[j] * expf(3.0f * logs[j]) : 0.0f;
}

// the workgroup's 256 values added up in a fixed tree order; every thread gets the sum
__device__ __forceinline__ double sc_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = SC_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

// grid n: ll[i] = sum_{c,p} -0.5 (lv_c + (z - mu_c)^2 e^{-lv_c}) + ldj[i] + sum_m ld[m].  prior row i at prior + i * prior_stride.
__global__ void __launch_bounds__(SC_THREADS) img_score_ll_kernel(const float* __restrict__ z, const float* __restrict__ ldj,
                                                                  const double* __restrict__ ld, int n_mix, const float* __restrict__ prior,
                                                                  int64_t prior_stride, int Cz, int HW, float* __restrict__ ll) {
  __shared__ double lds[SC_THREADS];
  const int64_t i = blockIdx.x;
  const float* zi = z + i * (int64_t)Cz * HW;
  const float* pr = prior + i * prior_stride;
  double acc = 0.0;
  for (int e = threadIdx.x; e < Cz * HW; e += SC_THREADS) {
    const int c = e / HW;
    const float mu = pr[c], lv = pr[Cz + c];
    const float d = zi[e] - mu;
    acc += -0.5 * ((double)lv + (double)(d * d * expf(-lv)));
  }
  const double s = sc_block_sum(acc, lds);
  if (threadIdx.x != 0) return;
  double lds_sum = 0.0;
  for (int m = 0; m < n_mix; ++m) lds_sum += ld[m];
  ll[i] = (float)(s + (double)ldj[i] + lds_sum);
}

// one thread per element of z (n, Cz, HW); r null: 1
__global__ void __launch_bounds__(SC_THREADS) img_score_seed_kernel(const float* __restrict__ z, const float* __restrict__ prior,
                                                                    int64_t prior_stride, const float* __restrict__ r, int Cz, int HW,
                                                                    float* __restrict__ g_z, float* __restrict__ g_ldj, int64_t total /* n Cz HW */) {
  const int64_t t = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (t >= total) return;
  const int per = Cz * HW;
  const int64_t i = t / per;
  const int e = (int)(t - i * per), c = e / HW;
  const float* pr = prior + i * prior_stride;
  const float ri = r != nullptr ? r[i] : 1.0f;
  g_z[t] = -ri * (z[t] - pr[c]) * expf(-pr[Cz + c]);
  if (e == 0) g_ldj[i] = ri;
}

// one thread per column: a_c = log_w[c] + ll[c][n] in f64; G = LSE_c a_c, r_c = exp(a_c - G) as exp(a_c - m) / sum.  A column whose
// largest a_c is -inf: G = -inf, r = 0 (torch.logsumexp's value; no NaN out of inf - inf).  NaN entries propagate.
__global__ void __launch_bounds__(SC_THREADS) mix_resp_kernel(const float* __restrict__ ll, const float* __restrict__ log_w, int C, int64_t N,
                                                              float* __restrict__ r, float* __restrict__ G) {
  const int64_t n = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (n >= N) return;
  double m = -INFINITY;
  bool nan = false;
  for (int c = 0; c < C; ++c) {
    const double a = (double)log_w[c] + (double)ll[(int64_t)c * N + n];
    if (a != a) nan = true;
    if (a > m) m = a;
  }
  if (nan) {
    G[n] = NAN;
    for (int c = 0; c < C; ++c) r[(int64_t)c * N + n] = NAN;
    return;
  }
  if (m == -INFINITY) {
    G[n] = -INFINITY;
    for (int c = 0; c < C; ++c) r[(int64_t)c * N + n] = 0.0f;
    return;
  }
  double sum = 0.0;
  for (int c = 0; c < C; ++c) sum += exp((double)log_w[c] + (double)ll[(int64_t)c * N + n] - m);
  G[n] = (float)(m + log(sum));
  for (int c = 0; c < C; ++c) r[(int64_t)c * N + n] = (float)(exp((double)log_w[c] + (double)ll[(int64_t)c * N + n] - m) / sum);
}

namespace {

int64_t sc_align256(int64_t b) { return (b + 255) / 256 * 256; }

void launch_seed(const float* z, const float* prior, int64_t prior_stride, const float* r, int64_t n, int Cz, int HW, float* g_z, float* g_ldj,
                 hipStream_t s) {
  const int64_t total = n * Cz * HW;
  hipLaunchKernelGGL(img_score_seed_kernel, dim3((unsigned)((total + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, s, z, prior,
                     prior_stride, r, Cz, HW, g_z, g_ldj, total);
}

void launch_resp(const float* ll, const float* log_w, int C, int64_t N, float* r, float* G, hipStream_t s) {
  hipLaunchKernelGGL(mix_resp_kernel, dim3((unsigned)((N + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, s, ll, log_w, C, N, r, G);
}

// the caller's workspace of one mixture score, in 256-byte aligned pieces: per component z | ldj | prior | trace, then the shared
// ll (C, n) | r (C, n) | g_z | g_ldj | the trainers' forward / backward workspace (the largest)
struct ScoreLayout {
  int64_t comp_bytes;                 // of one component's block (the largest component sizes every block)
  int64_t z, ldj, prior, trace;       // offsets inside a component's block
  int64_t ll, r, g_z, g_ldj, ws, ws_bytes, total;
};

int score_layout(const char* fn, gbnf_image_trainer* const* trainers, int C, int64_t n, ScoreLayout* L) {
  int64_t zf = 0, pf = 0, tf = 0, wsb = 0;
  for (int c = 0; c < C; ++c) {
    const gbnf_image_trainer* t = trainers[c];
    ImageScoreTop top{};
    if (const int rc = image_score_top(fn, t, &top)) return rc;
    int64_t trace_floats = 0, ws_bytes = 0;
    if (const int rc = gbnf_image_trainer_trace_floats(t, n, &trace_floats)) return rc;
    if (const int rc = gbnf_image_trainer_workspace_bytes(t, n, &ws_bytes)) return rc;
    zf = std::max(zf, n * t->zC * t->zH * t->zW);
    pf = std::max(pf, (top.y_classes > 0 ? n : 1) * 2 * (int64_t)t->zC);
    tf = std::max(tf, trace_floats);
    wsb = std::max(wsb, ws_bytes);
  }
  int64_t off = 0;
  L->z = off; off += sc_align256(zf * 4);
  L->ldj = off; off += sc_align256(n * 4);
  L->prior = off; off += sc_align256(pf * 4);
  L->trace = off; off += sc_align256(tf * 4);
  L->comp_bytes = off;
  off = L->comp_bytes * C;
  L->ll = off; off += sc_align256((int64_t)C * n * 4);
  L->r = off; off += sc_align256((int64_t)C * n * 4);
  L->g_z = off; off += sc_align256(zf * 4);
  L->g_ldj = off; off += sc_align256(n * 4);
  L->ws = off; L->ws_bytes = wsb; off += sc_align256(wsb);
  L->total = off;
  return GBNF_OK;
}

// non-null trainers of one input shape, all plain or all conditioned on one class count (*y_classes)
int check_score_trainers(const char* fn, gbnf_image_trainer* const* trainers, int C, int* y_classes) {
  for (int c = 0; c < C; ++c) {
    const gbnf_image_trainer* t = trainers[c];
    if (!t) return fail(GBNF_ERR_INVALID, "%s: trainers[%d] is null", fn, c);
    ImageScoreTop top{};
    if (const int rc = image_score_top(fn, t, &top)) return rc;
    const gbnf_image_trainer* t0 = trainers[0];
    if (t->C != t0->C || t->Hi != t0->Hi || t->Wi != t0->Wi)
      return fail(GBNF_ERR_INVALID, "%s: trainers[%d] takes %d x %d x %d images, trainers[0] %d x %d x %d", fn, c, t->C, t->Hi, t->Wi, t0->C,
                  t0->Hi, t0->Wi);
    if (c == 0) *y_classes = top.y_classes;
    else if (top.y_classes != *y_classes)
      return fail(GBNF_ERR_INVALID, "%s: trainers[%d] has %d classes bound, trainers[0] %d: y has one width", fn, c, top.y_classes, *y_classes);
  }
  return GBNF_OK;
}

}  // namespace

}  // namespace gbnf

using namespace gbnf;

extern "C" {

int gbnf_image_score_seed(const float* z, const float* prior, int64_t prior_stride, const float* r_or_null, int64_t n, int32_t Cz, int32_t HW,
                          float* g_z, float* g_ldj, void* stream) {
  const char* fn = "gbnf_image_score_seed";
  if (!z || !prior || !g_z || !g_ldj) return fail(GBNF_ERR_INVALID, "%s: z / prior / g_z / g_ldj is null", fn);
  if (n < 0 || Cz < 1 || HW < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld, Cz = %d, HW = %d", fn, (long long)n, (int)Cz, (int)HW);
  if (prior_stride != 0 && prior_stride != 2 * (int64_t)Cz)
    return fail(GBNF_ERR_INVALID, "%s: prior_stride = %lld (0: one prior for all rows, or 2 Cz = %d)", fn, (long long)prior_stride, 2 * (int)Cz);
  if (n == 0) return GBNF_OK;
  launch_seed(z, prior, prior_stride, r_or_null, n, Cz, HW, g_z, g_ldj, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

int gbnf_mixture_responsibilities(const float* ll, const float* log_w, int32_t n_components, int64_t n, float* r, float* G, void* stream) {
  const char* fn = "gbnf_mixture_responsibilities";
  if (!ll || !log_w || !r || !G) return fail(GBNF_ERR_INVALID, "%s: ll / log_w / r / G is null", fn);
  if (n_components < 1 || n < 0) return fail(GBNF_ERR_INVALID, "%s: n_components = %d, n = %lld", fn, (int)n_components, (long long)n);
  if (n == 0) return GBNF_OK;
  launch_resp(ll, log_w, n_components, n, r, G, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

int gbnf_image_mixture_score_workspace_bytes(gbnf_image_trainer* const* trainers, int32_t n_components, int64_t n, int64_t* bytes) {
  const char* fn = "gbnf_image_mixture_score_workspace_bytes";
  if (!trainers || !bytes) return fail(GBNF_ERR_INVALID, "%s: trainers / bytes is null", fn);
  if (n_components < 1 || n < 0) return fail(GBNF_ERR_INVALID, "%s: n_components = %d, n = %lld", fn, (int)n_components, (long long)n);
  int y_classes = 0;
  if (const int rc = check_score_trainers(fn, trainers, n_components, &y_classes)) return rc;
  ScoreLayout L;
  if (const int rc = score_layout(fn, trainers, n_components, n, &L)) return rc;
  *bytes = L.total;
  return GBNF_OK;
}

int gbnf_image_mixture_score(gbnf_image_trainer* const* trainers, int32_t n_components, const float* log_w, const float* x, const float* noise,
                             const float* y_or_null, int64_t n, float* g_x, float* G, float* r_or_null, void* workspace, int64_t workspace_bytes,
                             void* stream) {
  const char* fn = "gbnf_image_mixture_score";
  if (!trainers || !log_w || !x || !g_x || !G || !workspace)
    return fail(GBNF_ERR_INVALID, "%s: trainers / log_w / x / g_x / G / workspace is null", fn);
  if (n_components < 1) return fail(GBNF_ERR_INVALID, "%s: n_components = %d (must be >= 1)", fn, (int)n_components);
  if (n < 0) return fail(GBNF_ERR_INVALID, "%s: n < 0", fn);
  if (n > 65535) return fail(GBNF_ERR_UNSUPPORTED, "%s: at most 65535 images per call", fn);
  const int C = (int)n_components;
  int y_classes = 0;
  if (const int rc = check_score_trainers(fn, trainers, C, &y_classes)) return rc;
  if (y_classes > 0 && !y_or_null) return fail(GBNF_ERR_INVALID, "%s: the trainers are class-conditional (%d classes): y is null", fn, y_classes);
  if (y_classes == 0 && y_or_null) return fail(GBNF_ERR_INVALID, "%s: y given, but the trainers have no conditioning bound", fn);
  if (n == 0) return GBNF_OK;
  ScoreLayout L;
  if (const int rc = score_layout(fn, trainers, C, n, &L)) return rc;
  if (workspace_bytes < L.total)
    return fail(GBNF_ERR_INVALID, "%s: workspace too small: %lld bytes < %lld (gbnf_image_mixture_score_workspace_bytes)", fn,
                (long long)workspace_bytes, (long long)L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* ll = (float*)(ws + L.ll);
  float* r = (float*)(ws + L.r);
  float* g_z = (float*)(ws + L.g_z);
  float* g_ldj = (float*)(ws + L.g_ldj);
  // 1. every component's forward on (x, noise) and its full ll: the trace, z and the prior stay in the component's block
  for (int c = 0; c < C; ++c) {
    gbnf_image_trainer* t = trainers[c];
    char* blk = ws + L.comp_bytes * c;
    float* z = (float*)(blk + L.z);
    float* ldj = (float*)(blk + L.ldj);
    float* prior = (float*)(blk + L.prior);
    ImageScoreTop top{};
    if (const int rc = image_score_top(fn, t, &top)) return rc;
    if (const int rc = image_score_logdets(fn, t, stream)) return rc;
    if (const int rc = gbnf_image_trainer_forward(t, x, noise, n, z, ldj, (float*)(blk + L.trace), ws + L.ws, L.ws_bytes, stream)) return rc;
    const int Cz = t->zC, HW = t->zH * t->zW;
    if (top.y_classes > 0) {
      YCond yc{};
      yc.top_bias = top.top_bias; yc.top_logs = top.top_logs;
      yc.cond_w = top.yc[0]; yc.cond_b = top.yc[1]; yc.cond_logs = top.yc[2]; yc.class_w = top.yc[3]; yc.class_b = top.yc[4]; yc.class_logs = top.yc[5];
      yc.Y = top.y_classes; yc.Cz = Cz; yc.HW = HW;
      ycond_launch_prior(yc, y_or_null, n, nullptr, 0.0f, prior, nullptr, s);
    } else {
      hipLaunchKernelGGL(img_score_prior_kernel, dim3((unsigned)((2 * Cz + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, s, top.top_bias,
                         top.top_logs, 2 * Cz, prior);
    }
    hipLaunchKernelGGL(img_score_ll_kernel, dim3((unsigned)n), dim3(SC_THREADS), 0, s, (const float*)z, (const float*)ldj, top.ld, top.n_mix,
                       (const float*)prior, top.y_classes > 0 ? 2 * (int64_t)Cz : (int64_t)0, Cz, HW, ll + (int64_t)c * n);
  }
  // 2. the responsibilities and log p
  launch_resp(ll, log_w, C, n, r, G, s);
  if (r_or_null != nullptr && hipMemcpyAsync(r_or_null, r, (size_t)C * n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return fail(GBNF_ERR_HIP, "%s: the copy of r failed", fn);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  // 3. one data-gradient-only backward per component, seeded with its row of r, added into g_x in component order
  for (int c = 0; c < C; ++c) {
    gbnf_image_trainer* t = trainers[c];
    char* blk = ws + L.comp_bytes * c;
    ImageScoreTop top{};
    if (const int rc = image_score_top(fn, t, &top)) return rc;
    const int Cz = t->zC, HW = t->zH * t->zW;
    launch_seed((const float*)(blk + L.z), (const float*)(blk + L.prior), top.y_classes > 0 ? 2 * (int64_t)Cz : (int64_t)0, r + (int64_t)c * n, n,
                Cz, HW, g_z, g_ldj, s);
    if (const int rc = gbnf_image_trainer_backward_x(t, (const float*)(blk + L.trace), x, noise, n, g_z, g_ldj, nullptr, g_x, c > 0 ? 1 : 0,
                                                     ws + L.ws, L.ws_bytes, stream))
      return rc;
  }
  e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

}  // extern "C"
