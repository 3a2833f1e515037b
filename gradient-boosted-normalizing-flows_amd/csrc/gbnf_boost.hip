// gbnf_boost.hip -- the parts of a BOOSTED training step that belong to boosting itself, on the device (gfx950): what the reference does
// in eager PyTorch around the library's mixture, weights and training calls.
//
//   resample_scan_kernel     the inclusive prefix sum of the boosting weights in f64 (the cdf behind torch.multinomial(weights, N,
//                            replacement=True), density_experiment.py:643), plus the step's G_nll, effective sample size and bad-weight count
//   resample_search_kernel   one draw per thread: the smallest row whose cdf entry exceeds u * total      (:643-644)
//   rho_partial_kernel       per-workgroup sums of fixed_ll - new_ll, fixed_ll by the un-normalised recursion of
//                            models/boosted_flow.py:119-139
//   rho_finalize_kernel      the gradient, the step and the clamp of update_rho                           (models/boosted_flow.py:141-207)
//   rho_update_launch        those two launches on a (component + 1, n) table: shared with the image call (gbnf_image_boost.hip)
//
// Launch-latency sized like boosting_weights_kernel (gbnf_api.hip): no matrix pipe, no LDS staging.  Every reduction runs in f64 in an
// order that depends on the sizes alone -- no atomics --, so the cdf, the rows and the statistics are bit-identical from run to run.
// Why f64: with boosting-shaped weights a sequential f32 prefix sum moves 3 % of the draws at n = 4 099 and 10 % at n = 70 001.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <mutex>

#include "../../include/gbnf.h"
#include "gbnf_internal.h"
#include "gbnf_opt.h"

namespace gbnf {

constexpr int SCAN_THREADS = 1024;               // one workgroup: 16 waves
constexpr int SCAN_WAVES = SCAN_THREADS / 64;
constexpr int SEARCH_THREADS = 256;
constexpr int RHO_THREADS = 256;
constexpr int RHO_MAX_PARTIALS = 256;
static_assert(RHO_MAX_PARTIALS <= RHO_THREADS, "the finalise kernel re-adds the partial sums one per thread");

static int64_t boost_align256(int64_t b) { return (b + 255) / 256 * 256; }

// what a weight counts for: max(w, 0), a non-finite one 0
__device__ __forceinline__ double weight_mass(float w) { return (w > 0.0f && w < INFINITY) ? (double)w : 0.0; }

// the wave's 64 values added in a fixed butterfly order; every lane gets the sum
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// cdf[j] = sum_{k <= j} max(w_k, 0).  Thread t owns the rows [t * chunk, (t + 1) * chunk): it adds them up, the chunk sums are scanned
// across the wave with shuffles and across the 16 waves through LDS, then the thread walks its rows again from its exclusive prefix.
// With `stats` (gbnf_boosted_nll_step) the same walk leaves  [4] -mean(G)  [5] (sum w)^2 / sum w^2  [6] bad weights  [7] 0.
__global__ void __launch_bounds__(SCAN_THREADS) resample_scan_kernel(const float* __restrict__ w, int64_t n, double* __restrict__ cdf,
                                                                     const float* __restrict__ G, float* __restrict__ stats) {
  __shared__ double wave_tot[SCAN_WAVES];
  __shared__ double red[3][SCAN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t chunk = (n + SCAN_THREADS - 1) / SCAN_THREADS;
  int64_t begin = (int64_t)tid * chunk;
  if (begin > n) begin = n;
  int64_t end = begin + chunk;
  if (end > n) end = n;
  double s = 0.0, s2 = 0.0, g = 0.0, bad = 0.0;
  for (int64_t j = begin; j < end; ++j) {
    const float v = w[j];
    const double a = weight_mass(v);
    s += a;
    s2 += a * a;
    if (!(v >= 0.0f && v < INFINITY)) bad += 1.0;
    if (G != nullptr) g += (double)G[j];
  }
  double incl = s;                                 // inclusive scan of the chunk sums across the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  double excl = __shfl_up(incl, 1);
  if (lane == 0) excl = 0.0;
  if (lane == 63) wave_tot[wave] = incl;
  if (stats != nullptr) {
    s2 = wave_sum(s2);
    g = wave_sum(g);
    bad = wave_sum(bad);
    if (lane == 0) { red[0][wave] = s2; red[1][wave] = g; red[2][wave] = bad; }
  }
  __syncthreads();
  double run = 0.0;                                // the waves before this one, in order
  for (int k = 0; k < wave; ++k) run += wave_tot[k];
  run += excl;
  for (int64_t j = begin; j < end; ++j) {
    run += weight_mass(w[j]);
    cdf[j] = run;
  }
  if (stats != nullptr && tid == 0) {
    double T = 0.0, S2 = 0.0, Gs = 0.0, B = 0.0;
    for (int k = 0; k < SCAN_WAVES; ++k) { T += wave_tot[k]; S2 += red[0][k]; Gs += red[1][k]; B += red[2][k]; }
    stats[4] = (float)(-(Gs / (double)n));
    stats[5] = S2 > 0.0 ? (float)(T * T / S2) : 0.0f;
    stats[6] = (float)B;
    stats[7] = 0.0f;
  }
}

// rows[i] = the smallest j with u[i] * T < cdf[j], T = cdf[n - 1].  Rounding between two threads' chunks of the scan may leave the cdf a
// last bit short of monotone there, so a row of no weight that the search lands on is passed over: such a row is never written.  A draw
// beyond the cdf (u >= 1, NaN, T == 0) takes the last row of positive weight, and row i % n when no row has any.
__global__ void __launch_bounds__(SEARCH_THREADS) resample_search_kernel(const float* __restrict__ w, const double* __restrict__ cdf, int64_t n,
                                                                         const float* __restrict__ u, int64_t m, int64_t* __restrict__ rows,
                                                                         int64_t* __restrict__ rows_copy) {
  const int64_t i = (int64_t)blockIdx.x * SEARCH_THREADS + threadIdx.x;
  if (i >= m) return;
  double target = (double)u[i] * cdf[n - 1];
  if (target < 0.0) target = 0.0;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (target < cdf[mid]) hi = mid; else lo = mid + 1;      // (a NaN target compares false: it ends beyond the cdf)
  }
  while (lo < n && !(weight_mass(w[lo]) > 0.0)) ++lo;
  if (lo >= n) {
    lo = n - 1;
    while (lo >= 0 && !(weight_mass(w[lo]) > 0.0)) --lo;
    if (lo < 0) lo = i % n;
  }
  rows[i] = lo;
  if (rows_copy != nullptr) rows_copy[i] = lo;
}

// the workgroup's 256 values added up in a fixed tree order; every thread gets the sum
__device__ __forceinline__ double rho_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = RHO_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

// partial[b] = sum over this workgroup's rows of fixed_ll - new_ll (each difference in f32 as the reference forms it, the sum in f64):
//   fixed_ll = ll_0;  for c = 1 .. component - 1:  fixed_ll = LSE(log(1 - rho[c]) + fixed_ll, log(rho[c]) + ll_c)   (torch.logsumexp
//   semantics, rho NOT normalised: NaN for rho[c] > 1);  new_ll = ll_component.  rho[component] is not read.
__global__ void __launch_bounds__(RHO_THREADS) rho_partial_kernel(const float* __restrict__ ll, int64_t n, int component,
                                                                  const float* __restrict__ rho, double* __restrict__ partial) {
  __shared__ double lds[RHO_THREADS];
  const int64_t stride = (int64_t)gridDim.x * RHO_THREADS;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * RHO_THREADS + threadIdx.x; i < n; i += stride) {
    float fixed = ll[i];
    for (int c = 1; c < component; ++c) {
      const float r = rho[c];
      const float a = logf(1.0f - r) + fixed;
      const float b = logf(r) + ll[(int64_t)c * n + i];
      float mx = fmaxf(a, b);                      // (as mixture_lse_kernel: a NaN term still makes the sum NaN)
      if (isinf(mx)) mx = 0.0f;
      fixed = mx + logf(expf(a - mx) + expf(b - mx));
    }
    acc += (double)(fixed - ll[(int64_t)component * n + i]);
  }
  const double s = rho_block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// grad = mean(fixed_ll - new_ll);  rho[component] = min(max(rho - step * grad, 0.01), 100) evaluated in f64 as the reference's Python
// floats are (a NaN gradient stays NaN through both comparisons, as it does there);  stats = [grad, before, after, |after - before|]
__global__ void __launch_bounds__(RHO_THREADS) rho_finalize_kernel(const double* __restrict__ partial, int n_partial, int64_t n, int component,
                                                                   float* __restrict__ rho, float step_size, float* __restrict__ stats) {
  __shared__ double lds[RHO_THREADS];
  const int tid = threadIdx.x;
  const double s = rho_block_sum(tid < n_partial ? partial[tid] : 0.0, lds);
  if (tid != 0) return;
  const float grad = (float)(s / (double)n);
  const float before = rho[component];
  double v = (double)before - (double)step_size * (double)grad;
  if (0.01 > v) v = 0.01;
  if (100.0 < v) v = 100.0;
  const float after = (float)v;
  rho[component] = after;
  stats[0] = grad;
  stats[1] = before;
  stats[2] = after;
  stats[3] = fabsf(after - before);
}

// per device: the partial sums between the two kernels of a rho update (neither gbnf_mixture_rho_step nor its image counterpart has
// a workspace argument for them); allocated on first use, never freed
static double* g_rho_partials[MAX_DEVICES] = {};
static std::mutex g_rho_mu;

// The tail of one update_rho iteration, shared by gbnf_mixture_rho_step and gbnf_image_mixture_rho_step (gbnf_image_boost.hip): the two
// launches above on a (component + 1, n) log-likelihood table, through the current device's partial-sum buffer.
int rho_update_launch(const char* fn, const float* ll, int64_t n, int component, float* rho_dev, float step_size, float* stats_dev,
                      hipStream_t s) {
  double* partial = nullptr;
  {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s: hipGetDevice: %s", fn, hipGetErrorString(e));
    if (dev < 0 || dev >= MAX_DEVICES) return fail(GBNF_ERR_UNSUPPORTED, "%s: device index %d", fn, dev);
    std::lock_guard<std::mutex> lk(g_rho_mu);
    if (!g_rho_partials[dev]) {
      e = hipMalloc((void**)&g_rho_partials[dev], sizeof(double) * RHO_MAX_PARTIALS);
      if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s: hipMalloc: %s", fn, hipGetErrorString(e));
    }
    partial = g_rho_partials[dev];
  }
  int64_t nb = (n + 4 * RHO_THREADS - 1) / (4 * RHO_THREADS);
  if (nb > RHO_MAX_PARTIALS) nb = RHO_MAX_PARTIALS;
  hipLaunchKernelGGL(rho_partial_kernel, dim3((unsigned)nb), dim3(RHO_THREADS), 0, s, ll, n, component, (const float*)rho_dev, partial);
  hipLaunchKernelGGL(rho_finalize_kernel, dim3(1), dim3(RHO_THREADS), 0, s, (const double*)partial, (int)nb, n, component, rho_dev,
                     step_size, stats_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

static int launch_resample(const float* w, int64_t n, const float* u, int64_t m, int64_t* rows, int64_t* rows_copy, double* cdf,
                           const float* G, float* stats, hipStream_t s, const char* fn) {
  hipLaunchKernelGGL(resample_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, w, n, cdf, G, stats);
  hipLaunchKernelGGL(resample_search_kernel, dim3((unsigned)((m + SEARCH_THREADS - 1) / SEARCH_THREADS)), dim3(SEARCH_THREADS), 0, s, w,
                     (const double*)cdf, n, u, m, rows, rows_copy);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

// the caller's workspace of one boosted step, in 256-byte aligned pieces
struct BoostLayout {
  int64_t step, step_bytes, ll, G, w, cdf, rows, total;
};
static int boost_layout(const gbnf_trainer* t, int n_fixed, int64_t n, BoostLayout* L) {
  int64_t step_bytes = 0;
  if (const int rc = gbnf_trainer_step_workspace_bytes(t, n, &step_bytes)) return rc;
  const int64_t nn = boost_align256(n * 4);
  int64_t off = 0;
  L->step = off; L->step_bytes = step_bytes; off += boost_align256(step_bytes);
  L->ll = off; off += boost_align256((int64_t)n_fixed * n * 4);
  L->G = off; off += nn;
  L->w = off; off += nn;
  L->cdf = off; off += boost_align256(n * 8);
  L->rows = off; off += boost_align256(n * 8);
  L->total = off;
  return GBNF_OK;
}

static int check_fixed(const char* fn, const gbnf_mixture* fixed, int n_fixed, const gbnf_trainer* t, TrainerOptView* tv) {
  if (!fixed || !t) return fail(GBNF_ERR_INVALID, "%s: fixed / trainer is null", fn);
  int C = 0, d = 0;
  if (const int rc = mixture_shape(fixed, &C, &d)) return rc;
  if (n_fixed < 1 || n_fixed > C) return fail(GBNF_ERR_INVALID, "%s: n_fixed = %d outside [1,%d]", fn, n_fixed, C);
  if (const int rc = trainer_opt_view(t, tv)) return rc;
  if (d != tv->d) return fail(GBNF_ERR_INVALID, "%s: the mixture has d = %d, the trainer d = %d", fn, d, tv->d);
  return GBNF_OK;
}

}  // namespace gbnf

using namespace gbnf;

extern "C" {

int gbnf_resample_workspace_bytes(int64_t n, int64_t* bytes) {
  if (!bytes || n < 1) return fail(GBNF_ERR_INVALID, "gbnf_resample_workspace_bytes: bad argument");
  *bytes = boost_align256(n * 8);
  return GBNF_OK;
}

int gbnf_resample_rows(const float* w, int64_t n, const float* u, int64_t m, int64_t* rows, void* workspace, int64_t workspace_bytes,
                       void* stream) {
  const char* fn = "gbnf_resample_rows";
  if (!w || !u || !rows || !workspace) return fail(GBNF_ERR_INVALID, "%s: w / u / rows / workspace is null", fn);
  if (n < 1 || m < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld, m = %lld (both must be >= 1)", fn, (long long)n, (long long)m);
  if (workspace_bytes < boost_align256(n * 8))
    return fail(GBNF_ERR_INVALID, "%s: workspace of %lld bytes < %lld (gbnf_resample_workspace_bytes)", fn, (long long)workspace_bytes,
                (long long)boost_align256(n * 8));
  return launch_resample(w, n, u, m, rows, nullptr, (double*)workspace, nullptr, nullptr, (hipStream_t)stream, fn);
}

int gbnf_boosted_step_workspace_bytes(const gbnf_mixture* fixed, int32_t n_fixed, const gbnf_trainer* trainer, int64_t n, int64_t* bytes) {
  const char* fn = "gbnf_boosted_step_workspace_bytes";
  if (!bytes || n < 1) return fail(GBNF_ERR_INVALID, "%s: bad argument", fn);
  TrainerOptView tv;
  if (const int rc = check_fixed(fn, fixed, n_fixed, trainer, &tv)) return rc;
  BoostLayout L;
  if (const int rc = boost_layout(trainer, n_fixed, n, &L)) return rc;
  *bytes = L.total;
  return GBNF_OK;
}

int gbnf_boosted_nll_step(const gbnf_mixture* fixed, int32_t n_fixed, const float* rho_dev, float beta, const gbnf_trainer* trainer,
                          const float* x, int64_t n, const float* u, float* grads, float* exp_avg, float* exp_avg_sq,
                          const gbnf_opt_hyper* hyper, float* stats_dev, int64_t* rows_out, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  const char* fn = "gbnf_boosted_nll_step";
  if (!trainer || !x || !grads || !stats_dev || !workspace) return fail(GBNF_ERR_INVALID, "%s: trainer / x / grads / stats_dev / workspace is null", fn);
  if (!u || !rho_dev) return fail(GBNF_ERR_INVALID, "%s: u / rho_dev is null", fn);
  if (n < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld (must be >= 1)", fn, (long long)n);
  if (const int rc = check_hyper(fn, hyper, exp_avg, exp_avg_sq)) return rc;
  TrainerOptView tv;
  if (const int rc = check_fixed(fn, fixed, n_fixed, trainer, &tv)) return rc;
  BoostLayout L;
  if (const int rc = boost_layout(trainer, n_fixed, n, &L)) return rc;
  if (workspace_bytes < L.total)
    return fail(GBNF_ERR_INVALID, "%s: workspace too small: %lld bytes < %lld (gbnf_boosted_step_workspace_bytes)", fn, (long long)workspace_bytes, (long long)L.total);
  if (const int rc = trainer_deterministic_check(trainer, n, /*traced=*/true, fn)) return rc;
  char* ws = (char*)workspace;
  float* ll = (float*)(ws + L.ll);
  float* G = (float*)(ws + L.G);
  float* w = (float*)(ws + L.w);
  double* cdf = (double*)(ws + L.cdf);
  int64_t* rows = (int64_t*)(ws + L.rows);
  int rc = gbnf_mixture_log_prob(fixed, x, n, n_fixed, rho_dev, ll, G, stream);
  if (rc == GBNF_OK) rc = gbnf_boosting_weights(G, n, beta, w, stream);
  if (rc == GBNF_OK) rc = launch_resample(w, n, u, n, rows, rows_out, cdf, G, stats_dev, (hipStream_t)stream, fn);
  if (rc) return rc;
  return gbnf_trainer_nll_step(trainer, x, n, rows, n, grads, exp_avg, exp_avg_sq, hyper, stats_dev, ws + L.step, L.step_bytes, stream);
}

int gbnf_mixture_rho_step(const gbnf_mixture* mix, const float* x, int64_t n, int32_t component, float* rho_dev, float step_size,
                          float* ll_workspace, float* stats_dev, void* stream) {
  const char* fn = "gbnf_mixture_rho_step";
  if (!mix || !x || !rho_dev || !ll_workspace || !stats_dev) return fail(GBNF_ERR_INVALID, "%s: null pointer", fn);
  if (n < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld (must be >= 1)", fn, (long long)n);
  int C = 0, d = 0;
  if (const int rc = mixture_shape(mix, &C, &d)) return rc;
  if (component < 1 || component >= C) return fail(GBNF_ERR_INVALID, "%s: component = %d outside [1,%d)", fn, component, C);
  if (const int rc = gbnf_mixture_component_log_prob(mix, x, n, 0, component + 1, ll_workspace, stream)) return rc;
  return rho_update_launch(fn, ll_workspace, n, (int)component, rho_dev, step_size, stats_dev, (hipStream_t)stream);
}

}  // extern "C"
