// gbnf_weights.hip -- all mixture weights at once (gfx950): EM for the weights of  G(x) = sum_c w_c g_c(x)  with the components fixed,
// over a cached (C, n) table of per-component log-likelihoods (what gbnf_mixture_component_log_prob[_strided] or an image call wrote).
// The fully-corrective step of boosting; it has no counterpart in the reference, whose update_rho (models/boosted_flow.py:141-207)
// moves one rho along the sign of a difference of two log-likelihoods and never revisits earlier weights.
//
//   weights_em_kernel      launch k = 0 .. max_iters + 1.  Every workgroup first re-adds the partial sums of launch k - 1 in index order
//                          (so all of them hold the same bits), decides whether evaluation k - 1 was the stopping one, and otherwise
//                          forms w^(k) and evaluates it: per row G_i = LSE_c(log w_c + ll[c][i]) and r_c = exp(log w_c + ll[c][i] - G_i),
//                          summed per workgroup.  Two partial buffers and two control blocks alternate between launches: a launch reads
//                          what the one before wrote and writes what the one after reads, so nothing is read and written by one launch.
//                          "Stopped" is a word of the control block: every launch behind the stopping one copies it on and returns.
//   weights_to_rho_kernel  rho[c] = clamp(w_c * sum(rho[0..C)), rho_min, rho_max), one wave
//
// Launch-latency sized like gbnf_eval.hip: no matrix pipe, no LDS opt-in.  Every sum is f64 in an order that depends on the sizes alone
// (across a wave, then over the rows a wave walks, then over the 4 waves, then over the workgroups in index order; no atomics), so the
// same call gives the same bits.  Lanes are on rows and the table is read along n; a component's r_c is reduced across the wave before
// it meets the wave's LDS accumulator, so no per-thread array is indexed by a runtime c (it would live in scratch).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gbnf.h"
#include "gbnf_internal.h"

namespace gbnf {

constexpr int WT_THREADS = 256;
constexpr int WT_WAVES = WT_THREADS / 64;
constexpr int WT_ROWS_PER_WG = 4 * WT_THREADS;          // rows a workgroup takes before the grid-stride loop wraps (as gbnf_eval.hip)
constexpr int WT_MAX_PARTIALS = 256;
constexpr int WT_MAX_C = GBNF_WEIGHTS_MAX_COMPONENTS;
// one control block (doubles):  [0] stopped  [1] bad rho  [2] L of the last finished evaluation  [3] L_0  [8 .. 8 + C) the weights in use
constexpr int WT_CTRL_DOUBLES = 80;
constexpr int64_t WT_CTRL_BYTES = 2LL * WT_CTRL_DOUBLES * sizeof(double);
static_assert(WT_CTRL_DOUBLES >= 8 + WT_MAX_C, "a control block holds the weights");
static_assert(WT_CTRL_BYTES % 256 == 0, "the partial sums start 256-byte aligned");
static_assert(GBNF_WEIGHTS_STATE_DOUBLES == 8 + WT_MAX_C, "the state holds 8 words and the weights");

// partial sums of one launch: row 0 = sum of G_i, row 1 = rows used, row 2 + c = S_c; WT_MAX_PARTIALS entries per row
static int64_t weights_partial_doubles(int C) { return (int64_t)(C + 2) * WT_MAX_PARTIALS; }
static int64_t weights_workspace_bytes(int C) { return WT_CTRL_BYTES + 2 * weights_partial_doubles(C) * (int64_t)sizeof(double); }

static unsigned weights_grid(int64_t n) {
  int64_t nb = (n + WT_ROWS_PER_WG - 1) / WT_ROWS_PER_WG;
  if (nb < 1) nb = 1;
  if (nb > WT_MAX_PARTIALS) nb = WT_MAX_PARTIALS;
  return (unsigned)nb;
}

// the wave's 64 values added in a fixed tree order; lane 0 holds the sum
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__global__ void __launch_bounds__(WT_THREADS) weights_em_kernel(const float* __restrict__ ll, int64_t stride, int C, int64_t n,
                                                                const float* __restrict__ rho, int k, int max_iters, double tol,
                                                                int n_partial, double* __restrict__ ctrl2, double* __restrict__ part2,
                                                                double* __restrict__ state) {
  __shared__ double sh_w[WT_MAX_C];                 // w^(k), then log w^(k)
  __shared__ double sh_sum[2];                      // launch k - 1: sum of G_i, rows used
  __shared__ double sh_acc[WT_WAVES][WT_MAX_C + 2]; // per wave: S_c, sum of G_i, rows used
  __shared__ int sh_stop;
  const int tid = threadIdx.x;
  const double* __restrict__ prev = ctrl2 + (size_t)((k + 1) & 1) * WT_CTRL_DOUBLES;       // written by launch k - 1
  double* __restrict__ cur = ctrl2 + (size_t)(k & 1) * WT_CTRL_DOUBLES;
  const double* __restrict__ pin = part2 + (size_t)((k + 1) & 1) * (size_t)(C + 2) * WT_MAX_PARTIALS;
  double* __restrict__ pout = part2 + (size_t)(k & 1) * (size_t)(C + 2) * WT_MAX_PARTIALS;
  const bool first_wg = blockIdx.x == 0;

  if (k == 0) {
    // w^(0) = rho / sum(rho), in double from the float32 entries, in index order
    if (tid == 0) {
      double total = 0.0;
      bool bad = false;
      for (int c = 0; c < C; ++c) {
        const double r = (double)rho[c];
        if (!(fabs(r) < (double)INFINITY) || r < 0.0) bad = true;
        total = __dadd_rn(total, r);
      }
      if (!(total > 0.0)) bad = true;
      for (int c = 0; c < C; ++c) sh_w[c] = (double)rho[c] / total;
      if (first_wg) {
        cur[0] = 0.0; cur[1] = bad ? 1.0 : 0.0; cur[2] = 0.0; cur[3] = 0.0;
        for (int c = 0; c < C; ++c) cur[8 + c] = sh_w[c];
      }
    }
    __syncthreads();
  } else {
    if (prev[0] != 0.0) {                                     // stopped: hand the word on and return at once
      if (first_wg && tid == 0) cur[0] = 1.0;
      return;
    }
    // the partial sums of evaluation t = k - 1, each row added in index order by one thread (every workgroup: the same bits)
    if (tid < C + 2) {
      const double* __restrict__ row = pin + (size_t)tid * WT_MAX_PARTIALS;
      double s = 0.0;
      for (int b = 0; b < n_partial; ++b) s += row[b];
      if (tid < 2) sh_sum[tid] = s; else sh_w[tid - 2] = s;
    }
    __syncthreads();
    if (tid == 0) {
      const int t = k - 1;
      const double used = sh_sum[1];
      const double L = sh_sum[0] / used;
      const bool bad = prev[1] != 0.0 || !(used > 0.0);
      const double delta = t >= 1 ? fabs(L - prev[2]) : 0.0;
      const bool conv = !bad && t >= 1 && tol > 0.0 && delta <= tol;
      const bool stop = bad || conv || t >= max_iters;
      sh_stop = stop ? 1 : 0;
      if (first_wg) {
        const double L0 = t == 0 ? L : prev[3];
        if (stop) {
          state[0] = bad ? 0.0 : (double)t;
          state[1] = conv ? 1.0 : 0.0;
          state[2] = used;
          state[3] = (double)n - used;
          state[4] = L0;
          state[5] = L;
          state[6] = delta;
          state[7] = bad ? 1.0 : 0.0;
          for (int c = 0; c < C; ++c) state[8 + c] = prev[8 + c];
          cur[0] = 1.0;
        } else {
          cur[0] = 0.0; cur[1] = 0.0; cur[2] = L; cur[3] = L0;
          for (int c = 0; c < C; ++c) cur[8 + c] = sh_w[c] / used;
        }
      }
    }
    __syncthreads();
    if (sh_stop) return;
    if (tid < C) sh_w[tid] = sh_w[tid] / sh_sum[1];           // w^(k) = S / N_used
    __syncthreads();
  }
  if (tid < C) sh_w[tid] = log(sh_w[tid]);                    // log 0 = -inf: a weight of 0 is a fixed point
  for (int j = tid; j < WT_WAVES * (WT_MAX_C + 2); j += WT_THREADS) (&sh_acc[0][0])[j] = 0.0;
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  const int64_t step = (int64_t)gridDim.x * WT_THREADS;
  double sG = 0.0, cnt = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * WT_THREADS; base < n; base += step) {      // (the bound is the same for the whole workgroup)
    const int64_t i = base + tid;
    const bool in = i < n;
    // the row's largest term, and whether the row counts: no NaN, no +inf, not all -inf
    double m = -(double)INFINITY;
    bool ok = in, any = false;
    for (int c = 0; c < C; ++c) {
      const float v = in ? ll[(int64_t)c * stride + i] : 0.0f;
      if (v != v || v == INFINITY) ok = false;
      if (v > -INFINITY) any = true;
      const double a = sh_w[c] + (double)v;
      if (a > m) m = a;
    }
    ok = ok && any;
    const bool live = ok && m > -(double)INFINITY;             // (every supported component at weight 0: G = -inf, r = 0)
    double s = 0.0;
    if (live)
      for (int c = 0; c < C; ++c) s = __dadd_rn(s, exp(sh_w[c] + (double)ll[(int64_t)c * stride + i] - m));
    const double G = live ? m + log(s) : -(double)INFINITY;
    if (ok) { sG += G; cnt += 1.0; }
    for (int c = 0; c < C; ++c) {
      const double r = live ? exp(sh_w[c] + (double)ll[(int64_t)c * stride + i] - G) : 0.0;
      const double w = wave_sum(r);
      if (lane == 0) sh_acc[wave][c] += w;
    }
  }
  {
    const double a = wave_sum(sG), b = wave_sum(cnt);
    if (lane == 0) { sh_acc[wave][WT_MAX_C] = a; sh_acc[wave][WT_MAX_C + 1] = b; }
  }
  __syncthreads();
  if (tid < C + 2) {
    const int col = tid < 2 ? WT_MAX_C + tid : tid - 2;
    double s = sh_acc[0][col];
#pragma unroll
    for (int w = 1; w < WT_WAVES; ++w) s += sh_acc[w][col];
    pout[(size_t)tid * WT_MAX_PARTIALS + blockIdx.x] = s;
  }
}

// One wave.  Every lane adds the old rho[0..C) in double in index order (the same bits), then lane c < C writes its entry; the number
// of clamped entries goes into state[7] as 2 * count (bit 0 of that word is bad_start, and a bad start writes nothing).
__global__ void __launch_bounds__(64) weights_to_rho_kernel(double* __restrict__ state, int C, float rho_min, float rho_max,
                                                            float* __restrict__ rho) {
  const int c = threadIdx.x;
  if (fmod(state[7], 2.0) != 0.0) return;
  double S = 0.0;
  for (int j = 0; j < C; ++j) S = __dadd_rn(S, (double)rho[j]);
  __syncthreads();                                     // every lane has read the old entries
  bool clamped = false;
  if (c < C) {
    const float v = (float)(state[8 + c] * S);
    clamped = v < rho_min || v > rho_max;
    rho[c] = fminf(fmaxf(v, rho_min), rho_max);
  }
  const unsigned long long hit = __ballot(clamped);
  if (c == 0) state[7] += 2.0 * (double)__popcll(hit);
}

}  // namespace gbnf

using namespace gbnf;

extern "C" {

int gbnf_weights_em_workspace_bytes(int32_t n_components, int64_t n, int64_t* bytes) {
  const char* fn = "gbnf_weights_em_workspace_bytes";
  if (!bytes) return fail(GBNF_ERR_INVALID, "%s: bytes is null", fn);
  if (n < 0) return fail(GBNF_ERR_INVALID, "%s: n = %lld (must be >= 0)", fn, (long long)n);
  if (n_components < 1 || n_components > WT_MAX_C)
    return fail(GBNF_ERR_INVALID, "%s: n_components = %d outside [1,%d]", fn, (int)n_components, WT_MAX_C);
  *bytes = weights_workspace_bytes(n_components);
  return GBNF_OK;
}

int gbnf_weights_em(const float* ll, int64_t ll_row_stride, int32_t n_components, int64_t n, const float* rho_dev, int32_t max_iters,
                    double tol, double* state_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "gbnf_weights_em";
  if (!ll || !rho_dev || !state_dev || !workspace) return fail(GBNF_ERR_INVALID, "%s: ll / rho_dev / state_dev / workspace is null", fn);
  if (n < 0) return fail(GBNF_ERR_INVALID, "%s: n = %lld (must be >= 0)", fn, (long long)n);
  if (n_components < 1 || n_components > WT_MAX_C)
    return fail(GBNF_ERR_INVALID, "%s: n_components = %d outside [1,%d]", fn, (int)n_components, WT_MAX_C);
  if (ll_row_stride < n) return fail(GBNF_ERR_INVALID, "%s: ll_row_stride = %lld < n = %lld", fn, (long long)ll_row_stride, (long long)n);
  if (max_iters < 0) return fail(GBNF_ERR_INVALID, "%s: max_iters = %d (must be >= 0)", fn, (int)max_iters);
  if (tol != tol) return fail(GBNF_ERR_INVALID, "%s: tol is NaN", fn);
  if (workspace_bytes < weights_workspace_bytes(n_components))
    return fail(GBNF_ERR_INVALID, "%s: workspace of %lld bytes < %lld (gbnf_weights_em_workspace_bytes)", fn, (long long)workspace_bytes,
                (long long)weights_workspace_bytes(n_components));
  hipStream_t s = (hipStream_t)stream;
  double* ctrl = (double*)workspace;
  double* part = (double*)((char*)workspace + WT_CTRL_BYTES);
  const unsigned nb = weights_grid(n);
  // evaluations k = 0 .. max_iters on the whole grid; launch max_iters + 1 only finalises the last of them: one workgroup
  for (int64_t k = 0; k <= (int64_t)max_iters + 1; ++k)
    hipLaunchKernelGGL(weights_em_kernel, dim3(k == (int64_t)max_iters + 1 ? 1u : nb), dim3(WT_THREADS), 0, s, ll, ll_row_stride,
                       (int)n_components, n, rho_dev, (int)k, (int)max_iters, tol, (int)nb, ctrl, part, state_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

int gbnf_weights_to_rho(double* state_dev, int32_t n_components, float rho_min, float rho_max, float* rho_dev, void* stream) {
  const char* fn = "gbnf_weights_to_rho";
  if (!state_dev || !rho_dev) return fail(GBNF_ERR_INVALID, "%s: state_dev / rho_dev is null", fn);
  if (n_components < 1 || n_components > WT_MAX_C)
    return fail(GBNF_ERR_INVALID, "%s: n_components = %d outside [1,%d]", fn, (int)n_components, WT_MAX_C);
  if (!(rho_min <= rho_max)) return fail(GBNF_ERR_INVALID, "%s: rho_min = %g, rho_max = %g (need rho_min <= rho_max)", fn, rho_min, rho_max);
  hipLaunchKernelGGL(weights_to_rho_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state_dev, (int)n_components, rho_min, rho_max,
                     rho_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

}  // extern "C"
