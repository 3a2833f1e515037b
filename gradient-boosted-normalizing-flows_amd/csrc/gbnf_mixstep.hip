// gbnf_mixstep.hip -- one joint likelihood step of the whole tabular mixture on the device (gfx950): every component moves on
//   L = -1/n sum_i G_i,   G_i = LSE_c(log_w_c + ll_c(x_i)),
// whose gradient with respect to component c's parameters is  -1/n sum_i r_ic d ll_c(x_i) / d theta_c  with the responsibilities
// r = softmax_c(log_w + ll)  (the identity behind the score, gbnf_score.hip, taken in theta instead of x).  Component c's backward
// therefore runs unchanged on the seeds g_z = (r_c / n) z_c, g_ldj = -r_c / n.  No reference counterpart: the reference trains one
// component at a time (density_experiment.py:340-374, its second pass `all_trained` included).
//
//   mix_seed_kernel      s_i = r_c[i] / n;  g_z[i][j] = s_i z_c[i][j];  g_ldj[i] = -s_i: one wave per 64 rows
//   mix_sums_kernel      per-workgroup f64 partial sums of G and of every row of r
//   mix_finish_kernel    one workgroup re-adds all partials in component and partial order: nll, the mean responsibilities, every
//                        component's gradient norm and the squared total the update kernels clip by
//
// All elementwise or reductions: no MFMA, no LDS beyond the block-sum tree, no atomics, plain vector stores.  The forward and backward
// sweeps are the trainers' own (gbnf_train.hip), the table's ll is score_seed_kernel's (gbnf_score.hip), r and G are
// gbnf_mixture_responsibilities' (gbnf_image_score.hip), the norm partials and the update are gbnf_opt.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/gbnf.h"
#include "gbnf_internal.h"
#include "gbnf_opt.h"

namespace gbnf {

constexpr int MS_THREADS = 256;                     // 4 waves
constexpr int MS_ROWS = 64;                         // rows per wave of the seed kernel
static_assert(OPT_MAX_PARTIALS <= MS_THREADS, "the finish re-adds the partial sums one per thread");

// the workgroup's 256 values added up in a fixed tree order (opt_block_sum's order, gbnf_opt.hip); every thread gets the sum
__device__ __forceinline__ double ms_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = MS_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

// A wave owns rows [row0, row0 + 64): 64 d contiguous floats of z and g_z, swept lane-contiguously (16 bytes per lane when VEC: both
// arrays 16-byte aligned; the wave's piece starts 256-byte aligned then), the tail by element; then one lane per row for g_ldj.
// s_i = r[i] * inv_n is formed once per element, so that r = 1 gives nll_seed_kernel's z * inv_n bit for bit.
template <bool VEC>
__global__ void __launch_bounds__(MS_THREADS) mix_seed_kernel(const float* __restrict__ z, const float* __restrict__ r, int64_t n, int d,
                                                              float inv_n, float* __restrict__ g_z, float* __restrict__ g_ldj) {
  const int lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * (MS_THREADS / 64) + (threadIdx.x >> 6)) * MS_ROWS;
  if (row0 >= n) return;
  const int rows = (int)(n - row0 < MS_ROWS ? n - row0 : MS_ROWS);
  const int cnt = rows * d;
  const float* zc = z + row0 * d;
  const float* rc = r + row0;
  float* gc = g_z + row0 * d;
  int e0 = 0;
  if constexpr (VEC) {
    const int nv = cnt >> 2;
    for (int v = lane; v < nv; v += 64) {
      const float4 a = reinterpret_cast<const float4*>(zc)[v];
      // one division per 16 bytes: the piece's first element, then (i, j) step along the row and wrap
      int i = (int)((unsigned)(4 * v) / (unsigned)d), j = 4 * v - i * d;
      const float in[4] = {a.x, a.y, a.z, a.w};
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        o[q] = (rc[i] * inv_n) * in[q];           // (i < rows: 4 v + q < cnt)
        if (++j == d) { j = 0; ++i; }
      }
      reinterpret_cast<float4*>(gc)[v] = make_float4(o[0], o[1], o[2], o[3]);
    }
    e0 = nv << 2;
  }
  for (int e = e0 + lane; e < cnt; e += 64) {
    const int i = (int)((unsigned)e / (unsigned)d);
    gc[e] = (rc[i] * inv_n) * zc[e];
  }
  if (lane < rows) g_ldj[row0 + lane] = -(rc[lane] * inv_n);
}

// partial[q][b] = the sum over workgroup b's rows of G (q == 0) or of row q - 1 of r: blockIdx.y = q, rows by grid stride
__global__ void __launch_bounds__(MS_THREADS) mix_sums_kernel(const float* __restrict__ G, const float* __restrict__ r, int64_t n,
                                                              double* __restrict__ partial) {
  __shared__ double lds[MS_THREADS];
  const int q = blockIdx.y;
  const float* src = q == 0 ? G : r + (int64_t)(q - 1) * n;
  const int64_t stride = (int64_t)gridDim.x * MS_THREADS;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; i < n; i += stride) acc += (double)src[i];
  const double s = ms_block_sum(acc, lds);
  if (threadIdx.x == 0) partial[(int64_t)q * OPT_MAX_PARTIALS + blockIdx.x] = s;
}

struct MixFinish {
  const double* sums;          // [1 + C][OPT_MAX_PARTIALS]: mix_sums_kernel's
  const double* grad;          // [C][OPT_MAX_PARTIALS]: grad_sqsum_kernel's, per component
  int n_sums, C;
  int n_grad[GBNF_WEIGHTS_MAX_COMPONENTS];
  double inv_n;
  double* total_sq;            // the one double every component's update kernel reads
  float* stats;                // [0] nll, [4 + c] rbar_c, [4 + C + c] norm_c  (the update kernels write [1..3])
};

// one workgroup: every sum re-added in component order, partials in index order through the fixed tree
__global__ void __launch_bounds__(MS_THREADS) mix_finish_kernel(const MixFinish p) {
  __shared__ double lds[MS_THREADS];
  const int tid = threadIdx.x;
  for (int q = 0; q <= p.C; ++q) {
    const double s = ms_block_sum(tid < p.n_sums ? p.sums[q * OPT_MAX_PARTIALS + tid] : 0.0, lds);
    if (tid == 0) {
      if (q == 0) p.stats[0] = (float)(-s * p.inv_n);
      else p.stats[4 + (q - 1)] = (float)(s * p.inv_n);
    }
  }
  double total = 0.0;
  for (int c = 0; c < p.C; ++c) {
    const double sq = ms_block_sum(tid < p.n_grad[c] ? p.grad[c * OPT_MAX_PARTIALS + tid] : 0.0, lds);
    total += sq;
    if (tid == 0) p.stats[4 + p.C + c] = (float)sqrt(sq);
  }
  if (tid == 0) *p.total_sq = total;
}

namespace {

int64_t ms_align256(int64_t b) { return (b + 255) / 256 * 256; }

// the caller's workspace of one mixture step, in 256-byte aligned pieces: z (C of them) | ldj | ll (C, n) | r (C, n) | G | g_z | g_ldj |
// C traces, each its trainer's size | one backward workspace (the largest) | the partial sums and the squared total
struct MixStepLayout {
  int64_t z, nx, ldj, ll, r, G, g_z, g_ldj, bwd, bwd_bytes, sums, grad, total_sq, total;
  int64_t trace[GBNF_WEIGHTS_MAX_COMPONENTS];
  int d;
};

// trainers checked non-null and C in range by the caller
int mix_step_layout(const char* fn, gbnf_trainer* const* trainers, int C, int64_t n, MixStepLayout* L) {
  int64_t tf[GBNF_WEIGHTS_MAX_COMPONENTS];
  int64_t bwd = 0;
  int d = 0;
  for (int c = 0; c < C; ++c) {
    TrainerOptView tv;
    if (const int rc = trainer_opt_view(trainers[c], &tv)) return rc;
    if (c == 0) d = tv.d;
    else if (tv.d != d) return fail(GBNF_ERR_INVALID, "%s: trainers[%d] has d = %d, trainers[0] d = %d", fn, c, tv.d, d);
    int64_t b = 0;
    int rc = gbnf_trainer_trace_floats(trainers[c], n, &tf[c]);
    if (rc == GBNF_OK) rc = gbnf_trainer_workspace_bytes(trainers[c], n, &b);
    if (rc) return rc;
    bwd = std::max(bwd, b);
  }
  const int64_t nx = ms_align256(n * (int64_t)d * 4), nn = ms_align256(n * 4), cn = ms_align256((int64_t)C * n * 4);
  int64_t off = 0;
  L->z = off; L->nx = nx; off += (int64_t)C * nx;
  L->ldj = off; off += nn;
  L->ll = off; off += cn;
  L->r = off; off += cn;
  L->G = off; off += nn;
  L->g_z = off; off += nx;
  L->g_ldj = off; off += nn;
  for (int c = 0; c < C; ++c) { L->trace[c] = off; off += ms_align256(tf[c] * 4); }
  L->bwd = off; L->bwd_bytes = bwd; off += ms_align256(bwd);
  L->sums = off; off += ms_align256((int64_t)(1 + C) * OPT_MAX_PARTIALS * (int64_t)sizeof(double));
  L->grad = off; off += ms_align256((int64_t)C * OPT_MAX_PARTIALS * (int64_t)sizeof(double));
  L->total_sq = off; off += 256;
  L->total = off;
  L->d = d;
  return GBNF_OK;
}

// what both calls refuse of the handle array before anything else (GBNF_ERR_INVALID)
int check_mix_step_trainers(const char* fn, gbnf_trainer* const* trainers, int32_t n_components, int64_t n) {
  if (!trainers) return fail(GBNF_ERR_INVALID, "%s: trainers is null", fn);
  if (n_components < 1 || n_components > GBNF_WEIGHTS_MAX_COMPONENTS)
    return fail(GBNF_ERR_INVALID, "%s: n_components = %d (must be in [1, %d])", fn, (int)n_components, GBNF_WEIGHTS_MAX_COMPONENTS);
  if (n < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld (must be >= 1)", fn, (long long)n);
  for (int c = 0; c < n_components; ++c) {
    if (!trainers[c]) return fail(GBNF_ERR_INVALID, "%s: trainers[%d] is null", fn, c);
    for (int b = 0; b < c; ++b)
      if (trainers[b] == trainers[c])
        return fail(GBNF_ERR_INVALID, "%s: trainers[%d] and trainers[%d] are the same trainer: a component is stepped once", fn, b, c);
  }
  return GBNF_OK;
}

}  // namespace

}  // namespace gbnf

using namespace gbnf;

extern "C" {

int gbnf_mixture_step_workspace_bytes(gbnf_trainer* const* trainers, int32_t n_components, int64_t n, int64_t* bytes) {
  const char* fn = "gbnf_mixture_step_workspace_bytes";
  if (!bytes) return fail(GBNF_ERR_INVALID, "%s: bytes is null", fn);
  if (const int rc = check_mix_step_trainers(fn, trainers, n_components, n)) return rc;
  MixStepLayout L;
  if (const int rc = mix_step_layout(fn, trainers, n_components, n, &L)) return rc;
  *bytes = L.total;
  return GBNF_OK;
}

int gbnf_mixture_nll_step(gbnf_trainer* const* trainers, int32_t n_components, const float* log_w, const float* x, int64_t n,
                          float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const gbnf_opt_hyper* hypers,
                          float* stats_dev, float* G_or_null, float* r_or_null, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "gbnf_mixture_nll_step";
  if (!grads || !exp_avg || !exp_avg_sq || !hypers) return fail(GBNF_ERR_INVALID, "%s: grads / exp_avg / exp_avg_sq / hypers is null", fn);
  if (!log_w || !x || !stats_dev || !workspace) return fail(GBNF_ERR_INVALID, "%s: log_w / x / stats_dev / workspace is null", fn);
  if (const int rc = check_mix_step_trainers(fn, trainers, n_components, n)) return rc;
  const int C = (int)n_components;
  for (int c = 0; c < C; ++c) {
    if (!grads[c]) return fail(GBNF_ERR_INVALID, "%s: grads[%d] is null", fn, c);
    if (const int rc = check_hyper(fn, &hypers[c], exp_avg[c], exp_avg_sq[c])) return rc;
    if (hypers[c].kind != hypers[0].kind)
      return fail(GBNF_ERR_INVALID, "%s: hypers[%d].kind = %d, hypers[0].kind = %d: one optimiser kind per call", fn, c, hypers[c].kind,
                  hypers[0].kind);
    if (!(hypers[c].max_grad_norm == hypers[0].max_grad_norm))
      return fail(GBNF_ERR_INVALID, "%s: hypers[%d].max_grad_norm = %g, hypers[0].max_grad_norm = %g: one clip coefficient spans all "
                  "components", fn, c, (double)hypers[c].max_grad_norm, (double)hypers[0].max_grad_norm);
  }
  MixStepLayout L;
  if (const int rc = mix_step_layout(fn, trainers, C, n, &L)) return rc;        // (also: one d)
  if (workspace_bytes < L.total)
    return fail(GBNF_ERR_INVALID, "%s: workspace too small: %lld bytes < %lld (gbnf_mixture_step_workspace_bytes)", fn,
                (long long)workspace_bytes, (long long)L.total);
  OptUpdateView view[GBNF_WEIGHTS_MAX_COMPONENTS];
  for (int c = 0; c < C; ++c) {
    TrainerOptView tv;
    if (const int rc = trainer_opt_view(trainers[c], &tv)) return rc;
    view[c] = OptUpdateView{tv.regions_dev, tv.n_regions, tv.grad_floats};
    if (tv.batch_stats)
      return fail(GBNF_ERR_UNSUPPORTED, "%s: trainers[%d] is in batch-statistics mode: the mixture step runs on the running statistics "
                  "(gbnf_trainer_set_batch_stats(0))", fn, c);
  }
  for (int c = 0; c < C; ++c)      // (the deterministic-mode refusals of every component's backward, before the first launch)
    if (const int rc = trainer_deterministic_check(trainers[c], n, /*traced=*/true, fn)) return rc;

  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* ldj = (float*)(ws + L.ldj);
  float* ll = (float*)(ws + L.ll);
  float* r = (float*)(ws + L.r);
  float* G = (float*)(ws + L.G);
  float* g_z = (float*)(ws + L.g_z);
  float* g_ldj = (float*)(ws + L.g_ldj);
  double* sums = (double*)(ws + L.sums);
  double* grad_partial = (double*)(ws + L.grad);
  double* total_sq = (double*)(ws + L.total_sq);
  const int d = L.d;
  auto z_of = [&](int c) { return (float*)(ws + L.z + (int64_t)c * L.nx); };
  auto trace_of = [&](int c) { return (float*)(ws + L.trace[c]); };
  // 1. every component's traced forward and its row of the table
  for (int c = 0; c < C; ++c) {
    if (const int rc = gbnf_trainer_forward(trainers[c], x, n, z_of(c), ldj, trace_of(c), stream)) return rc;
    score_launch_ll(z_of(c), ldj, n, d, ll + (int64_t)c * n, s);
  }
  // 2. the responsibilities and log p
  if (const int rc = gbnf_mixture_responsibilities(ll, log_w, C, n, r, G, stream)) return rc;
  hipError_t e = hipSuccess;
  if (G_or_null != nullptr) e = hipMemcpyAsync(G_or_null, G, (size_t)n * 4, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && r_or_null != nullptr) e = hipMemcpyAsync(r_or_null, r, (size_t)C * n * 4, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s: the copy of G / r failed: %s", fn, hipGetErrorString(e));
  // 3. the partial sums of G and of every row of r
  const unsigned nb = opt_partial_blocks(n);
  hipLaunchKernelGGL(mix_sums_kernel, dim3(nb, (unsigned)(C + 1)), dim3(MS_THREADS), 0, s, (const float*)G, (const float*)r, n, sums);
  // 4. per component, in order: the seed, the zeroed gradient, the backward on its own trace, the squared-norm partials
  MixFinish fin{};
  const float inv_n = 1.0f / (float)n;
  const int64_t rows_per_block = (int64_t)MS_ROWS * (MS_THREADS / 64);
  const dim3 seed_grid((unsigned)((n + rows_per_block - 1) / rows_per_block));
  for (int c = 0; c < C; ++c) {
    const float* zc = z_of(c);
    const float* rc_ = r + (int64_t)c * n;
    if ((((uintptr_t)zc | (uintptr_t)g_z) & 15u) == 0u)
      hipLaunchKernelGGL(mix_seed_kernel<true>, seed_grid, dim3(MS_THREADS), 0, s, zc, rc_, n, d, inv_n, g_z, g_ldj);
    else
      hipLaunchKernelGGL(mix_seed_kernel<false>, seed_grid, dim3(MS_THREADS), 0, s, zc, rc_, n, d, inv_n, g_z, g_ldj);
    e = hipMemsetAsync(grads[c], 0, (size_t)view[c].grad_floats * 4, s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
    if (const int rc = gbnf_trainer_backward(trainers[c], x, n, trace_of(c), g_z, g_ldj, nullptr, grads[c], ws + L.bwd, L.bwd_bytes, stream))
      return rc;
    fin.n_grad[c] = opt_launch_grad_sqsum(grads[c], view[c].grad_floats, grad_partial + (int64_t)c * OPT_MAX_PARTIALS, stream);
  }
  // 5. nll, the mean responsibilities, the norms, the squared total
  fin.sums = sums; fin.grad = grad_partial; fin.n_sums = (int)nb; fin.C = C;
  fin.inv_n = 1.0 / (double)n;
  fin.total_sq = total_sq; fin.stats = stats_dev;
  hipLaunchKernelGGL(mix_finish_kernel, dim3(1), dim3(MS_THREADS), 0, s, fin);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  // 6. every component's update on the one clip coefficient (each writes the same stats[1..3])
  for (int c = 0; c < C; ++c)
    if (const int rc = opt_launch_update_from(fn, view[c], grads[c], exp_avg[c], exp_avg_sq[c], &hypers[c], stats_dev, total_sq, 1, nullptr, 0,
                                              0.0, 0.0, stream))
      return rc;
  return GBNF_OK;
}

}  // extern "C"
