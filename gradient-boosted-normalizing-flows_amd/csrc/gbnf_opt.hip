// gbnf_opt.hip -- the tail of a training step on the device (gfx950): what the reference's driver does in eager PyTorch between
// and behind the library's forward / backward calls (density_experiment.py:340-374, compute_kl_pq_loss :606-674):
//
//   gather_rows_kernel    x[reweighted_idx]                                    (density_experiment.py:643-644)
//   nll_seed_kernel       nll = mean(-(log_normal_standard(z) + ldj)) and its autograd seed g_z = z / n, g_ldj = -1 / n
//                         (:647-649, utils/distributions.py:44-60); per-workgroup partial sums
//   bn_running_kernel     BatchNorm.running_mean / running_var in train() mode  (models/layers.py:339-344)
//   grad_sqsum_kernel     per-workgroup partial sums of the squared gradient    (clip_grad_norm_, :363-364)
//   opt_update_kernel     the clip coefficient and optim.AdamW / optim.SGD on the LIVE parameter tensors
//                         (optimization/optimizers.py:54-65, optimizer.step() :374)
//
// All of it is latency- and bandwidth-bound (MINIBOONE K = 5: 3e5 parameters, ~8 MB per update): few launches, no host read, no
// synchronisation.  Reductions: a producer kernel writes at most OPT_MAX_PARTIALS per-workgroup sums (f64); the consumer, behind it in
// stream order, re-adds them in a fixed order in f64 -- every workgroup of the update kernel does so for itself.  No float atomics, no
// cross-workgroup fence: the norm, the coefficient and the loss are bit-identical from run to run for the same inputs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/gbnf.h"
#include "gbnf_internal.h"
#include "gbnf_opt.h"

namespace gbnf {

constexpr int OPT_THREADS = 256;
constexpr int OPT_ITEMS = 4;                     // flat entries per thread of the update kernel
static_assert(OPT_MAX_PARTIALS <= OPT_THREADS, "a workgroup re-adds the partial sums one per thread");

// the workgroup's 256 values added up in a fixed tree order; every thread gets the sum
__device__ __forceinline__ double opt_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = OPT_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

// workgroups of a producer over `work` entries: one per 1024 entries, at most OPT_MAX_PARTIALS (a function of the size alone)
unsigned opt_partial_blocks(int64_t work) {
  const int64_t b = (work + 4 * OPT_THREADS - 1) / (4 * OPT_THREADS);
  return (unsigned)(b < 1 ? 1 : (b > OPT_MAX_PARTIALS ? OPT_MAX_PARTIALS : b));
}

// out[i, :] = x[rows[i], :].  An index outside [0, n_x) is clamped to it (the call cannot report it without a host read).
__global__ void __launch_bounds__(OPT_THREADS) gather_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ rows, int64_t n_x,
                                                                  int64_t n, int d, float* __restrict__ out) {
  const int64_t total = n * d, stride = (int64_t)gridDim.x * OPT_THREADS;
  for (int64_t e = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; e < total; e += stride) {
    const int64_t i = e / d;
    const int j = (int)(e - i * d);
    int64_t r = rows[i];
    r = r < 0 ? 0 : (r >= n_x ? n_x - 1 : r);
    out[e] = x[r * d + j];
  }
}

// partial[b] = sum over this workgroup's entries of 0.5 z^2 (all of z) - ldj (all rows); g_z = z / n, g_ldj = -1 / n
__global__ void __launch_bounds__(OPT_THREADS) nll_seed_kernel(const float* __restrict__ z, const float* __restrict__ ldj, int64_t n, int d,
                                                               float inv_n, float* __restrict__ g_z, float* __restrict__ g_ldj,
                                                               double* __restrict__ partial) {
  __shared__ double lds[OPT_THREADS];
  const int64_t total = n * d, stride = (int64_t)gridDim.x * OPT_THREADS, first = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  double acc = 0.0;
  for (int64_t e = first; e < total; e += stride) {
    const float v = z[e];
    acc += 0.5 * (double)v * (double)v;
    g_z[e] = v * inv_n;
  }
  for (int64_t i = first; i < n; i += stride) {
    acc -= (double)ldj[i];
    g_ldj[i] = -inv_n;
  }
  const double s = opt_block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// running = momentum * running + (1 - momentum) * batch, in the reference's operation order (mul_, then add_ of the scaled statistics)
__global__ void __launch_bounds__(64) bn_running_kernel(const OptBnTable tab, int d, float momentum) {
  const int k = blockIdx.x, j = threadIdx.x;
  if (j >= d) return;
  const float w = 1.0f - momentum;
  tab.mean[k][j] = __fadd_rn(__fmul_rn(tab.mean[k][j], momentum), __fmul_rn(tab.bmean[k][j], w));
  tab.var[k][j] = __fadd_rn(__fmul_rn(tab.var[k][j], momentum), __fmul_rn(tab.bvar[k][j], w));
}

__global__ void __launch_bounds__(OPT_THREADS) grad_sqsum_kernel(const float* __restrict__ g, int64_t ng, double* __restrict__ partial) {
  __shared__ double lds[OPT_THREADS];
  const int64_t stride = (int64_t)gridDim.x * OPT_THREADS;
  double acc = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; e < ng; e += stride) {
    const double v = (double)g[e];
    acc += v * v;
  }
  const double s = opt_block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

struct OptLaunch {
  const OptRegion* regions;     // sorted by flat offset; reserved regions are not listed
  int n_regions, kind;
  int64_t ng;
  const float* grads;
  float* m;
  float* v;
  const double* grad_partial;   // grad_sqsum_kernel's sums
  int n_grad_partial;
  const double* nll_partial;    // nll_seed_kernel's sums, or null (gbnf_trainer_apply_update)
  int n_nll_partial;
  double nll_scale, nll_const;  // nll = sum * scale + const
  float max_norm;               // <= 0: no clipping
  float decay;                  // AdamW: 1 - lr wd
  float lr, wd;                 // SGD
  float b1, b2, omb1, omb2;     // AdamW: the betas and 1 - beta (rounded from double, see decimal_meant)
  float step_size, bc2_sqrt, eps;     // AdamW: step_size = lr / (1 - b1^step), bc2_sqrt = sqrt(1 - b2^step)
  float* stats;
};

// the last region whose offset is <= i, or -1
__device__ __forceinline__ int opt_find_region(const OptRegion* __restrict__ regions, int n, int64_t i) {
  int lo = -1, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (regions[mid].off <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(OPT_THREADS) opt_update_kernel(const OptLaunch p) {
  __shared__ double lds[OPT_THREADS];
  const int tid = threadIdx.x;
  const double sq = opt_block_sum(tid < p.n_grad_partial ? p.grad_partial[tid] : 0.0, lds);
  const double norm = sqrt(sq);
  float coef = 1.0f;
  if (p.max_norm > 0.0f) {
    const double c = (double)p.max_norm / (norm + 1e-6);
    coef = c < 1.0 ? (float)c : 1.0f;
  }
  if (blockIdx.x == 0) {
    if (p.nll_partial != nullptr) {
      const double s = opt_block_sum(tid < p.n_nll_partial ? p.nll_partial[tid] : 0.0, lds);
      if (tid == 0) p.stats[0] = (float)(s * p.nll_scale + p.nll_const);
    }
    if (tid == 0) {
      p.stats[1] = (float)norm;
      p.stats[2] = coef;
      p.stats[3] = 0.0f;
    }
  }
  // this workgroup's OPT_THREADS * OPT_ITEMS consecutive flat entries; a thread's entries ascend, so its region index only moves forward
  int64_t i = (int64_t)blockIdx.x * (OPT_THREADS * OPT_ITEMS) + tid;
  if (i >= p.ng) return;
  int r = opt_find_region(p.regions, p.n_regions, i);
  OptRegion reg = r >= 0 ? p.regions[r] : OptRegion{nullptr, 0, 0};
#pragma unroll
  for (int it = 0; it < OPT_ITEMS; ++it, i += OPT_THREADS) {
    if (i >= p.ng) break;
    bool moved = false;
    while (r + 1 < p.n_regions && p.regions[r + 1].off <= i) { ++r; moved = true; }
    if (moved) reg = p.regions[r];
    if (r < 0 || i >= reg.off + reg.len) continue;        // a reserved region: no tensor behind it
    float* pp = reg.p + (i - reg.off);
    const float g = coef * p.grads[i];
    float w = *pp;
    if (p.kind == GBNF_OPT_ADAMW) {
      w *= p.decay;
      const float m = p.b1 * p.m[i] + p.omb1 * g;
      const float v = p.b2 * p.v[i] + p.omb2 * g * g;
      p.m[i] = m;
      p.v[i] = v;
      w -= p.step_size * (m / (sqrtf(v) / p.bc2_sqrt + p.eps));
    } else {
      w -= p.lr * (g + p.wd * w);
    }
    *pp = w;
  }
}

// The double a float hyper-parameter stands for: the shortest decimal that rounds to it (0.999f -> 0.999).  torch.optim computes
// 1 - beta2 and the bias corrections from the Python float 0.999; 1 - (double)0.999f is off by 1.3e-5 of its value (cancellation), which
// would show in exp_avg_sq at that relative size.
static double decimal_meant(float f) {
  if (!std::isfinite(f)) return (double)f;
  char buf[40];
  for (int digits = 1; digits <= 9; ++digits) {
    std::snprintf(buf, sizeof(buf), "%.*g", digits, (double)f);
    if (std::strtof(buf, nullptr) == f) return std::strtod(buf, nullptr);
  }
  return (double)f;
}

int check_hyper(const char* fn, const gbnf_opt_hyper* h, const float* m, const float* v) {
  if (h == nullptr) return fail(GBNF_ERR_INVALID, "%s: hyper is null", fn);
  if (h->kind != GBNF_OPT_SGD && h->kind != GBNF_OPT_ADAMW) return fail(GBNF_ERR_INVALID, "%s: unknown optimiser kind %d", fn, h->kind);
  if (h->kind == GBNF_OPT_ADAMW) {
    if (h->step <= 0) return fail(GBNF_ERR_INVALID, "%s: AdamW needs the 1-based index of this update (step = %lld)", fn, (long long)h->step);
    if (m == nullptr || v == nullptr) return fail(GBNF_ERR_INVALID, "%s: AdamW needs exp_avg and exp_avg_sq", fn);
  }
  return GBNF_OK;
}

// the squared-norm partials of a flat gradient buffer: one launch; returns how many partials it leaves (a function of the size alone)
int opt_launch_grad_sqsum(const float* grads, int64_t grad_floats, double* partials, void* stream) {
  const unsigned gb = opt_partial_blocks(grad_floats);
  hipLaunchKernelGGL(grad_sqsum_kernel, dim3(gb), dim3(OPT_THREADS), 0, (hipStream_t)stream, grads, grad_floats, partials);
  return (int)gb;
}

// clip coefficient + update (+ the loss of nll_step) from squared-norm sums that are in memory already -- one launch
int opt_launch_update_from(const char* fn, const OptUpdateView& tv, const float* grads, float* m, float* v, const gbnf_opt_hyper* h,
                           float* stats, const double* grad_partial, int n_grad_partial, const double* nll_partial, int n_nll_partial,
                           double nll_scale, double nll_const, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  OptLaunch p{};
  p.regions = tv.regions_dev; p.n_regions = tv.n_regions; p.kind = h->kind; p.ng = tv.grad_floats;
  p.grads = grads; p.m = m; p.v = v;
  p.grad_partial = grad_partial; p.n_grad_partial = n_grad_partial;
  p.nll_partial = nll_partial; p.n_nll_partial = n_nll_partial;
  if (nll_partial != nullptr) {
    p.nll_scale = nll_scale;
    p.nll_const = nll_const;
  }
  p.max_norm = h->max_grad_norm;
  p.lr = h->lr; p.wd = h->weight_decay; p.b1 = h->beta1; p.b2 = h->beta2; p.eps = h->eps;
  if (h->kind == GBNF_OPT_ADAMW) {        // the scalars in double precision, as torch.optim computes them on the host
    const double lr = decimal_meant(h->lr), b1 = decimal_meant(h->beta1), b2 = decimal_meant(h->beta2);
    p.decay = (float)(1.0 - lr * decimal_meant(h->weight_decay));
    p.omb1 = (float)(1.0 - b1);
    p.omb2 = (float)(1.0 - b2);
    p.step_size = (float)(lr / (1.0 - std::pow(b1, (double)h->step)));
    p.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, (double)h->step));
  }
  p.stats = stats;
  const int64_t per = OPT_THREADS * OPT_ITEMS;
  hipLaunchKernelGGL(opt_update_kernel, dim3((unsigned)((tv.grad_floats + per - 1) / per)), dim3(OPT_THREADS), 0, s, p);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

// norm partials -> clip coefficient + update (+ the loss of nll_step) -- the two launches above
int opt_launch_update(const char* fn, const OptUpdateView& tv, const float* grads, float* m, float* v, const gbnf_opt_hyper* h, float* stats,
                      double* partials, const double* nll_partial, int n_nll_partial, double nll_scale, double nll_const, void* stream) {
  const int gb = opt_launch_grad_sqsum(grads, tv.grad_floats, partials, stream);
  return opt_launch_update_from(fn, tv, grads, m, v, h, stats, partials, gb, nll_partial, n_nll_partial, nll_scale, nll_const, stream);
}

// ... for a gbnf_trainer: the tabular loss is nll = sum / n + 0.5 d log 2 pi
static int launch_update(const TrainerOptView& tv, const float* grads, float* m, float* v, const gbnf_opt_hyper* h, float* stats,
                         double* partials, const double* nll_partial, int n_nll_partial, int64_t n, hipStream_t s) {
  const OptUpdateView view{tv.regions_dev, tv.n_regions, tv.grad_floats};
  const bool loss = nll_partial != nullptr;
  return opt_launch_update("gbnf_trainer_apply_update", view, grads, m, v, h, stats, partials, nll_partial, n_nll_partial,
                           loss ? 1.0 / (double)n : 0.0, loss ? 0.5 * (double)tv.d * std::log(2.0 * M_PI) : 0.0, (void*)s);
}

// the caller's workspace of one whole step, in 256-byte aligned pieces
struct StepLayout {
  int64_t xg, z, ldj, trace, g_z, g_ldj, bwd, bwd_bytes, partials, total;
};
static int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }
static int step_layout(const gbnf_trainer* t, const TrainerOptView& tv, int64_t n, StepLayout* L) {
  int64_t trace_floats = 0, bwd_bytes = 0;
  int rc = gbnf_trainer_trace_floats(t, n, &trace_floats);
  if (rc == GBNF_OK) rc = gbnf_trainer_workspace_bytes(t, n, &bwd_bytes);
  if (rc) return rc;
  const int64_t nd = align256(n * tv.d * 4), nn = align256(n * 4);
  int64_t off = 0;
  L->xg = off; off += nd;
  L->z = off; off += nd;
  L->ldj = off; off += nn;
  L->trace = off; off += align256(trace_floats * 4);
  L->g_z = off; off += nd;
  L->g_ldj = off; off += nn;
  L->bwd = off; L->bwd_bytes = bwd_bytes; off += align256(bwd_bytes);
  L->partials = off; off += align256(2 * OPT_MAX_PARTIALS * (int64_t)sizeof(double));
  L->total = off;
  return GBNF_OK;
}

}  // namespace gbnf

using namespace gbnf;

extern "C" {

int gbnf_trainer_apply_update(const gbnf_trainer* t, const float* grads, float* exp_avg, float* exp_avg_sq, const gbnf_opt_hyper* h,
                              float* stats_dev, void* stream) {
  if (!t || !grads || !stats_dev) return fail(GBNF_ERR_INVALID, "gbnf_trainer_apply_update: trainer / grads / stats_dev is null");
  if (const int rc = check_hyper("gbnf_trainer_apply_update", h, exp_avg, exp_avg_sq)) return rc;
  TrainerOptView tv;
  if (const int rc = trainer_opt_view(t, &tv)) return rc;
  return launch_update(tv, grads, exp_avg, exp_avg_sq, h, stats_dev, tv.partials_dev, nullptr, 0, 0, (hipStream_t)stream);
}

int gbnf_trainer_step_workspace_bytes(const gbnf_trainer* t, int64_t n, int64_t* bytes) {
  if (!t || !bytes || n < 0) return fail(GBNF_ERR_INVALID, "gbnf_trainer_step_workspace_bytes: bad argument");
  TrainerOptView tv;
  if (const int rc = trainer_opt_view(t, &tv)) return rc;
  StepLayout L;
  if (const int rc = step_layout(t, tv, n, &L)) return rc;
  *bytes = L.total;
  return GBNF_OK;
}

int gbnf_trainer_nll_step(const gbnf_trainer* t, const float* x, int64_t n_x, const int64_t* rows, int64_t n, float* grads, float* exp_avg,
                          float* exp_avg_sq, const gbnf_opt_hyper* h, float* stats_dev, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  const char* fn = "gbnf_trainer_nll_step";
  if (!t || !x || !grads || !stats_dev || !workspace) return fail(GBNF_ERR_INVALID, "%s: trainer / x / grads / stats_dev / workspace is null", fn);
  if (n < 1 || n_x < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld, n_x = %lld (both must be >= 1)", fn, (long long)n, (long long)n_x);
  if (rows == nullptr && n != n_x) return fail(GBNF_ERR_INVALID, "%s: without rows the batch is x itself: n = %lld != n_x = %lld", fn, (long long)n, (long long)n_x);
  if (const int rc = check_hyper(fn, h, exp_avg, exp_avg_sq)) return rc;
  TrainerOptView tv;
  if (const int rc = trainer_opt_view(t, &tv)) return rc;
  StepLayout L;
  if (const int rc = step_layout(t, tv, n, &L)) return rc;
  if (workspace_bytes < L.total)
    return fail(GBNF_ERR_INVALID, "%s: workspace too small: %lld bytes < %lld (gbnf_trainer_step_workspace_bytes)", fn, (long long)workspace_bytes, (long long)L.total);
  if (const int rc = trainer_deterministic_check(t, n, /*traced=*/true, fn)) return rc;
  const bool running_update = tv.batch_stats && n >= 2 && h->bn_momentum >= 0.0f && tv.bn.n > 0;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* z = (float*)(ws + L.z);
  float* ldj = (float*)(ws + L.ldj);
  float* trace = (float*)(ws + L.trace);
  float* g_z = (float*)(ws + L.g_z);
  float* g_ldj = (float*)(ws + L.g_ldj);
  double* nll_partial = (double*)(ws + L.partials);
  double* grad_partial = nll_partial + OPT_MAX_PARTIALS;
  const int64_t nd = n * tv.d;
  if (rows != nullptr) {
    float* xg = (float*)(ws + L.xg);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(opt_partial_blocks(nd)), dim3(OPT_THREADS), 0, s, x, rows, n_x, n, tv.d, xg);
    x = xg;
  }
  int rc = gbnf_trainer_forward(t, x, n, z, ldj, trace, stream);
  if (rc) return rc;
  if (running_update) hipLaunchKernelGGL(bn_running_kernel, dim3((unsigned)tv.bn.n), dim3(64), 0, s, tv.bn, tv.d, h->bn_momentum);
  const unsigned nb = opt_partial_blocks(nd);
  hipLaunchKernelGGL(nll_seed_kernel, dim3(nb), dim3(OPT_THREADS), 0, s, (const float*)z, (const float*)ldj, n, tv.d, 1.0f / (float)n, g_z, g_ldj,
                     nll_partial);
  hipError_t e = hipMemsetAsync(grads, 0, (size_t)tv.grad_floats * 4, s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  rc = gbnf_trainer_backward(t, x, n, trace, g_z, g_ldj, nullptr, grads, ws + L.bwd, L.bwd_bytes, stream);
  if (rc) return rc;
  return launch_update(tv, grads, exp_avg, exp_avg_sq, h, stats_dev, grad_partial, nll_partial, (int)nb, n, s);
}

}  // extern "C"
