// gbnf_score.hip -- the score of the tabular path on the device (gfx950): grad_x log p(x) of one flow component and of the boosted
// mixture  log p(x) = LSE_c(log_w_c + ll_c(x)),  whose gradient is  sum_c r_c grad_x ll_c  with the responsibilities
// r_c = softmax_c(log_w + ll)  (gbnf_mixture_responsibilities, gbnf_image_score.hip: a (C, N) table is a (C, N) table).
//
//   score_seed_kernel       g_z = -r (z - mean) / std^2, g_ldj = r, ll = sum_j log N(z_j; mean_j, std_j) [+ ldj]: one wave per 64 rows
//   score_add_kernel        g_x += t: the `accumulate` form of gbnf_trainer_backward_x (the backward kernels only store)
//
// Both are elementwise: no MFMA, no LDS, no atomics, plain vector stores.  The sweeps of the backward are the trainer's own through
// trainer_backward_x (gbnf_train.hip): gbnf_trainer_backward's launches without the ones that serve the weight gradients alone.
//
// Reference semantics: density_experiment.py:561-573 (the mixture's recursion; its closed form is log_w_c = log(rho_c / sum_j rho_j)),
// utils/distributions.py:44-60 and models/generative_flow.py:22-42 (the base density, 2 pi term included).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../include/gbnf.h"
#include "gbnf_internal.h"
#include "gbnf_opt.h"

namespace gbnf {

constexpr int SS_THREADS = 256;                     // 4 waves
constexpr int SS_ROWS = 64;                         // rows per wave: one lane per row in the per-row pass
constexpr double SS_HALF_LOG_2PI = 0.91893853320467274178;

// A wave owns rows [row0, row0 + 64): 64 d contiguous floats of z and g_z, swept lane-contiguously (16 bytes per lane when VEC: both
// arrays 16-byte aligned; the wave's piece starts 256-byte aligned then): that sweep is the coalesced one.  Then one lane per row
// for g_ldj and the ordered f64 sum of ll: those reads have a lane stride of d floats -- not coalesced; they re-read the lines the
// wave has just streamed, out of the cache.  (The kernel has not been timed on its own.)
// g_z / g_ldj / ll: each may be null (not wanted).  mean null: the standard normal.
template <bool VEC>
__global__ void __launch_bounds__(SS_THREADS) score_seed_kernel(const float* __restrict__ z, const float* __restrict__ mean,
                                                                const float* __restrict__ std_, const float* __restrict__ r,
                                                                const float* __restrict__ ldj, int64_t n, int d, float* __restrict__ g_z,
                                                                float* __restrict__ g_ldj, float* __restrict__ ll) {
  const int lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * (SS_THREADS / 64) + (threadIdx.x >> 6)) * SS_ROWS;
  if (row0 >= n) return;
  const int rows = (int)(n - row0 < SS_ROWS ? n - row0 : SS_ROWS);
  const int cnt = rows * d;
  const float* zc = z + row0 * d;
  if (g_z != nullptr) {
    float* gc = g_z + row0 * d;
    // element (row i, feature j) of the wave's piece
    auto seed = [&](int i, int j, float v) -> float {
      const float ri = r != nullptr ? r[row0 + i] : 1.0f;
      if (mean == nullptr) return -ri * v;
      const float s = std_[j];
      return -ri * (v - mean[j]) / (s * s);
    };
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
          o[q] = seed(i, j, in[q]);
          if (++j == d) { j = 0; ++i; }
        }
        reinterpret_cast<float4*>(gc)[v] = make_float4(o[0], o[1], o[2], o[3]);
      }
      e0 = nv << 2;
    }
    for (int e = e0 + lane; e < cnt; e += 64) {
      const int i = (int)((unsigned)e / (unsigned)d);
      gc[e] = seed(i, e - i * d, zc[e]);
    }
  }
  if (lane >= rows) return;
  const int64_t i = row0 + lane;
  if (g_ldj != nullptr) g_ldj[i] = r != nullptr ? r[i] : 1.0f;
  if (ll == nullptr) return;
  const float* zi = zc + lane * d;
  double acc = 0.0;
  if (mean == nullptr) {
    for (int j = 0; j < d; ++j) {
      const double v = (double)zi[j];
      acc += -SS_HALF_LOG_2PI - 0.5 * v * v;
    }
  } else {
    for (int j = 0; j < d; ++j) {
      const double s = (double)std_[j], v = (double)zi[j] - (double)mean[j];
      acc += -(v * v) / (2.0 * s * s) - log(s) - SS_HALF_LOG_2PI;
    }
  }
  if (ldj != nullptr) acc += (double)ldj[i];
  ll[i] = (float)acc;
}

// g_x[e] += t[e], e < total: grid-stride, 16 bytes per lane when VEC (both arrays 16-byte aligned), the tail by element
template <bool VEC>
__global__ void __launch_bounds__(SS_THREADS) score_add_kernel(const float* __restrict__ t, float* __restrict__ g_x, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * SS_THREADS, tid = (int64_t)blockIdx.x * SS_THREADS + threadIdx.x;
  int64_t e0 = 0;
  if constexpr (VEC) {
    const int64_t nv = total >> 2;
    for (int64_t v = tid; v < nv; v += stride) {
      const float4 a = reinterpret_cast<const float4*>(t)[v];
      float4 o = reinterpret_cast<float4*>(g_x)[v];
      o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
      reinterpret_cast<float4*>(g_x)[v] = o;
    }
    e0 = nv << 2;
  }
  for (int64_t e = e0 + tid; e < total; e += stride) g_x[e] += t[e];
}

namespace {

int64_t ss_align256(int64_t b) { return (b + 255) / 256 * 256; }
bool ss_aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15u) == 0u; }

// ldj: added to ll inside the per-row sum (the mixture's own calls; the ABI call leaves it to its caller)
void launch_seed(const float* z, const float* mean, const float* std_, const float* r, const float* ldj, int64_t n, int d, float* g_z,
                 float* g_ldj, float* ll, hipStream_t s) {
  const int64_t rows_per_block = (int64_t)SS_ROWS * (SS_THREADS / 64);
  const dim3 grid((unsigned)((n + rows_per_block - 1) / rows_per_block)), blk(SS_THREADS);
  if (g_z == nullptr || ss_aligned16(z, g_z))
    hipLaunchKernelGGL(score_seed_kernel<true>, grid, blk, 0, s, z, mean, std_, r, ldj, n, d, g_z, g_ldj, ll);
  else
    hipLaunchKernelGGL(score_seed_kernel<false>, grid, blk, 0, s, z, mean, std_, r, ldj, n, d, g_z, g_ldj, ll);
}

void launch_add(const float* t, float* g_x, int64_t total, hipStream_t s) {
  const int64_t per = (int64_t)SS_THREADS * 4;
  const int64_t blocks = std::min<int64_t>((total + per - 1) / per, 2048);
  const dim3 grid((unsigned)(blocks ? blocks : 1)), blk(SS_THREADS);
  if (ss_aligned16(t, g_x)) hipLaunchKernelGGL(score_add_kernel<true>, grid, blk, 0, s, t, g_x, total);
  else hipLaunchKernelGGL(score_add_kernel<false>, grid, blk, 0, s, t, g_x, total);
}

// The workspace of one gbnf_trainer_backward_x call, in 256-byte aligned pieces: the backward workspace (gbnf_trainer_workspace_bytes
// without the deterministic mode's partials) | the discard region of the per-step kernels' parameter sums | the g_x of a repairing
// trainer's two forms | the (n, d) temporary of `accumulate`, last: a storing call does without it
struct BackwardXLayout {
  int64_t ws_bytes, discard, xpair, tmp, total;
  int d, repairing;
};

int backward_x_layout(const gbnf_trainer* t, int64_t n, bool accumulate, BackwardXLayout* L) {
  TrainerScoreView v{};
  if (const int rc = trainer_score_view(t, &v)) return rc;
  L->ws_bytes = trainer_backward_x_base_bytes(t, n);
  const int64_t nx = ss_align256(n * (int64_t)v.d * 4);
  int64_t off = ss_align256(L->ws_bytes);
  L->discard = off; off += ss_align256(v.grad_floats * 4);
  L->xpair = off; off += v.repairing ? 2 * nx : 0;
  L->tmp = off; off += accumulate ? nx : 0;
  L->total = off;
  L->d = v.d; L->repairing = v.repairing;
  return GBNF_OK;
}

int refuse_batch_stats(const char* fn, const gbnf_trainer* t, int c) {
  TrainerScoreView v{};
  if (const int rc = trainer_score_view(t, &v)) return rc;
  if (!v.batch_stats) return GBNF_OK;
  char who[32] = "the trainer";
  if (c >= 0) std::snprintf(who, sizeof(who), "trainers[%d]", c);
  return fail(GBNF_ERR_UNSUPPORTED, "%s: %s is in batch-statistics mode: its input gradient needs the batch sums that only "
              "gbnf_trainer_backward forms (gbnf_trainer_set_batch_stats(0) for the running statistics)", fn, who);
}

// the caller's workspace of one mixture score: z | ldj | ll (C, n) | r (C, n) | g_z | g_ldj | ONE trace (the widest component's) |
// one gbnf_trainer_backward_x workspace (the largest)
struct MixScoreLayout {
  int64_t z, ldj, ll, r, g_z, g_ldj, trace, bx, bx_bytes, total;
  int d;
};

// entries checked non-null by the caller
int mix_score_layout(const char* fn, gbnf_trainer* const* trainers, int C, int64_t n, MixScoreLayout* L) {
  int64_t tf = 0, bxb = 0;
  int d = 0;
  for (int c = 0; c < C; ++c) {
    BackwardXLayout B;
    if (const int rc = backward_x_layout(trainers[c], n, /*accumulate=*/C > 1, &B)) return rc;
    if (c == 0) d = B.d;
    else if (B.d != d) return fail(GBNF_ERR_INVALID, "%s: trainers[%d] has d = %d, trainers[0] d = %d", fn, c, B.d, d);
    int64_t trace_floats = 0;
    if (const int rc = gbnf_trainer_trace_floats(trainers[c], n, &trace_floats)) return rc;
    tf = std::max(tf, trace_floats);
    bxb = std::max(bxb, B.total);
  }
  const int64_t nx = ss_align256(n * (int64_t)d * 4), nn = ss_align256(n * 4), cn = ss_align256((int64_t)C * n * 4);
  int64_t off = 0;
  L->z = off; off += nx;
  L->ldj = off; off += nn;
  L->ll = off; off += cn;
  L->r = off; off += cn;
  L->g_z = off; off += nx;
  L->g_ldj = off; off += nn;
  L->trace = off; off += ss_align256(tf * 4);
  L->bx = off; L->bx_bytes = bxb; off += ss_align256(bxb);
  L->total = off;
  L->d = d;
  return GBNF_OK;
}

int check_mix_trainers(const char* fn, gbnf_trainer* const* trainers, int C) {
  for (int c = 0; c < C; ++c)
    if (!trainers[c]) return fail(GBNF_ERR_INVALID, "%s: trainers[%d] is null", fn, c);
  for (int c = 0; c < C; ++c)
    if (const int rc = refuse_batch_stats(fn, trainers[c], c)) return rc;
  return GBNF_OK;
}

}  // namespace

// ll[i] = log N(z_i; 0, I) + ldj[i]: the seed launch with nothing but ll wanted (the mixture step's table, gbnf_mixstep.hip)
void score_launch_ll(const float* z, const float* ldj, int64_t n, int d, float* ll, hipStream_t s) {
  launch_seed(z, nullptr, nullptr, nullptr, ldj, n, d, nullptr, nullptr, ll, s);
}

}  // namespace gbnf

using namespace gbnf;

extern "C" {

int gbnf_trainer_backward_x_workspace_bytes(const gbnf_trainer* t, int64_t n, int64_t* bytes) {
  if (!t || !bytes || n < 0) return fail(GBNF_ERR_INVALID, "gbnf_trainer_backward_x_workspace_bytes: bad argument");
  BackwardXLayout L;
  if (const int rc = backward_x_layout(t, n, /*accumulate=*/true, &L)) return rc;      // (the size that serves either form)
  *bytes = L.total;
  return GBNF_OK;
}

int gbnf_trainer_backward_x(const gbnf_trainer* t, const float* x, int64_t n, const float* trace, const float* g_z, const float* g_ldj,
                            float* g_x, int32_t accumulate, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "gbnf_trainer_backward_x";
  if (!t) return fail(GBNF_ERR_INVALID, "%s: trainer is null", fn);
  if (n < 0) return fail(GBNF_ERR_INVALID, "%s: n < 0", fn);
  if (!x || !g_x || !workspace) return fail(GBNF_ERR_INVALID, "%s: x / g_x / workspace is null", fn);
  if (const int rc = refuse_batch_stats(fn, t, -1)) return rc;
  if (n == 0) return GBNF_OK;
  BackwardXLayout L;
  if (const int rc = backward_x_layout(t, n, accumulate != 0, &L)) return rc;
  if (workspace_bytes < L.total)
    return fail(GBNF_ERR_INVALID, "%s: workspace too small: %lld bytes < %lld (gbnf_trainer_backward_x_workspace_bytes%s)", fn,
                (long long)workspace_bytes, (long long)L.total, accumulate ? "" : "; a storing call does without its last n d floats");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* tmp = (float*)(ws + L.tmp);
  float* out = accumulate ? tmp : g_x;
  if (const int rc = trainer_backward_x(t, x, n, trace, g_z, g_ldj, out, ws, L.ws_bytes, (float*)(ws + L.discard),
                                        L.repairing ? (float*)(ws + L.xpair) : nullptr, s))
    return rc;
  if (accumulate) {
    launch_add(tmp, g_x, n * (int64_t)L.d, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  }
  return GBNF_OK;
}

int gbnf_score_seed(const float* z, const float* base_mean_or_null, const float* base_std_or_null, const float* r_or_null, int64_t n,
                    int32_t d, float* g_z, float* g_ldj, float* ll_or_null, void* stream) {
  const char* fn = "gbnf_score_seed";
  if (!z || !g_z || !g_ldj) return fail(GBNF_ERR_INVALID, "%s: z / g_z / g_ldj is null", fn);
  if (n < 0 || d < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld, d = %d", fn, (long long)n, (int)d);
  if ((base_mean_or_null == nullptr) != (base_std_or_null == nullptr))
    return fail(GBNF_ERR_INVALID, "%s: the base density needs both mean and std (or neither: the standard normal)", fn);
  if (n == 0) return GBNF_OK;
  launch_seed(z, base_mean_or_null, base_std_or_null, r_or_null, nullptr, n, d, g_z, g_ldj, ll_or_null, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

int gbnf_mixture_score_workspace_bytes(gbnf_trainer* const* trainers, int32_t n_components, int64_t n, int64_t* bytes) {
  const char* fn = "gbnf_mixture_score_workspace_bytes";
  if (!trainers || !bytes) return fail(GBNF_ERR_INVALID, "%s: trainers / bytes is null", fn);
  if (n_components < 1 || n < 0) return fail(GBNF_ERR_INVALID, "%s: n_components = %d, n = %lld", fn, (int)n_components, (long long)n);
  for (int c = 0; c < n_components; ++c)
    if (!trainers[c]) return fail(GBNF_ERR_INVALID, "%s: trainers[%d] is null", fn, c);
  MixScoreLayout L;
  if (const int rc = mix_score_layout(fn, trainers, n_components, n, &L)) return rc;
  *bytes = L.total;
  return GBNF_OK;
}

int gbnf_mixture_score(gbnf_trainer* const* trainers, int32_t n_components, const float* log_w, const float* base_mean_or_null,
                       const float* base_std_or_null, const float* ll_or_null, const float* x, int64_t n, float* g_x, float* G,
                       float* r_or_null, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "gbnf_mixture_score";
  if (!trainers || !log_w || !x || !g_x || !G || !workspace)
    return fail(GBNF_ERR_INVALID, "%s: trainers / log_w / x / g_x / G / workspace is null", fn);
  if (n_components < 1) return fail(GBNF_ERR_INVALID, "%s: n_components = %d (must be >= 1)", fn, (int)n_components);
  if (n < 0) return fail(GBNF_ERR_INVALID, "%s: n < 0", fn);
  if ((base_mean_or_null == nullptr) != (base_std_or_null == nullptr))
    return fail(GBNF_ERR_INVALID, "%s: the base density needs both mean and std (or neither: the standard normal)", fn);
  const int C = (int)n_components;
  if (const int rc = check_mix_trainers(fn, trainers, C)) return rc;
  MixScoreLayout L;
  if (const int rc = mix_score_layout(fn, trainers, C, n, &L)) return rc;        // (also: one d)
  if (n == 0) return GBNF_OK;
  if (workspace_bytes < L.total)
    return fail(GBNF_ERR_INVALID, "%s: workspace too small: %lld bytes < %lld (gbnf_mixture_score_workspace_bytes)", fn,
                (long long)workspace_bytes, (long long)L.total);
  for (int c = 0; c < C; ++c)      // (the deterministic-mode refusals of every component's backward, before the first launch)
    if (const int rc = trainer_deterministic_check(trainers[c], n, /*traced=*/true, fn)) return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* z = (float*)(ws + L.z);
  float* ldj = (float*)(ws + L.ldj);
  float* ll = (float*)(ws + L.ll);
  float* r = (float*)(ws + L.r);
  float* g_z = (float*)(ws + L.g_z);
  float* g_ldj = (float*)(ws + L.g_ldj);
  float* trace = (float*)(ws + L.trace);
  const int d = L.d;
  const float* mean = base_mean_or_null;
  const float* sd = base_std_or_null;
  // A lone component without a table: its ll comes out of step 3's own forward (r = 1 whatever ll is)
  const bool lone = C == 1 && ll_or_null == nullptr;
  // 1. the table ll (C, n): the caller's, or one forward per component.  That forward runs on the ONE trace buffer too (step 3
  //    overwrites it): with a trace every math mode stays on its register-chained sweep and a range-safe trainer allocates nothing.
  const float* table = ll_or_null;
  if (table == nullptr && !lone) {
    for (int c = 0; c < C; ++c) {
      if (const int rc = gbnf_trainer_forward(trainers[c], x, n, z, ldj, trace, stream)) return rc;
      launch_seed(z, mean, sd, nullptr, ldj, n, d, nullptr, nullptr, ll + (int64_t)c * n, s);
    }
    table = ll;
  }
  // 2. the responsibilities and log p
  if (!lone) {
    if (const int rc = gbnf_mixture_responsibilities(table, log_w, C, n, r, G, stream)) return rc;
    if (r_or_null != nullptr && hipMemcpyAsync(r_or_null, r, (size_t)C * n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return fail(GBNF_ERR_HIP, "%s: the copy of r failed", fn);
  }
  // 3. per component, in order: the traced forward, the seed with row c of r, the data-gradient-only backward (stored by component
  //    0, added by the others: the backward is linear in its seeds)
  for (int c = 0; c < C; ++c) {
    if (const int rc = gbnf_trainer_forward(trainers[c], x, n, z, ldj, trace, stream)) return rc;
    launch_seed(z, mean, sd, lone ? nullptr : r + (int64_t)c * n, lone ? ldj : nullptr, n, d, g_z, g_ldj, lone ? ll : nullptr, s);
    if (lone) {
      if (const int rc = gbnf_mixture_responsibilities(ll, log_w, 1, n, r, G, stream)) return rc;
      if (r_or_null != nullptr && hipMemcpyAsync(r_or_null, r, (size_t)n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(GBNF_ERR_HIP, "%s: the copy of r failed", fn);
    }
    if (const int rc = gbnf_trainer_backward_x(trainers[c], x, n, trace, g_z, g_ldj, g_x, c > 0 ? 1 : 0, ws + L.bx, L.bx_bytes, stream))
      return rc;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

}  // extern "C"
