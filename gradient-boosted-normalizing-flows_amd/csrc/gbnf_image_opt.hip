// gbnf_image_opt.hip -- one iteration of the reference's image training loop for ONE Glow component in one call on the device (gfx950):
// what image_experiment.py:378-419 runs in eager PyTorch around the component's forward and backward.
//
//   img_mix_logdet_kernel<0>   before the forward, one workgroup per bound 1x1 step: an LU step's matrix W = P (lower.m + I)
//                              (upper.m^T + diag(sign_s e^log_s)) is composed from the live factors into the tensor the trainer binds as
//                              perm_weight (models/layers.py:757-768) and its log-det is hw sum(log_s); a plain weight is inverted by
//                              Gauss-Jordan with partial pivoting: hw log|det W| and W^-T (kept for the gradient)
//   img_nll_seed_kernel        nll_i = -(log_normal_diag(z, mu, lv) + ldj_i + the log-dets) (image_experiment.py:227-229,
//                              utils/distributions.py:13-21), its autograd seed g_z, g_ldj scaled by loss_scale / n, per-workgroup
//                              partial sums of the loss and of the top prior's per-channel gradients
//   img_mix_logdet_kernel<1>   behind the backward: g_W += -k hw W^-T for a plain weight; for an LU step the chain from the composed
//                              matrix's gradient to lower / upper / log_s (the composed region is zeroed: no tensor behind it); one more
//                              workgroup turns the prior partials into the gradients of learn_top_fn's bias and logs
//   grad_sqsum_kernel, opt_update_kernel (gbnf_opt.hip)   clip_grad_norm_ and optim.AdamW / optim.SGD on the live tensors
//
// Everything here is small and latency-bound: C <= 64, matrices in LDS in f64, no MFMA, no float atomics.  Reductions follow
// gbnf_opt.hip: per-workgroup f64 partial sums, re-added in a fixed order by the consumer behind it in stream order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/gbnf.h"
#include "gbnf_internal.h"
#include "gbnf_opt.h"
#include "gbnf_image_train.h"
#include "gbnf_image_ycond.h"

namespace gbnf {

constexpr int IOPT_THREADS = 256;
constexpr int MIX_MAX_C = 64;                                 // channels of a level (gbnf_image_trainer_create refuses more)
// dynamic LDS of img_mix_logdet_kernel (doubles): three C x C matrices or one C x 2C augmented one | the column factors | the pivot row.
// All of it is dynamic: the opt-in (DynamicLdsOptIn) raises the dynamic limit to the whole 160 KB, which leaves no room for static LDS.
constexpr int MIX_LDS_MATS = 3 * MIX_MAX_C * MIX_MAX_C;
constexpr size_t MIX_LDS_BYTES = (MIX_LDS_MATS + MIX_MAX_C + 2) * sizeof(double);
static_assert(OPT_MAX_PARTIALS == IOPT_THREADS, "a workgroup re-adds the partial sums one per thread");

// One 1x1 step whose matrix is a bound tensor (perm_weight), plain or LU
struct MixStep {
  float* w;                 // the (C, C) matrix the forward reads: the plain weight, or the persistent composed one of an LU step
  int C;
  float hw;                 // pixels of the level's map
  int64_t g_w;              // its region of the flat gradient buffer (LU: reserved, zero behind the step)
  const float* p;           // LU: (C, C) permutation, null = plain weight
  const float* sign_s;      //     (C,)
  const float* lower;       //     (C, C), (C, C), (C,): the live factors
  const float* upper;
  const float* log_s;
  int64_t g_lower, g_upper, g_log_s;
  double* inv;              // plain: W^-T as img_mix_logdet_kernel<0> left it (C * C, trainer-owned)
};

struct TopPrior {           // learn_top_fn (Conv2dZeros 2Cz -> 2Cz of a zero input: bias * exp(3 logs)); bias null = zero-mean unit prior
  const float* bias;
  const float* logs;
  int64_t g_bias, g_logs;
  int Cz;
};

// the workgroup's 256 values added up in a fixed tree order; every thread gets the sum
__device__ __forceinline__ double iopt_block_sum(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = IOPT_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

// L' = lower . m + I and U' = upper . m^T + diag(sign_s e^log_s) of an LU step, as doubles (C * C each)
__device__ __forceinline__ void mix_load_lu(const MixStep& st, double* Lp, double* Up) {
  const int C = st.C;
  for (int idx = threadIdx.x; idx < C * C; idx += IOPT_THREADS) {
    const int i = idx / C, j = idx - i * C;
    if (Lp != nullptr) Lp[idx] = i > j ? (double)st.lower[idx] : (i == j ? 1.0 : 0.0);
    if (Up != nullptr) Up[idx] = i < j ? (double)st.upper[idx] : (i == j ? (double)st.sign_s[i] * exp((double)st.log_s[i]) : 0.0);
  }
}

struct MixLaunch {
  const MixStep* steps;
  int n_mix;
  double* ld;               // [n_mix] hw log|det W| per step
  float k;                  // loss_scale
  float* grads;             // PHASE 1
  TopPrior top;             // PHASE 1: workgroup n_mix (when top.bias != null)
  const double* mu_part;    //   per-workgroup sums of img_nll_seed_kernel: [Cz][bpc] each
  const double* lv_part;
  int bpc;
};

template <int PHASE>
__global__ void __launch_bounds__(IOPT_THREADS) img_mix_logdet_kernel(const MixLaunch q) {
  extern __shared__ __attribute__((aligned(16))) double mlds[];
  double* fac = mlds + MIX_LDS_MATS;
  int& piv_s = *reinterpret_cast<int*>(mlds + MIX_LDS_MATS + MIX_MAX_C);
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= q.n_mix) {
    // ---- the top prior (PHASE 1 only): h = bias e^{3 logs}; g_bias = g_h e^{3 logs}, g_logs = 3 g_h h ----
    if (PHASE == 0 || q.top.bias == nullptr) return;
    const int Cz = q.top.Cz;
    for (int j = tid; j < 2 * Cz; j += IOPT_THREADS) {
      const int c = j < Cz ? j : j - Cz;
      const double* part = (j < Cz ? q.mu_part : q.lv_part) + (int64_t)c * q.bpc;
      double g_h = 0.0;
      for (int b = 0; b < q.bpc; ++b) g_h += part[b];
      if (j < Cz) g_h = -g_h;                               // g_mu = -sum g_z
      const double e3 = exp(3.0 * (double)q.top.logs[j]), h = (double)q.top.bias[j] * e3;
      q.grads[q.top.g_bias + j] += (float)(g_h * e3);
      q.grads[q.top.g_logs + j] += (float)(3.0 * g_h * h);
    }
    return;
  }
  const MixStep st = q.steps[blockIdx.x];
  const int C = st.C, CC = C * C;
  if (st.p != nullptr) {
    double* b0 = mlds;
    double* b1 = mlds + CC;
    double* b2 = mlds + 2 * CC;
    if (PHASE == 0) {
      // ---- compose W = P (L' U') into the bound tensor; log|det W| = sum(log_s) ----
      mix_load_lu(st, b0, b1);
      __syncthreads();
      for (int idx = tid; idx < CC; idx += IOPT_THREADS) {
        const int i = idx / C, j = idx - i * C;
        double acc = 0.0;
        for (int r = 0; r < C; ++r) acc = fma(b0[i * C + r], b1[r * C + j], acc);
        b2[idx] = acc;
      }
      __syncthreads();
      for (int idx = tid; idx < CC; idx += IOPT_THREADS) {
        const int i = idx / C, j = idx - i * C;
        double acc = 0.0;
        for (int r = 0; r < C; ++r) acc = fma((double)st.p[i * C + r], b2[r * C + j], acc);
        st.w[idx] = (float)acc;
      }
      if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < C; ++i) s += (double)st.log_s[i];
        q.ld[blockIdx.x] = (double)st.hw * s;
      }
    } else {
      // ---- G (the composed matrix's data-path gradient) -> lower / upper / log_s; A = P^T G ----
      float* G = q.grads + st.g_w;
      for (int idx = tid; idx < CC; idx += IOPT_THREADS) {
        b1[idx] = (double)G[idx];
        b2[idx] = (double)st.p[idx];
        G[idx] = 0.0f;                                        // a reserved region from here on: nothing for the norm or the update
      }
      __syncthreads();
      for (int idx = tid; idx < CC; idx += IOPT_THREADS) {
        const int i = idx / C, j = idx - i * C;
        double acc = 0.0;
        for (int r = 0; r < C; ++r) acc = fma(b2[r * C + i], b1[r * C + j], acc);
        b0[idx] = acc;
      }
      __syncthreads();
      mix_load_lu(st, b2, b1);
      __syncthreads();
      const double kh = (double)q.k * (double)st.hw;
      for (int idx = tid; idx < CC; idx += IOPT_THREADS) {
        const int i = idx / C, j = idx - i * C;
        if (i > j) {                                          // g_lower = (A U'^T) . m
          double acc = 0.0;
          for (int r = 0; r < C; ++r) acc = fma(b0[i * C + r], b1[j * C + r], acc);
          q.grads[st.g_lower + idx] += (float)acc;
        } else {                                              // g_upper = (L'^T A) . m^T; its diagonal is log_s's
          double acc = 0.0;
          for (int r = 0; r < C; ++r) acc = fma(b2[r * C + i], b0[r * C + j], acc);
          if (i < j) q.grads[st.g_upper + idx] += (float)acc;
          else q.grads[st.g_log_s + i] += (float)(acc * b1[idx] - kh);
        }
      }
    }
    return;
  }
  // ---- plain weight ----
  if (PHASE == 1) {
    const double coef = -(double)q.k * (double)st.hw;
    for (int idx = tid; idx < CC; idx += IOPT_THREADS) q.grads[st.g_w + idx] += (float)(coef * st.inv[idx]);
    return;
  }
  // Gauss-Jordan with partial pivoting on [W | I] (C x 2C): row operations only, so the right half ends as W^-1
  double* A = mlds;
  const int S = 2 * C;
  for (int idx = tid; idx < C * S; idx += IOPT_THREADS) {
    const int i = idx / S, j = idx - i * S;
    A[idx] = j < C ? (double)st.w[i * C + j] : (j - C == i ? 1.0 : 0.0);
  }
  __syncthreads();
  double logdet = 0.0;                                        // (every thread keeps the same value)
  for (int kcol = 0; kcol < C; ++kcol) {
    if (tid < 64) {                                           // wave 0: the largest |entry| of the column at or below the diagonal
      double v = (tid >= kcol && tid < C) ? fabs(A[tid * S + kcol]) : -1.0;
      int at = tid;
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        const double ov = __shfl_xor(v, m);
        const int oi = __shfl_xor(at, m);
        if (ov > v || (ov == v && oi < at)) { v = ov; at = oi; }
      }
      if (tid == 0) piv_s = (at >= kcol && at < C) ? at : kcol;     // (a column of NaN: no lane wins, stay on the diagonal)
    }
    __syncthreads();
    const int piv = piv_s;
    if (piv != kcol) {
      for (int j = tid; j < S; j += IOPT_THREADS) {
        const double a = A[kcol * S + j];
        A[kcol * S + j] = A[piv * S + j];
        A[piv * S + j] = a;
      }
    }
    __syncthreads();
    const double pivot = A[kcol * S + kcol];
    logdet += log(fabs(pivot));                               // a zero pivot: -inf, as torch's slogdet
    if (tid < C) fac[tid] = tid == kcol ? 0.0 : A[tid * S + kcol];
    __syncthreads();
    for (int j = tid; j < S; j += IOPT_THREADS) A[kcol * S + j] = A[kcol * S + j] / pivot;
    __syncthreads();
    for (int idx = tid; idx < C * S; idx += IOPT_THREADS) {
      const int r = idx / S, j = idx - r * S;
      if (r != kcol) A[idx] = fma(-fac[r], A[kcol * S + j], A[idx]);
    }
    __syncthreads();
  }
  for (int idx = tid; idx < CC; idx += IOPT_THREADS) {
    const int i = idx / C, j = idx - i * C;
    st.inv[idx] = A[j * S + C + i];                           // W^-T[i][j] = W^-1[j][i]
  }
  if (tid == 0) q.ld[blockIdx.x] = (double)st.hw * logdet;
}

struct SeedLaunch {
  const float* z;           // (n, Cz, HW)
  const float* ldj;         // (n,) without the 1x1 matrices' log-dets
  const double* ld;         // [n_mix]
  int n_mix;
  const float* top_bias;    // (2 Cz,) or null
  const float* top_logs;
  int64_t n;
  int Cz, HW, bpc;
  float kn;                 // loss_scale / n
  float* g_z;
  float* g_ldj;
  double* nll_part;         // [Cz * bpc]
  double* mu_part;
  double* lv_part;
};

// grid (bpc, Cz): workgroup (b, c) takes a strided share of channel c's n * HW entries and of the n rows
__global__ void __launch_bounds__(IOPT_THREADS) img_nll_seed_kernel(const SeedLaunch q) {
  __shared__ double lds[IOPT_THREADS];
  __shared__ double ld_total;
  const int tid = threadIdx.x, c = blockIdx.y;
  const int lb = c * q.bpc + blockIdx.x, nbk = q.bpc * q.Cz;
  if (tid == 0) {
    double s = 0.0;
    for (int m = 0; m < q.n_mix; ++m) s += q.ld[m];
    ld_total = s;
  }
  __syncthreads();
  float mu = 0.0f, lv = 0.0f;
  if (q.top_bias != nullptr) {                                // Conv2dZeros of a zero input (models/layers.py:609-630), f32 as torch computes it
    mu = q.top_bias[c] * expf(3.0f * q.top_logs[c]);
    lv = q.top_bias[q.Cz + c] * expf(3.0f * q.top_logs[q.Cz + c]);
  }
  const float e = expf(-lv);
  double a_nll = 0.0, a_gz = 0.0, a_lv = 0.0;
  const int64_t total = q.n * q.HW, stride = (int64_t)q.bpc * IOPT_THREADS;
  for (int64_t t = (int64_t)blockIdx.x * IOPT_THREADS + tid; t < total; t += stride) {
    const int64_t i = t / q.HW;
    const int64_t at = (i * q.Cz + c) * q.HW + (t - i * q.HW);
    const float d = q.z[at] - mu;
    const float dde = d * d * e, gz = q.kn * d * e;
    q.g_z[at] = gz;
    a_nll += 0.5 * ((double)lv + (double)dde);
    a_gz += (double)gz;
    a_lv += (double)q.kn * 0.5 * (1.0 - (double)dde);
  }
  for (int64_t i = (int64_t)lb * IOPT_THREADS + tid; i < q.n; i += (int64_t)nbk * IOPT_THREADS) {
    a_nll -= (double)q.ldj[i] + ld_total;
    q.g_ldj[i] = -q.kn;
  }
  const double s_nll = iopt_block_sum(a_nll, lds), s_gz = iopt_block_sum(a_gz, lds), s_lv = iopt_block_sum(a_lv, lds);
  if (tid == 0) {
    q.nll_part[lb] = s_nll;
    q.mu_part[lb] = s_gz;
    q.lv_part[lb] = s_lv;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct ImageStepState {
  struct Lu {
    int level, step, entry;
    const float* p; const float* sign_s; float* lower; float* upper; float* log_s;
  };
  std::vector<Lu> lu;                          // in bind order: the order of their regions behind the trainer's own
  float* top_weight = nullptr;                 // may stay null with bias / logs bound (no region then)
  float* top_bias = nullptr;
  float* top_logs = nullptr;
  int64_t g_top_w = -1, g_top_bias = -1, g_top_logs = -1;
  // gbnf_image_trainer_bind_ycond: project_ycond / project_class (live tensors) and their regions behind the top prior's
  int y_classes = 0;
  float* yc[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // cond weight, bias, logs, class weight, bias, logs
  int64_t g_yc[6] = {-1, -1, -1, -1, -1, -1};
  int64_t step_grad_floats = 0;
  int n_mix = 0, n_regions = 0;
  bool ready = false;                          // the device tables below match the bindings (false after a failed rebuild: every step call refuses)
  MixStep* mix_dev = nullptr;
  OptRegion* regions_dev = nullptr;
  double* sums_dev = nullptr;                  // [n_mix] log-dets | OPT_MAX_PARTIALS (gbnf_image_trainer_apply_update) | W^-T per plain step
};

namespace {

int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

void free_device(ImageStepState* s) {
  if (s->mix_dev) (void)hipFree(s->mix_dev);
  if (s->regions_dev) (void)hipFree(s->regions_dev);
  if (s->sums_dev) (void)hipFree(s->sums_dev);
  s->mix_dev = nullptr; s->regions_dev = nullptr; s->sums_dev = nullptr;
}

hipError_t mix_allow_lds() {
  static DynamicLdsOptIn optin;
  return optin({(const void*)img_mix_logdet_kernel<0>, (const void*)img_mix_logdet_kernel<1>});
}

// the step layout, the 1x1 table and the update kernel's region table from the trainer's table and the bindings
int rebuild(gbnf_image_trainer* t) {
  ImageStepState* s = t->step;
  s->ready = false;
  free_device(s);
  int64_t off = t->grad_floats;
  std::vector<int64_t> lu_off;
  for (const auto& b : s->lu) {
    lu_off.push_back(off);
    const int64_t C = t->table[b.entry].cin;
    off += 2 * C * C + C;
  }
  s->g_top_w = s->g_top_bias = s->g_top_logs = -1;
  const int64_t top_c = 2 * (int64_t)t->zC;
  if (s->top_bias != nullptr) {
    if (s->top_weight != nullptr) { s->g_top_w = off; off += top_c * top_c * 9; }
    s->g_top_bias = off; off += top_c;
    s->g_top_logs = off; off += top_c;
  }
  const int64_t yc_len[6] = {top_c * s->y_classes, top_c, top_c, (int64_t)s->y_classes * t->zC, s->y_classes, s->y_classes};
  for (int k = 0; k < 6; ++k) {
    s->g_yc[k] = -1;
    if (s->y_classes > 0) { s->g_yc[k] = off; off += yc_len[k]; }
  }
  s->step_grad_floats = off;

  std::vector<MixStep> mix;
  std::vector<int64_t> inv_slot;                              // per entry of mix: which W^-T buffer (plain weights), -1 = LU
  std::vector<OptRegion> regions;
  auto region = [&](const float* p, int64_t o, int64_t len) {
    if (p != nullptr && o >= 0) regions.push_back(OptRegion{const_cast<float*>(p), o, len});
  };
  int n_plain = 0;
  for (size_t k = 0; k < t->table.size(); ++k) {
    const TConv& e = t->table[k];
    if (!e.mix) {
      region(e.w, e.g_w, (int64_t)e.cout * e.cin * e.ks * e.ks);
      region(e.bias, e.g_bias, e.cout);
      region(e.an_bias, e.g_an_bias, e.cout);
      region(e.an_logs, e.g_an_logs, e.cout);
      region(e.logs, e.g_logs, e.cout);
      continue;
    }
    region(e.an_bias, e.g_an_bias, e.cin);
    region(e.an_logs, e.g_an_logs, e.cin);
    if (e.g_w < 0) continue;                                  // a permutation: no tensor, no log-det
    MixStep m{};
    m.w = const_cast<float*>(e.w); m.C = e.cin; m.hw = e.hw; m.g_w = e.g_w;
    for (size_t b = 0; b < s->lu.size(); ++b) {
      if (s->lu[b].entry != (int)k) continue;
      const auto& lu = s->lu[b];
      const int64_t CC = (int64_t)e.cin * e.cin;
      m.p = lu.p; m.sign_s = lu.sign_s; m.lower = lu.lower; m.upper = lu.upper; m.log_s = lu.log_s;
      m.g_lower = lu_off[b]; m.g_upper = lu_off[b] + CC; m.g_log_s = lu_off[b] + 2 * CC;
    }
    if (m.p == nullptr) {
      region(e.w, e.g_w, (int64_t)e.cin * e.cin);
    }
    inv_slot.push_back(m.p == nullptr ? n_plain++ : -1);
    mix.push_back(m);
  }
  for (size_t b = 0; b < s->lu.size(); ++b) {
    const auto& lu = s->lu[b];
    const int64_t C = t->table[lu.entry].cin;
    region(lu.lower, lu_off[b], C * C);
    region(lu.upper, lu_off[b] + C * C, C * C);
    region(lu.log_s, lu_off[b] + 2 * C * C, C);
  }
  region(s->top_weight, s->g_top_w, top_c * top_c * 9);
  region(s->top_bias, s->g_top_bias, top_c);
  region(s->top_logs, s->g_top_logs, top_c);
  for (int k = 0; k < 6; ++k) region(s->yc[k], s->g_yc[k], yc_len[k]);
  s->n_mix = (int)mix.size();
  s->n_regions = (int)regions.size();

  const int64_t ld_slots = align256((int64_t)s->n_mix * 8) / 8;
  const int64_t sums = ld_slots + OPT_MAX_PARTIALS + (int64_t)n_plain * MIX_MAX_C * MIX_MAX_C;
  hipError_t e = hipMalloc((void**)&s->sums_dev, (size_t)sums * sizeof(double));
  if (e == hipSuccess) e = hipMemset(s->sums_dev, 0, (size_t)sums * sizeof(double));
  for (size_t k = 0; k < mix.size() && e == hipSuccess; ++k)
    if (inv_slot[k] >= 0) mix[k].inv = s->sums_dev + ld_slots + OPT_MAX_PARTIALS + inv_slot[k] * MIX_MAX_C * MIX_MAX_C;
  if (e == hipSuccess && !mix.empty()) {
    e = hipMalloc((void**)&s->mix_dev, mix.size() * sizeof(MixStep));
    if (e == hipSuccess) e = hipMemcpy(s->mix_dev, mix.data(), mix.size() * sizeof(MixStep), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMalloc((void**)&s->regions_dev, regions.size() * sizeof(OptRegion));
  if (e == hipSuccess) e = hipMemcpy(s->regions_dev, regions.data(), regions.size() * sizeof(OptRegion), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = mix_allow_lds();
  if (e != hipSuccess) {
    free_device(s);
    return fail(GBNF_ERR_HIP, "gbnf_image_trainer (training-step tables): %s", hipGetErrorString(e));
  }
  s->ready = true;
  return GBNF_OK;
}

double* ld_sums(const ImageStepState* s) { return s->sums_dev; }
double* update_partials(const ImageStepState* s) { return s->sums_dev + align256((int64_t)s->n_mix * 8) / 8; }

// the caller's workspace of one whole step, in 256-byte aligned pieces
struct ImageStepLayout {
  int64_t z, ldj, trace, g_z, g_ldj, ws, ws_bytes, partials, yterms, total;
};
int image_step_layout(const gbnf_image_trainer* t, int64_t n, ImageStepLayout* L) {
  int64_t trace_floats = 0, ws_bytes = 0;
  int rc = gbnf_image_trainer_trace_floats(t, n, &trace_floats);
  if (rc == GBNF_OK) rc = gbnf_image_trainer_workspace_bytes(t, n, &ws_bytes);
  if (rc) return rc;
  const int64_t nz = align256(n * t->zC * t->zH * t->zW * 4), nn = align256(n * 4);
  int64_t off = 0;
  L->z = off; off += nz;
  L->ldj = off; off += nn;
  L->trace = off; off += align256(trace_floats * 4);
  L->g_z = off; off += nz;
  L->g_ldj = off; off += nn;
  L->ws = off; L->ws_bytes = ws_bytes; off += align256(ws_bytes);
  L->partials = off; off += align256(4 * OPT_MAX_PARTIALS * (int64_t)sizeof(double));    // loss | prior mean | prior log-var | norm
  L->yterms = off;                                            // the per-image terms of a conditioned trainer's step (gbnf_image_ycond.hip)
  if (t->step->y_classes > 0) off += align256(ycond_terms_bytes(n, t->step->y_classes, t->zC));
  L->total = off;
  return GBNF_OK;
}

OptUpdateView update_view(const gbnf_image_trainer* t) {
  return OptUpdateView{t->step->regions_dev, t->step->n_regions, t->step->step_grad_floats};
}

}  // namespace

int image_step_state_create(gbnf_image_trainer* t) {
  t->step = new ImageStepState();
  return rebuild(t);
}

void image_step_state_destroy(ImageStepState* s) {
  if (!s) return;
  free_device(s);
  delete s;
}

int image_step_compose(const gbnf_image_trainer* t, void* stream) {
  const ImageStepState* st = t->step;
  if (!st) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_actnorm_init: trainer is null");
  if (st->lu.empty()) return GBNF_OK;
  if (!st->ready) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_actnorm_init: the last bind call failed: bind again first");
  if (mix_allow_lds() != hipSuccess) return fail(GBNF_ERR_HIP, "gbnf_image_trainer_actnorm_init: the 1x1 kernels' LDS opt-in failed");
  MixLaunch mq{};
  mq.steps = st->mix_dev; mq.n_mix = st->n_mix; mq.ld = ld_sums(st); mq.k = 1.0f;
  hipLaunchKernelGGL((img_mix_logdet_kernel<0>), dim3((unsigned)st->n_mix), dim3(IOPT_THREADS), MIX_LDS_BYTES, (hipStream_t)stream, mq);
  return GBNF_OK;
}

int image_score_top(const char* fn, const gbnf_image_trainer* t, ImageScoreTop* out) {
  const ImageStepState* st = t->step;
  if (!st || !st->ready) return fail(GBNF_ERR_INVALID, "%s: the last bind call of a trainer failed: bind again first", fn);
  out->ld = ld_sums(st); out->n_mix = st->n_mix; out->top_bias = st->top_bias; out->top_logs = st->top_logs;
  out->y_classes = st->y_classes;
  for (int k = 0; k < 6; ++k) out->yc[k] = st->yc[k];
  return GBNF_OK;
}

int image_score_logdets(const char* fn, const gbnf_image_trainer* t, void* stream) {
  const ImageStepState* st = t->step;
  if (st->n_mix == 0) return GBNF_OK;
  if (mix_allow_lds() != hipSuccess) return fail(GBNF_ERR_HIP, "%s: the 1x1 kernels' LDS opt-in failed", fn);
  MixLaunch mq{};
  mq.steps = st->mix_dev; mq.n_mix = st->n_mix; mq.ld = ld_sums(st); mq.k = 1.0f;
  hipLaunchKernelGGL((img_mix_logdet_kernel<0>), dim3((unsigned)st->n_mix), dim3(IOPT_THREADS), MIX_LDS_BYTES, (hipStream_t)stream, mq);
  return GBNF_OK;
}

}  // namespace gbnf

using namespace gbnf;

extern "C" {

int gbnf_image_trainer_bind_lu(gbnf_image_trainer* t, int32_t level, int32_t step, const float* p, const float* sign_s, float* lower,
                               float* upper, float* log_s) {
  const char* fn = "gbnf_image_trainer_bind_lu";
  if (!t || !t->step) return fail(GBNF_ERR_INVALID, "%s: trainer is null", fn);
  if (!p || !sign_s || !lower || !upper || !log_s) return fail(GBNF_ERR_INVALID, "%s: p / sign_s / lower / upper / log_s is null", fn);
  if (level < 0 || level >= t->L || step < 0 || step >= t->levels[level].K)
    return fail(GBNF_ERR_INVALID, "%s: level %d step %d is outside the component", fn, (int)level, (int)step);
  const int entry = t->step_first[level][step];
  if (t->table[entry].g_w < 0)
    return fail(GBNF_ERR_INVALID, "%s: level %d step %d is a permutation: it has no perm_weight to compose into", fn, (int)level, (int)step);
  ImageStepState::Lu b{(int)level, (int)step, entry, p, sign_s, lower, upper, log_s};
  bool found = false;
  for (auto& o : t->step->lu)
    if (o.entry == entry) { o = b; found = true; }
  if (!found) t->step->lu.push_back(b);
  return rebuild(t);
}

int gbnf_image_trainer_bind_top(gbnf_image_trainer* t, float* weight_or_null, float* bias, float* logs) {
  const char* fn = "gbnf_image_trainer_bind_top";
  if (!t || !t->step) return fail(GBNF_ERR_INVALID, "%s: trainer is null", fn);
  if (!bias || !logs) return fail(GBNF_ERR_INVALID, "%s: bias / logs is null", fn);
  t->step->top_weight = weight_or_null; t->step->top_bias = bias; t->step->top_logs = logs;
  return rebuild(t);
}

int gbnf_image_trainer_step_grad_floats(const gbnf_image_trainer* t, int64_t* floats) {
  if (!t || !t->step || !floats) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_step_grad_floats: bad argument");
  if (!t->step->ready) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_step_grad_floats: the last bind call failed: bind again first");
  *floats = t->step->step_grad_floats;
  return GBNF_OK;
}

int gbnf_image_trainer_step_workspace_bytes(const gbnf_image_trainer* t, int64_t n, int64_t* bytes) {
  if (!t || !t->step || !bytes || n < 0) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_step_workspace_bytes: bad argument");
  ImageStepLayout L;
  if (const int rc = image_step_layout(t, n, &L)) return rc;
  *bytes = L.total;
  return GBNF_OK;
}

int gbnf_image_trainer_apply_update(gbnf_image_trainer* t, const float* grads, float* exp_avg, float* exp_avg_sq, const gbnf_opt_hyper* h,
                                    float* stats_dev, void* stream) {
  const char* fn = "gbnf_image_trainer_apply_update";
  if (!t || !t->step || !grads || !stats_dev) return fail(GBNF_ERR_INVALID, "%s: trainer / grads / stats_dev is null", fn);
  if (!t->step->ready) return fail(GBNF_ERR_INVALID, "%s: the last bind call failed: bind again first", fn);
  if (const int rc = check_hyper(fn, h, exp_avg, exp_avg_sq)) return rc;
  return opt_launch_update(fn, update_view(t), grads, exp_avg, exp_avg_sq, h, stats_dev, update_partials(t->step), nullptr, 0, 0.0, 0.0,
                           stream);
}

int gbnf_image_trainer_bind_ycond(gbnf_image_trainer* t, int32_t y_classes, float* cond_w, float* cond_b, float* cond_logs, float* class_w,
                                  float* class_b, float* class_logs) {
  const char* fn = "gbnf_image_trainer_bind_ycond";
  if (!t || !t->step) return fail(GBNF_ERR_INVALID, "%s: trainer is null", fn);
  if (y_classes < 1) return fail(GBNF_ERR_INVALID, "%s: y_classes = %d (must be >= 1)", fn, (int)y_classes);
  if (y_classes > YC_MAX_CLASSES) return fail(GBNF_ERR_UNSUPPORTED, "%s: y_classes = %d > %d", fn, (int)y_classes, YC_MAX_CLASSES);
  if (t->zC > YC_MAX_CZ) return fail(GBNF_ERR_UNSUPPORTED, "%s: %d top channels > %d", fn, t->zC, YC_MAX_CZ);
  if (!cond_w || !cond_b || !cond_logs || !class_w || !class_b || !class_logs)
    return fail(GBNF_ERR_INVALID, "%s: a project_ycond / project_class tensor is null", fn);
  ImageStepState* s = t->step;
  s->y_classes = y_classes;
  s->yc[0] = cond_w; s->yc[1] = cond_b; s->yc[2] = cond_logs; s->yc[3] = class_w; s->yc[4] = class_b; s->yc[5] = class_logs;
  return rebuild(t);
}

int gbnf_image_trainer_y_classes(const gbnf_image_trainer* t, int32_t* y_classes) {
  if (!t || !t->step || !y_classes) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_y_classes: bad argument");
  *y_classes = t->step->y_classes;
  return GBNF_OK;
}

// gbnf_image_trainer_nll_step (y null: refused on a conditioned trainer) and gbnf_image_trainer_nll_step_y (y non-null)
static int image_nll_step(const char* fn, bool want_y, gbnf_image_trainer* t, const float* x, const float* noise, const float* y, int64_t n,
                          float loss_scale, float y_weight, float* grads, float* exp_avg, float* exp_avg_sq, const gbnf_opt_hyper* h,
                          float* stats_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!t || !t->step || !x || !grads || !stats_dev || !workspace)
    return fail(GBNF_ERR_INVALID, "%s: trainer / x / grads / stats_dev / workspace is null", fn);
  if (!t->step->ready) return fail(GBNF_ERR_INVALID, "%s: the last bind call failed: bind again first", fn);
  if (!want_y && t->step->y_classes > 0)
    return fail(GBNF_ERR_INVALID, "%s: the trainer is class-conditional: it needs y (gbnf_image_trainer_nll_step_y)", fn);
  if (want_y && t->step->y_classes == 0)
    return fail(GBNF_ERR_INVALID, "%s: no conditioning bound (gbnf_image_trainer_bind_ycond)", fn);
  if (want_y && !y) return fail(GBNF_ERR_INVALID, "%s: y is null", fn);
  // (with these checks gbnf_image_trainer_forward / _backward below have nothing left to refuse: their own refusals are a null x /
  // ldj / trace, n outside [1, 65535] and a workspace below gbnf_image_trainer_workspace_bytes, which the step layout contains)
  if (n < 1 || n > 65535) return fail(GBNF_ERR_INVALID, "%s: n = %lld (1 to 65535 images per call)", fn, (long long)n);
  if (const int rc = check_hyper(fn, h, exp_avg, exp_avg_sq)) return rc;
  ImageStepLayout L;
  if (const int rc = image_step_layout(t, n, &L)) return rc;
  if (workspace_bytes < L.total)
    return fail(GBNF_ERR_INVALID, "%s: workspace too small: %lld bytes < %lld (gbnf_image_trainer_step_workspace_bytes)", fn,
                (long long)workspace_bytes, (long long)L.total);
  if (mix_allow_lds() != hipSuccess) return fail(GBNF_ERR_HIP, "%s: the 1x1 kernels' LDS opt-in failed", fn);
  const ImageStepState* st = t->step;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* z = (float*)(ws + L.z);
  float* ldj = (float*)(ws + L.ldj);
  float* trace = (float*)(ws + L.trace);
  float* g_z = (float*)(ws + L.g_z);
  float* g_ldj = (float*)(ws + L.g_ldj);
  double* nll_part = (double*)(ws + L.partials);
  double* mu_part = nll_part + OPT_MAX_PARTIALS;
  double* lv_part = mu_part + OPT_MAX_PARTIALS;
  double* grad_part = lv_part + OPT_MAX_PARTIALS;

  MixLaunch mq{};
  mq.steps = st->mix_dev; mq.n_mix = st->n_mix; mq.ld = ld_sums(st); mq.k = loss_scale; mq.grads = grads;
  if (st->n_mix > 0)
    hipLaunchKernelGGL((img_mix_logdet_kernel<0>), dim3((unsigned)st->n_mix), dim3(IOPT_THREADS), MIX_LDS_BYTES, s, mq);
  int rc = gbnf_image_trainer_forward(t, x, noise, n, z, ldj, trace, ws + L.ws, L.ws_bytes, stream);
  if (rc) return rc;

  SeedLaunch sq{};
  sq.z = z; sq.ldj = ldj; sq.ld = ld_sums(st); sq.n_mix = st->n_mix; sq.top_bias = st->top_bias; sq.top_logs = st->top_logs;
  sq.n = n; sq.Cz = t->zC; sq.HW = t->zH * t->zW;
  const int64_t per_channel = (n * sq.HW + 4 * IOPT_THREADS - 1) / (4 * IOPT_THREADS);
  sq.bpc = (int)std::max<int64_t>(1, std::min<int64_t>(OPT_MAX_PARTIALS / sq.Cz, per_channel));
  sq.kn = (float)((double)loss_scale / (double)n);
  sq.g_z = g_z; sq.g_ldj = g_ldj; sq.nll_part = nll_part; sq.mu_part = mu_part; sq.lv_part = lv_part;
  YCond yc{};
  YCondTerms yt{};
  if (want_y) {
    // the per-image prior, the class head and the cross-entropy: one workgroup per image leaves the seed and the image's terms
    yc.top_bias = st->top_bias; yc.top_logs = st->top_logs;
    yc.cond_w = st->yc[0]; yc.cond_b = st->yc[1]; yc.cond_logs = st->yc[2]; yc.class_w = st->yc[3]; yc.class_b = st->yc[4]; yc.class_logs = st->yc[5];
    yc.Y = st->y_classes; yc.Cz = t->zC; yc.HW = sq.HW;
    yt = ycond_terms(ws + L.yterms, n, yc.Y, yc.Cz);
    ycond_launch_seed(yc, z, ldj, ld_sums(st), st->n_mix, y, n, sq.kn, (float)((double)y_weight / (double)n), g_z, g_ldj, yt, s);
  } else {
    hipLaunchKernelGGL(img_nll_seed_kernel, dim3((unsigned)sq.bpc, (unsigned)sq.Cz), dim3(IOPT_THREADS), 0, s, sq);
  }
  hipError_t e = hipMemsetAsync(grads, 0, (size_t)st->step_grad_floats * 4, s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  rc = gbnf_image_trainer_backward(t, trace, n, g_z, g_ldj, grads, ws + L.ws, L.ws_bytes, stream);
  if (rc) return rc;
  const bool top = st->top_bias != nullptr && !want_y;        // (conditioned: the top prior's gradient has per-image terms, below)
  if (st->n_mix > 0 || top) {
    mq.top = TopPrior{top ? st->top_bias : nullptr, st->top_logs, st->g_top_bias, st->g_top_logs, t->zC};
    mq.mu_part = mu_part; mq.lv_part = lv_part; mq.bpc = sq.bpc;
    hipLaunchKernelGGL((img_mix_logdet_kernel<1>), dim3((unsigned)(st->n_mix + (top ? 1 : 0))), dim3(IOPT_THREADS), MIX_LDS_BYTES, s, mq);
  }
  if (want_y) {
    const YCondRegions yr{st->top_bias ? st->g_top_bias : -1, st->g_top_logs, st->g_yc[0], st->g_yc[1], st->g_yc[2], st->g_yc[3], st->g_yc[4],
                          st->g_yc[5]};
    ycond_launch_reduce(yc, y, n, yt, yr, grads, nll_part, stats_dev, s);
    return opt_launch_update(fn, update_view(t), grads, exp_avg, exp_avg_sq, h, stats_dev, grad_part, nll_part, 1, 1.0 / (double)n, 0.0,
                             stream);
  }
  return opt_launch_update(fn, update_view(t), grads, exp_avg, exp_avg_sq, h, stats_dev, grad_part, nll_part, sq.bpc * sq.Cz,
                           1.0 / (double)n, 0.0, stream);
}

int gbnf_image_trainer_nll_step(gbnf_image_trainer* t, const float* x, const float* noise, int64_t n, float loss_scale, float* grads,
                                float* exp_avg, float* exp_avg_sq, const gbnf_opt_hyper* h, float* stats_dev, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  return image_nll_step("gbnf_image_trainer_nll_step", false, t, x, noise, nullptr, n, loss_scale, 0.0f, grads, exp_avg, exp_avg_sq, h,
                        stats_dev, workspace, workspace_bytes, stream);
}

int gbnf_image_trainer_nll_step_y(gbnf_image_trainer* t, const float* x, const float* noise, const float* y, int64_t n, float loss_scale,
                                  float y_weight, float* grads, float* exp_avg, float* exp_avg_sq, const gbnf_opt_hyper* h, float* stats_dev,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  return image_nll_step("gbnf_image_trainer_nll_step_y", true, t, x, noise, y, n, loss_scale, y_weight, grads, exp_avg, exp_avg_sq, h,
                        stats_dev, workspace, workspace_bytes, stream);
}

}  // extern "C"
