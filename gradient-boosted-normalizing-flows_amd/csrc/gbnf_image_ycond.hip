// gbnf_image_ycond.hip -- the class-conditional top of an image Glow component on the device (gfx950): what `--y_condition` adds to
// the reference's Glow (models/glow.py:36-39, 62-84, 105-106) and to its loss (image_experiment.py:227-239).
//
//   prior    u = y W_c^T + b_c, h_i = top_h + u_i e^{3 l_c}: a mean and a log-variance per image and channel, constant over the map
//   head     zbar = the mean of z over the map, y_logits = (zbar W_k^T + b_k) e^{3 l_k}
//   loss     loss_scale mean_i nll_i + y_weight mean_i CE(y_logits_i, argmax y_i)
//
//   img_ycond_image_kernel<TRAIN>   one workgroup per image.  Evaluation: ll_i and the logits.  Training: nll_i, CE_i, the correct flag,
//                                   the seed g_z / g_ldj of the whole loss and the image's terms of every parameter gradient
//   img_ycond_reduce_kernel         one thread per parameter entry: the images' terms added in image order in f64 -> the gradient
//                                   regions of the top prior, project_ycond and project_class, the loss sums, stats[4..7]
//   img_ycond_prior_kernel          the per-image prior and the top latent of a class-conditional draw
//   img_ycond_table_kernel          one workgroup per image: ll_i under EVERY class (n, Y) from per-channel mean and centred second
//                                   moment of z -- the flow does not depend on y, so one forward serves all classes -- and the logits
//
// z is the compact top latent (n, Cz, HW of the map proper): nothing here sees the padding of the storage.  Everything is small and
// latency-bound: no MFMA, no atomics; every sum runs in f64 in an order the sizes alone decide, so every value written here is
// bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gbnf_image_ycond.h"

namespace gbnf {

constexpr int YC_THREADS = 256;
static_assert(YC_MAX_CLASSES <= YC_THREADS && 2 * YC_MAX_CZ <= YC_THREADS, "one thread per class / prior entry");

__device__ __forceinline__ double yc_wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// the largest of the wave's (value, index) pairs, the lowest index on a tie (a NaN never wins); every lane gets it
__device__ __forceinline__ int yc_wave_argmax(float v, int at) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const float ov = __shfl_xor(v, m);
    const int oi = __shfl_xor(at, m);
    if (oi >= 0 && (at < 0 || ov > v || (ov == v && oi < at))) { v = ov; at = oi; }
  }
  return at;
}

// lane-strided argmax of a[0 .. len) by one wave: torch.argmax's first-of-the-largest
__device__ __forceinline__ int yc_argmax(const float* a, int len, int lane) {
  float v = 0.0f;
  int at = -1;
  for (int k = lane; k < len; k += 64) {
    const float w = a[k];
    if (at < 0 || w > v) { v = w; at = k; }
  }
  at = yc_wave_argmax(v, at);
  return at < 0 ? 0 : at;
}

// ys: the image's y row; -> hs[2 Cz] (the prior) and us[2 Cz] (u) in LDS.  Threads [0, 2 Cz) work; the caller synchronises.
__device__ __forceinline__ void yc_prior(const YCond& c, const float* ys, double* hs, double* us) {
  const int j = threadIdx.x;
  if (j >= 2 * c.Cz) return;
  double acc = 0.0;
  for (int k = 0; k < c.Y; ++k) acc = fma((double)ys[k], (double)c.cond_w[(int64_t)j * c.Y + k], acc);
  acc += (double)c.cond_b[j];
  double top = 0.0;
  if (c.top_h != nullptr) top = (double)c.top_h[j];
  else if (c.top_bias != nullptr) top = (double)c.top_bias[j] * exp(3.0 * (double)c.top_logs[j]);
  us[j] = acc;
  hs[j] = top + acc * exp(3.0 * (double)c.cond_logs[j]);
}

struct YImage {
  YCond c;
  const float* z;           // (n, Cz, HW)
  const float* ldj;         // (n,)
  const double* ld;         // [n_mix] or null
  int n_mix;
  const float* y;           // (n, Y)
  float kn, ywn;            // loss_scale / n, y_weight / n
  float* g_z;               // TRAIN
  float* g_ldj;
  YCondTerms t;
  float* ll;                // evaluation
  float* logits;            // evaluation, or null
};

template <bool TRAIN>
__global__ void __launch_bounds__(YC_THREADS) img_ycond_image_kernel(const YImage q) {
  __shared__ float ys[YC_MAX_CLASSES];
  __shared__ float lf[YC_MAX_CLASSES];
  __shared__ double hs[2 * YC_MAX_CZ], us[2 * YC_MAX_CZ];
  __shared__ double zb[YC_MAX_CZ], nl[YC_MAX_CZ], vs[YC_MAX_CZ];
  __shared__ double lg[YC_MAX_CLASSES], sks[YC_MAX_CLASSES], gls[YC_MAX_CLASSES];
  const YCond& c = q.c;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Y = c.Y, Cz = c.Cz, HW = c.HW;
  const int64_t i = blockIdx.x;
  if (tid < Y) ys[tid] = q.y[i * Y + tid];
  __syncthreads();
  yc_prior(c, ys, hs, us);
  __syncthreads();
  // ---- per channel: the sums over the map (a wave per channel, lanes over the pixels) ----
  const float* zi = q.z + i * (int64_t)Cz * HW;
  for (int ch = wave; ch < Cz; ch += YC_THREADS / 64) {
    const double mu = hs[ch], lv = hs[Cz + ch], e = exp(-lv);
    double s_z = 0.0, s_d = 0.0, s_dd = 0.0;
    for (int p = lane; p < HW; p += 64) {
      const double zv = (double)zi[(int64_t)ch * HW + p], d = zv - mu;
      s_z += zv;
      s_d += d * e;
      s_dd += d * d * e;
    }
    s_z = yc_wave_sum(s_z); s_d = yc_wave_sum(s_d); s_dd = yc_wave_sum(s_dd);
    if (lane == 0) {
      zb[ch] = s_z / (double)HW;
      nl[ch] = 0.5 * ((double)HW * lv + s_dd);
      if (TRAIN) {
        q.t.g_h[i * 2 * Cz + ch] = -(double)q.kn * s_d;
        q.t.g_h[i * 2 * Cz + Cz + ch] = (double)q.kn * 0.5 * ((double)HW - s_dd);
      }
    }
  }
  __syncthreads();
  const bool head = c.class_w != nullptr;
  if (head && tid < Y) {
    double acc = 0.0;
    for (int ch = 0; ch < Cz; ++ch) acc = fma(zb[ch], (double)c.class_w[(int64_t)tid * Cz + ch], acc);
    const double sk = exp(3.0 * (double)c.class_logs[tid]);
    const double l = (acc + (double)c.class_b[tid]) * sk;
    sks[tid] = sk;
    lg[tid] = l;
    lf[tid] = (float)l;
    if (!TRAIN && q.logits != nullptr) q.logits[i * Y + tid] = (float)l;
  }
  if (tid == 0) {
    double s = 0.0;
    for (int ch = 0; ch < Cz; ++ch) s += nl[ch];
    double ldv = (double)q.ldj[i];
    if (q.ld != nullptr)
      for (int m = 0; m < q.n_mix; ++m) ldv += q.ld[m];
    if (TRAIN) {
      q.t.loss[i * 3] = s - ldv;
      q.g_ldj[i] = -q.kn;
    } else {
      q.ll[i] = (float)(ldv - s);
    }
  }
  if (!TRAIN) return;
  __syncthreads();
  // ---- cross-entropy against t = argmax y (wave 0), the logits' gradient ----
  if (wave == 0) {
    const int t = yc_argmax(ys, Y, lane), best = yc_argmax(lf, Y, lane);
    // (the f32 logits decide `correct`, as torch's argmax of an f32 tensor does; the maximum below only stabilises the sum)
    const double m = lg[best];
    double se = 0.0;
    for (int k = lane; k < Y; k += 64) se += exp(lg[k] - m);
    se = yc_wave_sum(se);
    const double lse = m + log(se);
    for (int k = lane; k < Y; k += 64) {
      const double g = (double)q.ywn * (exp(lg[k] - lse) - (k == t ? 1.0 : 0.0));
      gls[k] = g * sks[k];                                    // (gl sk): what the class loss hands back to z
      q.t.gl[i * Y + k] = g;
      q.t.logits[i * Y + k] = lg[k];
    }
    if (lane == 0) {
      q.t.loss[i * 3 + 1] = lse - lg[t];
      q.t.loss[i * 3 + 2] = best == t ? 1.0 : 0.0;
    }
  }
  if (tid < 2 * Cz) q.t.u[i * 2 * Cz + tid] = us[tid];
  if (tid < Cz) q.t.zbar[i * Cz + tid] = zb[tid];
  __syncthreads();
  if (tid < Cz) {                                             // the class loss's share of g_z: ((gl sk) W_k)[c] / HW
    double acc = 0.0;
    for (int k = 0; k < Y; ++k) acc = fma(gls[k], (double)c.class_w[(int64_t)k * Cz + tid], acc);
    vs[tid] = acc / (double)HW;
  }
  __syncthreads();
  float* gi = q.g_z + i * (int64_t)Cz * HW;
  for (int idx = tid; idx < Cz * HW; idx += YC_THREADS) {
    const int ch = idx / HW;
    const float d = zi[idx] - (float)hs[ch];
    gi[idx] = q.kn * d * expf(-(float)hs[Cz + ch]) + (float)vs[ch];
  }
}

struct YTable {
  YCond c;
  const float* z;           // (n, Cz, HW)
  const float* ldj;         // (n,)
  float* table;             // (n, Y)
  float* logits;            // (n, Y), or null
};

// One workgroup per image, every class at once.  The class moves the prior only, and the prior is constant over the map: with zbar_c the
// channel's mean and M2_c = sum_p (z - zbar_c)^2,
//   sum_p (z - mu)^2 = M2_c + HW (zbar_c - mu)^2        (two non-negative terms: nothing cancels, whatever mu is)
// so z is read twice per image (a wave per channel, lanes over the pixels, as img_ycond_image_kernel) and a class then costs Cz terms
// instead of Cz HW: thread k adds class k's channels in channel order.  The prior of class k is yc_prior's for y = e_k (its fma chain
// over a one-hot row leaves W_c[:, k] + b_c exactly), zbar and the logits are img_ycond_image_kernel's to the bit.
__global__ void __launch_bounds__(YC_THREADS) img_ycond_table_kernel(const YTable q) {
  __shared__ double zb[YC_MAX_CZ], m2[YC_MAX_CZ];
  __shared__ double top[2 * YC_MAX_CZ], cb[2 * YC_MAX_CZ], e3[2 * YC_MAX_CZ];
  const YCond& c = q.c;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Y = c.Y, Cz = c.Cz, HW = c.HW;
  const int64_t i = blockIdx.x;
  if (tid < 2 * Cz) {
    double t = 0.0;
    if (c.top_h != nullptr) t = (double)c.top_h[tid];
    else if (c.top_bias != nullptr) t = (double)c.top_bias[tid] * exp(3.0 * (double)c.top_logs[tid]);
    top[tid] = t;
    cb[tid] = (double)c.cond_b[tid];
    e3[tid] = exp(3.0 * (double)c.cond_logs[tid]);
  }
  const float* zi = q.z + i * (int64_t)Cz * HW;
  for (int ch = wave; ch < Cz; ch += YC_THREADS / 64) {
    const float* zc = zi + (int64_t)ch * HW;
    double s_z = 0.0;
    for (int p = lane; p < HW; p += 64) s_z += (double)zc[p];
    s_z = yc_wave_sum(s_z);
    const double mean = s_z / (double)HW;
    double s_dd = 0.0;
    for (int p = lane; p < HW; p += 64) {
      const double d = (double)zc[p] - mean;
      s_dd = fma(d, d, s_dd);
    }
    s_dd = yc_wave_sum(s_dd);
    if (lane == 0) { zb[ch] = mean; m2[ch] = s_dd; }
  }
  __syncthreads();
  if (tid >= Y) return;
  const double hw = (double)HW;
  double s = 0.0;
  for (int ch = 0; ch < Cz; ++ch) {
    const double mu = top[ch] + ((double)c.cond_w[(int64_t)ch * Y + tid] + cb[ch]) * e3[ch];
    const double lv = top[Cz + ch] + ((double)c.cond_w[(int64_t)(Cz + ch) * Y + tid] + cb[Cz + ch]) * e3[Cz + ch];
    const double dm = zb[ch] - mu;
    s += 0.5 * (hw * lv + (m2[ch] + hw * dm * dm) * exp(-lv));
  }
  q.table[i * Y + tid] = (float)((double)q.ldj[i] - s);
  if (q.logits != nullptr && c.class_w != nullptr) {
    double acc = 0.0;
    for (int ch = 0; ch < Cz; ++ch) acc = fma(zb[ch], (double)c.class_w[(int64_t)tid * Cz + ch], acc);
    q.logits[i * Y + tid] = (float)((acc + (double)c.class_b[tid]) * exp(3.0 * (double)c.class_logs[tid]));
  }
}

struct YReduce {
  YCond c;
  const float* y;
  int64_t n;
  YCondTerms t;
  YCondRegions r;
  float* grads;
  double* nll_sum;
  float* stats;
};

// entries: [top bias 2Cz | top logs 2Cz] (with learn_top) | cond weight 2Cz Y | cond bias 2Cz | cond logs 2Cz | class weight Y Cz |
// class bias Y | class logs Y | nll, CE, correct
__global__ void __launch_bounds__(YC_THREADS) img_ycond_reduce_kernel(const YReduce q) {
  const YCond& c = q.c;
  const int Y = c.Y, Cz = c.Cz, P = 2 * Cz;
  const int64_t n = q.n;
  int64_t e = (int64_t)blockIdx.x * YC_THREADS + threadIdx.x;
  if (q.r.g_top_bias >= 0) {
    if (e < 2 * P) {
      const int j = (int)(e < P ? e : e - P);
      double s = 0.0;
      for (int64_t i = 0; i < n; ++i) s += q.t.g_h[i * P + j];
      const double e3 = exp(3.0 * (double)c.top_logs[j]), h = (double)c.top_bias[j] * e3;
      if (e < P) q.grads[q.r.g_top_bias + j] = (float)(s * e3);
      else q.grads[q.r.g_top_logs + j] = (float)(3.0 * s * h);
      return;
    }
    e -= 2 * P;
  }
  if (e < (int64_t)P * Y) {
    const int j = (int)(e / Y), k = (int)(e - (int64_t)j * Y);
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s = fma(q.t.g_h[i * P + j], (double)q.y[i * Y + k], s);
    q.grads[q.r.g_cond_w + e] = (float)(s * exp(3.0 * (double)c.cond_logs[j]));
    return;
  }
  e -= (int64_t)P * Y;
  if (e < 2 * P) {
    const int j = (int)(e < P ? e : e - P);
    const double sc = exp(3.0 * (double)c.cond_logs[j]);
    double s = 0.0;
    if (e < P) {
      for (int64_t i = 0; i < n; ++i) s += q.t.g_h[i * P + j];
      q.grads[q.r.g_cond_b + j] = (float)(s * sc);
    } else {
      for (int64_t i = 0; i < n; ++i) s = fma(q.t.g_h[i * P + j], q.t.u[i * P + j], s);
      q.grads[q.r.g_cond_logs + j] = (float)(3.0 * s * sc);
    }
    return;
  }
  e -= 2 * P;
  if (e < (int64_t)Y * Cz) {
    const int j = (int)(e / Cz), ch = (int)(e - (int64_t)j * Cz);
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s = fma(q.t.gl[i * Y + j], q.t.zbar[i * Cz + ch], s);
    q.grads[q.r.g_class_w + e] = (float)(s * exp(3.0 * (double)c.class_logs[j]));
    return;
  }
  e -= (int64_t)Y * Cz;
  if (e < 2 * Y) {
    const int j = (int)(e < Y ? e : e - Y);
    double s = 0.0;
    if (e < Y) {
      for (int64_t i = 0; i < n; ++i) s += q.t.gl[i * Y + j];
      q.grads[q.r.g_class_b + j] = (float)(s * exp(3.0 * (double)c.class_logs[j]));
    } else {
      for (int64_t i = 0; i < n; ++i) s = fma(q.t.gl[i * Y + j], q.t.logits[i * Y + j], s);
      q.grads[q.r.g_class_logs + j] = (float)(3.0 * s);
    }
    return;
  }
  e -= 2 * Y;
  if (e < 3) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += q.t.loss[i * 3 + e];
    if (e == 0) { q.nll_sum[0] = s; q.stats[6] = 0.0f; q.stats[7] = 0.0f; }
    else if (e == 1) q.stats[4] = (float)(s / (double)n);
    else q.stats[5] = (float)s;
  }
}

struct YPrior {
  YCond c;
  const float* y;
  const float* e;
  float temperature;
  float* mean_logvar;
  float* z_out;
};

__global__ void __launch_bounds__(YC_THREADS) img_ycond_prior_kernel(const YPrior q) {
  __shared__ float ys[YC_MAX_CLASSES];
  __shared__ double hs[2 * YC_MAX_CZ], us[2 * YC_MAX_CZ];
  const YCond& c = q.c;
  const int tid = threadIdx.x, Cz = c.Cz, HW = c.HW;
  const int64_t i = blockIdx.x;
  if (tid < c.Y) ys[tid] = q.y[i * c.Y + tid];
  __syncthreads();
  yc_prior(c, ys, hs, us);
  __syncthreads();
  if (q.mean_logvar != nullptr && tid < 2 * Cz) q.mean_logvar[i * 2 * Cz + tid] = (float)hs[tid];
  if (q.z_out == nullptr) return;
  for (int idx = tid; idx < Cz * HW; idx += YC_THREADS) {
    const int ch = idx / HW;
    const int64_t at = i * (int64_t)Cz * HW + idx;
    q.z_out[at] = (float)hs[ch] + expf((float)hs[Cz + ch]) * q.temperature * q.e[at];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static int64_t yc_align(int64_t doubles) { return (doubles + 31) / 32 * 32; }

int64_t ycond_terms_bytes(int64_t n, int Y, int Cz) {
  return (2 * yc_align(n * 2 * Cz) + yc_align(n * Cz) + 2 * yc_align(n * Y) + yc_align(n * 3)) * (int64_t)sizeof(double);
}

YCondTerms ycond_terms(void* base, int64_t n, int Y, int Cz) {
  YCondTerms t{};
  double* p = (double*)base;
  t.g_h = p; p += yc_align(n * 2 * Cz);
  t.u = p; p += yc_align(n * 2 * Cz);
  t.zbar = p; p += yc_align(n * Cz);
  t.gl = p; p += yc_align(n * Y);
  t.logits = p; p += yc_align(n * Y);
  t.loss = p;
  return t;
}

void ycond_launch_eval(const YCond& c, const float* z, const float* ldj, const float* y, int64_t n, float* ll, float* logits, hipStream_t s) {
  YImage q{};
  q.c = c; q.z = z; q.ldj = ldj; q.y = y; q.ll = ll; q.logits = logits;
  hipLaunchKernelGGL((img_ycond_image_kernel<false>), dim3((unsigned)n), dim3(YC_THREADS), 0, s, q);
}

void ycond_launch_table(const YCond& c, const float* z, const float* ldj, int64_t n, float* table, float* logits, hipStream_t s) {
  YTable q{};
  q.c = c; q.z = z; q.ldj = ldj; q.table = table; q.logits = logits;
  hipLaunchKernelGGL(img_ycond_table_kernel, dim3((unsigned)n), dim3(YC_THREADS), 0, s, q);
}

void ycond_launch_seed(const YCond& c, const float* z, const float* ldj, const double* ld, int n_mix, const float* y, int64_t n, float kn,
                       float ywn, float* g_z, float* g_ldj, const YCondTerms& t, hipStream_t s) {
  YImage q{};
  q.c = c; q.z = z; q.ldj = ldj; q.ld = ld; q.n_mix = n_mix; q.y = y; q.kn = kn; q.ywn = ywn; q.g_z = g_z; q.g_ldj = g_ldj; q.t = t;
  hipLaunchKernelGGL((img_ycond_image_kernel<true>), dim3((unsigned)n), dim3(YC_THREADS), 0, s, q);
}

void ycond_launch_reduce(const YCond& c, const float* y, int64_t n, const YCondTerms& t, const YCondRegions& r, float* grads, double* nll_sum,
                         float* stats, hipStream_t s) {
  YReduce q{};
  q.c = c; q.y = y; q.n = n; q.t = t; q.r = r; q.grads = grads; q.nll_sum = nll_sum; q.stats = stats;
  const int64_t P = 2 * (int64_t)c.Cz;
  const int64_t entries = (r.g_top_bias >= 0 ? 2 * P : 0) + P * c.Y + 2 * P + (int64_t)c.Y * c.Cz + 2 * c.Y + 3;
  hipLaunchKernelGGL(img_ycond_reduce_kernel, dim3((unsigned)((entries + YC_THREADS - 1) / YC_THREADS)), dim3(YC_THREADS), 0, s, q);
}

void ycond_launch_prior(const YCond& c, const float* y, int64_t n, const float* e, float temperature, float* mean_logvar, float* z_out,
                        hipStream_t s) {
  YPrior q{};
  q.c = c; q.y = y; q.e = e; q.temperature = temperature; q.mean_logvar = mean_logvar; q.z_out = z_out;
  hipLaunchKernelGGL(img_ycond_prior_kernel, dim3((unsigned)n), dim3(YC_THREADS), 0, s, q);
}

}  // namespace gbnf
