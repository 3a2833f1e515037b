// gbnf_image_ycond.h -- the class-conditional top of an image Glow component (gbnf_image_ycond.hip) as the evaluation handle
// (gbnf_image.hip) and the one-call training step (gbnf_image_opt.hip) see it; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gbnf {

constexpr int YC_MAX_CLASSES = 256;     // y_classes of a conditioned component (gbnf_image_flow_set_ycond / gbnf_image_trainer_bind_ycond)
constexpr int YC_MAX_CZ = 64;           // channels of the top latent (the handles refuse wider levels)

// project_ycond / project_class (LinearZeros: (x W^T + b) e^{3 logs}, models/layers.py:560-574) and the constant part of the prior.
// All pointers are DEVICE pointers.
struct YCond {
  const float* top_h;       // (2 Cz,) learn_top_fn's output as the evaluation handle packed it, or null
  const float* top_bias;    // ... or its live bias and logs (the trainer): top_h = bias e^{3 logs}; both null: zeros
  const float* top_logs;
  const float* cond_w;      // (2 Cz, Y)
  const float* cond_b;      // (2 Cz,)
  const float* cond_logs;   // (2 Cz,)
  const float* class_w;     // (Y, Cz), or null: no class head (evaluation only)
  const float* class_b;     // (Y,)
  const float* class_logs;  // (Y,)
  int Y, Cz, HW;            // HW: the map proper (z is stored compactly: (n, Cz, HW))
};

// What the per-image kernel leaves for the reduction kernel: doubles, [image][entry] each
struct YCondTerms {
  double* g_h;      // (n, 2 Cz)   gradient of the image's prior (mean half, log-variance half)
  double* u;        // (n, 2 Cz)   y W_c^T + b_c
  double* zbar;     // (n, Cz)
  double* gl;       // (n, Y)      (y_weight / n) (softmax - onehot)
  double* logits;   // (n, Y)
  double* loss;     // (n, 3)      nll_i, CE_i, correct_i
};
int64_t ycond_terms_bytes(int64_t n, int Y, int Cz);
YCondTerms ycond_terms(void* base, int64_t n, int Y, int Cz);

// Where the gradient regions live in the flat buffer (floats); g_top_bias < 0: no learn_top
struct YCondRegions {
  int64_t g_top_bias, g_top_logs, g_cond_w, g_cond_b, g_cond_logs, g_class_w, g_class_b, g_class_logs;
};

// evaluation: ll[i] = log N(z_i; mu_i, lv_i) + ldj[i] and, with a class head and a non-null `logits`, y_logits (n, Y)
void ycond_launch_eval(const YCond& c, const float* z, const float* ldj, const float* y, int64_t n, float* ll, float* logits, hipStream_t s);
// evaluation under EVERY class: table[i, k] = log N(z_i; mu(e_k), lv(e_k)) + ldj[i] ((n, Y): what ycond_launch_eval writes to ll[i] for
// y_i = the one-hot row of class k) and, with a class head and a non-null `logits`, y_logits (n, Y) -- one launch, no y
void ycond_launch_table(const YCond& c, const float* z, const float* ldj, int64_t n, float* table, float* logits, hipStream_t s);
// training: nll_i, CE_i, the autograd seed g_z / g_ldj of loss_scale mean(nll) + y_weight mean(CE), the per-image terms.
// ld: [n_mix] doubles added to every image's log-det (the 1x1 matrices'), or null
void ycond_launch_seed(const YCond& c, const float* z, const float* ldj, const double* ld, int n_mix, const float* y, int64_t n, float kn,
                       float ywn, float* g_z, float* g_ldj, const YCondTerms& t, hipStream_t s);
// the per-image terms added in image order: the eight gradient regions are WRITTEN, nll_sum[0] = sum nll_i, stats[4..7]
void ycond_launch_reduce(const YCond& c, const float* y, int64_t n, const YCondTerms& t, const YCondRegions& r, float* grads, double* nll_sum,
                         float* stats, hipStream_t s);
// the per-image prior (n, 2 Cz) and / or the top latent z = mu + exp(lv) temperature e (models/glow.py:116, as written)
void ycond_launch_prior(const YCond& c, const float* y, int64_t n, const float* e, float temperature, float* mean_logvar, float* z_out,
                        hipStream_t s);

}  // namespace gbnf
