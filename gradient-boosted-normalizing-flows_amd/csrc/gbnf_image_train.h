// gbnf_image_train.h -- the image trainer (gbnf_image_train.hip) as the one-call training step (gbnf_image_opt.hip) sees it; not part
// of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "../../include/gbnf.h"

namespace gbnf {

// One convolution of the component -- or the 1x1 "mix" of a FlowStep (ActNorm2d then invconv / permutation) -- as the pack, weight
// gradient and unfold kernels see it.  Parameter pointers are the caller's live device arrays.
struct TConv {
  const float* w;          // (cout, cin, ks, ks); mix: the C x C matrix (perm_weight, or the 0/1 matrix of a permutation)
  const float* bias;       // Conv2dZeros bias or null
  const float* an_bias;    // ActNorm2d behind a Conv2d, or null; mix: the step's ActNorm2d bias
  const float* an_logs;    //   ... logs
  const float* logs;       // Conv2dZeros logs or null
  int cout, cin, ks, mix;
  int64_t fwd_off, bwd_off, b_off;                            // floats into the pack blob: forward tiles, adjoint tiles, folded bias
  int64_t gw_off, gb_off;                                     // floats into the (dW', db') scratch
  int64_t g_w, g_bias, g_an_bias, g_an_logs, g_logs;          // floats into the flat gradient buffer, -1 = absent
  float hw;                // mix: pixels of the level's map (its ActNorm2d log-det is hw * sum(logs))
};

// The state of gbnf_image_trainer_nll_step / _apply_update: the LU and top-prior bindings, the region table of the update kernel, the
// trainer-owned partial sums.  Built at the end of gbnf_image_trainer_create and rebuilt by every bind call (so that a step allocates
// and copies nothing); freed by gbnf_image_trainer_destroy.  gbnf_image_opt.hip
struct ImageStepState;
int image_step_state_create(gbnf_image_trainer* t);
void image_step_state_destroy(ImageStepState* s);
// step 1 of gbnf_image_trainer_nll_step for gbnf_image_trainer_actnorm_init: with LU factors bound, the 1x1 matrices are composed
// into their bound tensors on `stream` (the same launch); nothing bound: nothing launched
int image_step_compose(const gbnf_image_trainer* t, void* stream);

// What gbnf_image_mixture_score (gbnf_image_score.hip) needs of a trainer's bindings to form ll on the device as the one-call step
// does: the 1x1 log-dets (hw log|det W| per bound matrix, doubles, written by image_score_logdets), the live top prior (null: zero
// mean, unit variance) and the conditioning (y_classes 0: none; yc: cond weight, bias, logs, class weight, bias, logs)
struct ImageScoreTop {
  const double* ld;
  int n_mix;
  const float* top_bias;
  const float* top_logs;
  int y_classes;
  const float* yc[6];
};
// GBNF_ERR_INVALID when the trainer's last bind call failed; launches nothing
int image_score_top(const char* fn, const gbnf_image_trainer* t, ImageScoreTop* out);
// step 1 of gbnf_image_trainer_nll_step: LU matrices composed into their bound tensors, every 1x1 log-det into `ld`
int image_score_logdets(const char* fn, const gbnf_image_trainer* t, void* stream);

// The adjoint of img_pre_body (gbnf_image.hip): gs (n, 4C, H/2, W/2) storage, the gradient of the squeezed logits, and g_ldj (n,) ->
// g_x (n, C, Hi, Wi), stored or added; v is recomputed from x and noise as the forward does (gbnf_image_score.hip)
void img_launch_pre_adjoint(const float* x, const float* noise, const float* gs, const float* g_ldj, float* g_x, int C, int H, int W, int Hi,
                            int Wi, float bounds, int accumulate, int64_t n, hipStream_t s);

}  // namespace gbnf

struct gbnf_image_trainer {
  int C = 0, H = 32, W = 32, Hi = 0, Wi = 0, L = 0, hidden = 0, additive = 0;
  float bounds = 0.9f;
  double ld_const = 0;                         // dequantisation only: everything else is read from the live parameters
  struct Level { int C, H, W, Hv, Wv, K; };
  std::vector<Level> levels;
  std::vector<gbnf::TConv> table;                    // per level: per step [mix, convs ...], then the split prior
  std::vector<std::vector<int>> step_first;    // [level][step] -> index of the step's mix entry (its convs follow)
  std::vector<int> step_convs;                 // convolutions of a step's net
  std::vector<int> split_entry;                // [level] -> entry or -1
  gbnf::TConv* table_dev = nullptr;
  gbnf::TConv* ident_dev = nullptr;            // the table with every ActNorm2d behind a Conv2d taken out (null arrays): the identity tiles
                                               // gbnf_image_trainer_actnorm_init packs for a layer it has yet to initialise
  float* blob_dev = nullptr;                   // packs; [zero_off, zero_off + 1024): zeros (bias of the adjoint launches, the prior)
  float* perm_dev = nullptr;                   // the 0/1 matrices of Permute2d steps
  int64_t blob_floats = 0, zero_off = 0, scratch_floats = 0, grad_floats = 0;
  int zC = 0, zH = 0, zW = 0;
  int n_net = 0;                               // convolutions per coupling net
  int64_t state_img = 0;                       // floats of the largest state tensor of one image
  int64_t trace_img = 0;                       // trace floats per image
  int deterministic = 0;                       // gbnf_image_trainer_set_deterministic: ordered weight-gradient and log-det sums; the
                                               // workspace then ends with the log-det slots and the weight-gradient partials
  gbnf::ImageStepState* step = nullptr;       // what the one-call training step adds (gbnf_image_opt.hip): bindings, region table, partial sums
};

