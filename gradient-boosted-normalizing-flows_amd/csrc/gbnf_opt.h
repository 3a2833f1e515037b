// gbnf_opt.h -- the tail of a training step (gbnf_opt.hip) on what a trainer (gbnf_train.hip) binds; not part of the C ABI.
#pragma once
#include <cstdint>
#include "../../include/gbnf.h"

namespace gbnf {

// One bound parameter tensor in the flat gradient-buffer layout (gbnf_trainer_grad_floats).  The trainer builds the table at creation,
// sorted by offset; a reserved region (a RealNVP step without BatchNorm) has no entry.  Lengths and offsets are arbitrary (215 * 21).
struct OptRegion {
  float* p;
  int64_t off, len;
};
constexpr int OPT_MAX_PARTIALS = 256;   // per-workgroup sums a reduction's producer leaves for its consumer
constexpr int OPT_MAX_BN_STEPS = 32;    // steps of a batch-statistics sweep (gbnf_trainer_set_batch_stats)
// The steps whose BatchNorm has batch-statistics buffers bound: running statistics and the batch's, (d,) device arrays each
struct OptBnTable {
  float* mean[OPT_MAX_BN_STEPS];
  float* var[OPT_MAX_BN_STEPS];
  const float* bmean[OPT_MAX_BN_STEPS];
  const float* bvar[OPT_MAX_BN_STEPS];
  int n;
};
struct TrainerOptView {
  const OptRegion* regions_dev;
  int n_regions;
  int64_t grad_floats;
  int d, K;
  int batch_stats;          // the trainer normalises with batch statistics
  double* partials_dev;     // OPT_MAX_PARTIALS sums, trainer-owned: gbnf_trainer_apply_update has no workspace argument
  OptBnTable bn;
};
int trainer_opt_view(const gbnf_trainer* t, TrainerOptView* out);
// Deterministic mode (gbnf_trainer_set_deterministic): GBNF_ERR_UNSUPPORTED, with the reason, if a backward call of n rows (traced: with
// the forward call's trace) would run kernels with unordered float accumulation; GBNF_OK otherwise and with the mode off.  Launches
// nothing: a one-call step asks before its first launch.  gbnf_train.hip
int trainer_deterministic_check(const gbnf_trainer* t, int64_t n, bool traced, const char* fn);
// What the norm + update launches need, for an owner that is not a gbnf_trainer (the image trainer, gbnf_image_opt.hip): the region
// table on the device (sorted by offset, reserved regions not listed) and the floats of the flat gradient buffer.
struct OptUpdateView {
  const OptRegion* regions_dev;
  int n_regions;
  int64_t grad_floats;
};
// grad_sqsum_kernel into `partials` (OPT_MAX_PARTIALS doubles), then opt_update_kernel: the clip coefficient, the update of every
// region's tensor in place, stats[1..3]; with nll_partial, stats[0] = sum(nll_partial) * nll_scale + nll_const.  Two launches on
// `stream` (a hipStream_t), no host read.  `fn` names the entry point in a launch error.  gbnf_opt.hip
int opt_launch_update(const char* fn, const OptUpdateView& view, const float* grads, float* m, float* v, const gbnf_opt_hyper* h,
                      float* stats, double* partials, const double* nll_partial, int n_nll_partial, double nll_scale, double nll_const,
                      void* stream);
// The two launches of opt_launch_update one by one, for a caller whose clip coefficient spans more than one gradient buffer (the
// mixture step, gbnf_mixstep.hip).  opt_launch_grad_sqsum: grad_sqsum_kernel into `partials`; returns how many it wrote (at most
// OPT_MAX_PARTIALS, a function of grad_floats alone).  opt_launch_update_from: opt_update_kernel on squared-norm sums that are in
// memory already -- it re-adds grad_partial[0 .. n_grad_partial) in a fixed order, whoever wrote them (one double: a finished sum).
int opt_launch_grad_sqsum(const float* grads, int64_t grad_floats, double* partials, void* stream);
int opt_launch_update_from(const char* fn, const OptUpdateView& view, const float* grads, float* m, float* v, const gbnf_opt_hyper* h,
                           float* stats, const double* grad_partial, int n_grad_partial, const double* nll_partial, int n_nll_partial,
                           double nll_scale, double nll_const, void* stream);
// Workgroups of a reduction's producer over `work` entries: one per 1024, at least 1, at most OPT_MAX_PARTIALS.  gbnf_opt.hip
unsigned opt_partial_blocks(int64_t work);
// What every call that ends in an update refuses before it launches anything (GBNF_ERR_INVALID: null hyper, unknown kind, AdamW with
// step <= 0 or without state); `fn` names the entry point in the message.  gbnf_opt.hip
int check_hyper(const char* fn, const gbnf_opt_hyper* h, const float* m, const float* v);

}  // namespace gbnf
