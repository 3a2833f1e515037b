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
// What every call that ends in an update refuses before it launches anything (GBNF_ERR_INVALID: null hyper, unknown kind, AdamW with
// step <= 0 or without state); `fn` names the entry point in the message.  gbnf_opt.hip
int check_hyper(const char* fn, const gbnf_opt_hyper* h, const float* m, const float* v);

}  // namespace gbnf
