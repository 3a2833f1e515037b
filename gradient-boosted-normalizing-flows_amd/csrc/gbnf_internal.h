// gbnf_internal.h -- shared between the translation units of libgbnf_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <initializer_list>
#include "../../include/gbnf.h"

namespace gbnf {

// Records the message behind gbnf_last_error() (thread-local) and returns `code`.
int fail(int code, const char* fmt, ...);

// The CURRENT device's counter of waves that stored a split-f16 operand beyond +-65504 (it saturates there); null if it
// could not be allocated.  Call it at launch time, with the launch's device current.  Read and reset by
// gbnf_saturation_count().
unsigned* saturation_counter();
// The same device's counter of the TRAINING kernels (word [1] of the same allocation): the traced forward sweep, the backward sweep, the
// per-step training kernels and the trainer's weight re-pack count here -- they saturate and have no repair pass, so THIS count means wrong
// gradients, while word [0] (evaluation: every marked sample is re-evaluated in the same call) is a data-quality alarm.  gbnf_saturation_count()
// reports their sum, gbnf_training_saturation_count() this word alone.
unsigned* training_saturation_counter();

// How many components a mixture holds and their feature count, for the translation units that do not see the handle (gbnf_boost.hip)
int mixture_shape(const gbnf_mixture* mix, int* n_components, int* d);
// ... and one component's feature count (gbnf_sample.hip)
int flow_features(const gbnf_flow* flow, int* d);

// The tail of one update_rho iteration (gbnf_boost.hip: rho_partial_kernel + rho_finalize_kernel through the current device's
// partial-sum buffer) on a (component + 1, n) DEVICE table of per-component log-likelihoods: what gbnf_mixture_rho_step and
// gbnf_image_mixture_rho_step (gbnf_image_boost.hip) share.  Writes rho_dev[component] and the 4 floats of stats_dev; no host read.
int rho_update_launch(const char* fn, const float* ll, int64_t n, int component, float* rho_dev, float step_size, float* stats_dev,
                      hipStream_t s);
// The input proper of an image evaluation handle (channels, height, width), for gbnf_image_boost.hip (gbnf_image.hip)
int image_flow_input_shape(const gbnf_image_flow* f, int* channels, int* height, int* width);
// Whether a conditioned handle was given project_class (it can write y_logits), for gbnf_eval.hip (gbnf_image.hip)
bool image_flow_has_class_head(const gbnf_image_flow* f);
// What gbnf_image_mixture_rho_step checks of its handles before the first launch, for the calls built like it (gbnf_eval.hip):
// handles [0, n_flows) non-null and of one input shape;  with_y false: every handle plain, true: every handle conditioned on one
// class count (*y_classes, may be null)  (gbnf_image_boost.hip)
int check_image_flows(const char* fn, const gbnf_image_flow* const* flows, int n_flows);
int check_image_flows_y(const char* fn, const gbnf_image_flow* const* flows, int n_flows, bool with_y, int32_t* y_classes);

// One row of the mixture recursion  G_0 = ll_0;  r_c = rho_c / sum(rho[0..c]);  G_c = LSE2(log(1 - r_c) + G_{c-1}, log r_c + ll_c)
// (density_experiment.py:567-571) in float32 with torch.logsumexp's semantics for the 2-way LSE: the body of mixture_lse_kernel
// (gbnf_api.hip), shared with eval_partial_kernel (gbnf_eval.hip) so that both give the same bits.  The rho prefix sums are
// recomputed per thread (C is tiny, the loads are wave-uniform).
__device__ __forceinline__ float mixture_lse_row(const float* __restrict__ ll, int64_t stride, const float* __restrict__ rho, int n_comp,
                                                 int64_t idx) {
  float G = ll[idx];
  float rsum = rho[0];
  for (int c = 1; c < n_comp; ++c) {
    rsum += rho[c];
    const float r = rho[c] / rsum;
    const float a = logf(1.0f - r) + G;
    const float b = logf(r) + ll[(int64_t)c * stride + idx];
    float m = fmaxf(a, b);
    if (isinf(m)) m = 0.0f;
    G = m + logf(expf(a - m) + expf(b - m));
  }
  return G;
}

// Kernel-variant key only (not a descriptor value): the activation differs between the steps / nets of a component
// (`--coupling_network random` in the reference); the kernel reads it per step and net from the step header.
constexpr int GBNF_ACT_PER_STEP = 3;
// Steps whose tables the chained training sweeps keep in LDS: LDS_TABLE_STEPS of gbnf_flow_kernel.hip.h (gbnf_api.hip asserts the two
// are equal), for the translation units that do not see the kernels
constexpr int CHAIN_TABLE_STEPS = 24;
// Per-device state of the library (the saturation counters, the dynamic-LDS opt-ins) is indexed by hipGetDevice up to here
constexpr int MAX_DEVICES = 64;

// The opt-in of a launcher's kernels to 160 KB of dynamic LDS, once per DEVICE: hipFuncSetAttribute applies to the current device's
// function object, so a process that drives several GPUs needs it on each of them.  One `static DynamicLdsOptIn` per launcher (per
// template instantiation); call it with the launch's device current.  A failed attribute call is returned and not remembered as done.
struct DynamicLdsOptIn {
  bool done[MAX_DEVICES] = {};
  hipError_t operator()(std::initializer_list<const void*> kernels) {
    // (a process that sees one device has nothing to look up: hipGetDevice per launch measured +0.2 us on a 52 us evaluation step)
    static const int n_devices = [] { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }();
    int dev = 0;
    hipError_t e = n_devices == 1 ? hipSuccess : hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= MAX_DEVICES) return hipErrorInvalidDevice;
    if (done[dev]) return hipSuccess;
    for (const void* k : kernels) {
      e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e != hipSuccess) return e;
    }
    done[dev] = true;
    return hipSuccess;
  }
};

// ---- the buffers of the training path: the caller's trace buffer and backward workspace ------------------------------
constexpr int TR_MAX_NT = 2;            // 16-sample tiles per workgroup of the per-step kernels (they share every weight fragment a wave loads)
constexpr int TR_WS_SLACK_ROWS = 320;   // workspace rows behind the last operand region: a block of wgrad_kernel reads up to 256 rows
// The chained backward leaves its ActNorm / BatchNorm parameter sums per workgroup in those slack rows ([n_wg][K][2][64] floats, whose
// contents are of no consequence to wgrad_kernel): at least 4 waves of 16 samples per workgroup => n_wg <= np / 64, K * 128 floats each
static_assert(2 * CHAIN_TABLE_STEPS <= TR_WS_SLACK_ROWS, "the backward sweep's per-workgroup partial sums must fit the slack rows");

// Where everything lives, for a flow of K steps on d features with `nnets` coupling nets per step (padded widths ip / hp / op, `n_hidden`
// hidden layers per net) at a batch of n rows.  All rows are np floats long.
//   trace buffer:  K normalised states | the parked state | operand regions [K][nnets][net_rows] | slack rows (partial sums)
//                  (the last two only for a trainer with a live blob: its forward sweep fills them)
//   workspace:     operand regions | slack rows | the gradient state parked between step launches
//   one net's operand region: net input (ip) | hidden activations (n_hidden x hp) | hidden gradients (n_hidden x hp) |
//                  output gradient (op) | the net's output as the forward sweep saved it (op)
struct TrainLayout {
  int K = 0, d = 0, nnets = 1, ip = 0, hp = 0, op = 0, n_hidden = 0;
  int64_t n = 0, np = 0;
  TrainLayout() = default;
  TrainLayout(int K_, int d_, int nnets_, int ip_, int hp_, int op_, int n_hidden_, int64_t n_ = 0)
      : K(K_), d(d_), nnets(nnets_), ip(ip_), hp(hp_), op(op_), n_hidden(n_hidden_), n(n_), np(padded(n_)) {}
  TrainLayout at(int64_t rows) const { return TrainLayout(K, d, nnets, ip, hp, op, n_hidden, rows); }
  // whole workgroups for every tile count of every kernel (32 rows)
  static int64_t padded(int64_t rows) { return (rows + 16 * TR_MAX_NT - 1) / (16 * TR_MAX_NT) * (16 * TR_MAX_NT); }

  // rows inside one net's operand region
  int64_t input_row() const { return 0; }
  int64_t hidden_row(int j) const { return (int64_t)ip + (int64_t)j * hp; }                       // activation of hidden layer j
  int64_t hidden_grad_row(int j) const { return (int64_t)ip + (int64_t)(n_hidden + j) * hp; }     // its gradient
  int64_t out_grad_row() const { return (int64_t)ip + 2LL * n_hidden * hp; }
  int64_t net_rows() const { return out_grad_row() + 2LL * op; }
  int64_t net_base_row(int step, int net) const { return ((int64_t)step * nnets + net) * net_rows(); }
  int64_t operand_rows() const { return (int64_t)K * nnets * net_rows(); }
  // the sweeps address one step's operand regions with 32-bit offsets
  bool fits_32bit() const { return (int64_t)nnets * net_rows() * np < (1LL << 31); }

  // float offsets inside the trace buffer
  int64_t state_floats() const { return (int64_t)d * np; }
  int64_t parked_off() const { return (int64_t)K * state_floats(); }           // the running state between step-range launches
  int64_t acts_off() const { return ((int64_t)K + 1) * state_floats(); }
  int64_t partials_off() const { return acts_off() + operand_rows() * np; }
  int64_t trace_floats(bool live) const { return acts_off() + (live ? (operand_rows() + TR_WS_SLACK_ROWS) * np : 0); }
  // float offset of the gradient state inside the backward workspace / its size
  int64_t gstate_off() const { return (operand_rows() + TR_WS_SLACK_ROWS) * np; }
  int64_t workspace_bytes() const { return (gstate_off() + state_floats()) * 4; }
};

// ---- the training path's forward sweep on the evaluation kernels (gbnf_api.hip; used by gbnf_train.hip) -------------
// A "live blob": the packed hx3 (f16x3) parameter blob of ONE component whose parameters live in device tensors that an
// optimiser updates in place.  The blob's layout is walked in ONE place (gbnf_api.hip: plan_net_hx3, step_order,
// for_table_entries, tile_elem), which yields records of where every value-dependent word comes from; the host packer of
// gbnf_flow_create evaluates them on host arrays, `live_blob_create` runs the same pack_component in its structure-only
// mode (slot maps, activation flags, identity constants written once; the records uploaded) and
// `live_blob_forward` re-derives those words on the device (one gather + split kernel, ~10 us) and launches the TRAIN
// instantiation of flow_kernel_hx3: x -> z, ldj + the trace and operand saves the backward pass needs.
struct LiveBlob;
// desc: a component descriptor whose parameter pointers are DEVICE pointers (perm_indices: host).  GBNF_ERR_UNSUPPORTED
// (and *out = nullptr) when no TRAIN kernel variant covers the geometry: the caller keeps its own forward kernel.
// norm_grad_offsets: [K][2] float offsets of every step's two normalisation-parameter gradients in the caller's flat gradient
// buffer (null: no backward sweep wanted)
// prec: 0 = f16x3 (the sweeps saturate at the fp16 range and count it), 1 = bf16x6 (f32 range: the blob of a range-safe trainer;
// only geometries with a `safe` line in variants.list have these sweeps)
int live_blob_create(const gbnf_flow_desc* desc, const int64_t* norm_grad_offsets, LiveBlob** out, int prec = 0);
// Hidden rows (16 x hidden tiles) of the TRAIN variant a trainer of this flow would run, 0 if none
int live_blob_train_rows(const gbnf_flow_desc* desc, int prec = 0);
bool live_blob_has_backward(const LiveBlob* lb);
int live_blob_hidden_rows(const LiveBlob* lb);      // 16 x the hidden tiles of the kernel variant behind it
// The backward kernel leaves the ActNorm / BatchNorm parameter gradients as per-workgroup partial sums; adding them up (in a
// fixed order) is a reduction of n_wg rows per (step, parameter array).  With `reduce_out` the caller takes that over (the
// trainer folds it into wgrad_kernel's launch as extra blocks: one launch less per step); with null it is launched here.
struct LiveReduce {
  const float* partials;      // [n_wg][K][2][64]
  int n_wg, K, d;
  const int64_t* goff;        // [K][2] float offsets into the flat gradient buffer
  unsigned skip_steps;        // bit k: step k's two sums are NOT added (they were, by an earlier launch: batch-statistics BatchNorm)
};
// One step RANGE of a training sweep (BatchNorm on batch statistics; FlowLaunch::k_begin ..).  Forward: state_in / state_out =
// the state parked in slot layout [d][np] (null: x rows / the flow's z, ldj outputs); bmean / bvar: device (d,) batch statistics
// of step k_begin's BatchNorm, or null (running statistics: what the re-pack derived); repack: re-derive the blob from the live
// parameters first (the first range of a sweep).  Backward: state_in / state_out = the scaled gradient state behind step
// k_end - 1 / in front of step k_begin (null: g_z rows / g_x rows).
struct LiveRange {
  int k_begin, k_end;
  const float* state_in;
  float* state_out;
  int ldj_accumulate;
  bool repack;
  const float* bmean;
  const float* bvar;
};
// trace: the buffer the forward sweep filled (layout: TrainLayout at this batch); the states are read, the gradient-side operands of
// the weight gradients written behind them
int live_blob_backward(LiveBlob* lb, const TrainLayout& lay, float* trace, const float* g_z, const float* g_ldj, float* g_x,
                       float* grads, const unsigned* gmax, void* stream, LiveReduce* reduce_out = nullptr,
                       const LiveRange* range = nullptr);
void live_blob_destroy(LiveBlob* lb);
// The two halves of a repairing trainer (gbnf_trainer_create_mode, GBNF_MATH_DEFAULT).  sat: the f16x3 blob's launches count the waves
// that met the fp16 range in this word (64-bit, trainer-owned) instead of the device's training counter.  gate: the bf16x6 blob's
// launches (re-pack, both sweeps) return at once while this device word is 0 -- the re-run of a call that did not meet the range.
void live_blob_set_repair(LiveBlob* lb, unsigned* sat, const unsigned* gate);
// trace: [K][d][np] normalised states (slot layout), the parked state and the operand workspace (FlowLaunch::acts_out) of `lay`
int live_blob_forward(LiveBlob* lb, const TrainLayout& lay, const float* x, float* z, float* ldj, float* trace, void* stream,
                      const LiveRange* range = nullptr);
// (tests) the blob as the device packer left it / size in words
int live_blob_words(const LiveBlob* lb, uint32_t* out_host, int64_t* n_words);

// ---- the data-gradient-only backward of a tabular trainer (gbnf_train.hip; used by gbnf_score.hip) -------------------
// What gbnf_score.hip needs of a trainer to lay out a call
struct TrainerScoreView {
  int d;
  int64_t grad_floats;
  int batch_stats;        // gbnf_trainer_set_batch_stats is on
  int repairing;          // GBNF_MATH_DEFAULT: two forms of every call
};
int trainer_score_view(const gbnf_trainer* t, TrainerScoreView* out);
// Bytes of backward workspace trainer_backward_x needs at n rows: gbnf_trainer_workspace_bytes without the deterministic mode's
// weight-gradient partials (no launch of the data-gradient-only form touches them)
int64_t trainer_backward_x_base_bytes(const gbnf_trainer* t, int64_t n);
// gbnf_trainer_backward cut down to dL/dx: the same sweeps on the same launch parameters STORE g_x (n, d); no weight-gradient launch,
// no partial-sum reduce, no gradient memset or commit.  The per-step kernels add their ActNorm / BatchNorm sums into `discard`
// (grad_floats floats, contents of no consequence); a repairing trainer leaves the g_x of its two forms in `xpair` (2 n d floats,
// unused otherwise) and selects between them on the device.  The caller has checked t, x, g_x, workspace, n > 0 and refused
// batch-statistics mode; the deterministic-mode and workspace-size refusals happen here, before any launch.
int trainer_backward_x(const gbnf_trainer* t, const float* x, int64_t n, const float* trace, const float* g_z, const float* g_ldj, float* g_x,
                       void* workspace, int64_t workspace_bytes, float* discard, float* xpair, hipStream_t s);
// ll[i] = sum_j log N(z_ij; 0, 1) + ldj[i]  (n,): score_seed_kernel with only ll wanted -- the per-row double sum in feature order,
// rounded once, the constant that of gbnf_mixture_component_log_prob.  One launch, n >= 1.  gbnf_score.hip; used by gbnf_mixstep.hip
void score_launch_ll(const float* z, const float* ldj, int64_t n, int d, float* ll, hipStream_t s);

}  // namespace gbnf
