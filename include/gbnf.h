/*
 * gbnf.h -- C ABI of libgbnf_hip.so: the MI355X (gfx950) boosted normalizing-flow
 * density evaluator.
 *
 * The reference project has NO native / FFI layer: its boundary for this path is the
 * Python call  BoostedFlow.forward(x=, components=c)  ->  self.flows[c](x)
 * (models/boosted_flow.py:220-228) and the mixture arithmetic its callers write inline
 * (density_experiment.py:561-573).  Each entry point below states which reference
 * code it replaces.  INTEGRATION.md shows the ctypes binding a reference maintainer
 * would add.
 *
 * Conventions
 *  - plain C, no torch types.  `x`, `z`, `ldj`, `ll`, `rho_dev`, `out` are DEVICE pointers
 *    to contiguous float32 owned by the caller (PyTorch tensors' data_ptr()); descriptor
 *    pointers (`gbnf_*_desc`, `gbnf_linear.weight`, ...) are HOST pointers that only need
 *    to stay valid for the duration of the create call (the handle owns packed copies).
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Kernels are
 *    enqueued on it; no call synchronises the device except create/destroy/set_base.
 *  - every function returns GBNF_OK (0) or a negative gbnf_status; it never throws and
 *    never exits.  gbnf_last_error() gives the message for the calling thread.
 *  - handles are immutable after creation: concurrent forward calls on different streams
 *    are safe; create/destroy must not race with in-flight work on the same handle.
 */
#ifndef GBNF_H_
#define GBNF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GBNF_ABI_VERSION 4

typedef enum gbnf_status {
  GBNF_OK = 0,
  GBNF_ERR_INVALID = -1,      /* bad argument / inconsistent descriptor            */
  GBNF_ERR_UNSUPPORTED = -2,  /* shape or option with no compiled kernel variant    */
  GBNF_ERR_HIP = -3,          /* a HIP runtime call failed                          */
  GBNF_ERR_NO_DEVICE = -4     /* no gfx950 device visible                           */
} gbnf_status;

enum { GBNF_KIND_GLOW = 0, GBNF_KIND_REALNVP = 1 };
/* TANH / RELU: TanhNet / ReLUNet (models/layers.py:208-243), n_layers = coupling_network_depth + 2 Linear layers.
 * RESIDUAL_RELU: ResidualNet (models/layers.py:246-301) of B = coupling_network_depth blocks, n_layers = 2 + 2 B Linear
 * layers in the order initial_layer, (blocks[b].linear_layers[0], blocks[b].linear_layers[1]) for b < B, final_layer:
 *     t = initial(x);  t += lin1_b(relu(lin0_b(relu(t)))) for every block;  out = final(t)
 * One block (the reference's default depth): the split kernels, every hidden width, both directions and training; two blocks: the
 * split kernels and the register-chained training kernels to hidden width 256 (round 5), the exact-f32 kernel and the per-step
 * training kernels beyond (B <= 2). */
enum { GBNF_ACT_TANH = 0, GBNF_ACT_RELU = 1, GBNF_ACT_RESIDUAL_RELU = 2 };
enum { GBNF_COUPLING_AFFINE = 0, GBNF_COUPLING_ADDITIVE = 1 };
/* How the coupling-network matrix products are evaluated:
 *   F32     exact f32 MFMA (v_mfma_f32_16x16x4_f32), bitwise an ordered fmaf chain (depth 0 / 1 / 2, ResidualNets of <= 2 blocks; hidden <= 512);
 *   F16X3   each f32 operand split into two fp16 pieces (22 significand bits); a.b = a_mid.b_hi + a_hi.b_mid +
 *           a_hi.b_hi on the f16 matrix pipe with f32 accumulation (TanhNet / ReLUNet, coupling_network_depth 0 / 1 / 2, hidden <= 512;
 *           ResidualNets of one block -- the reference's default depth -- at every width and of two blocks to 256, round 5): the fast
 *           path, ~1e-7 relative in the log-likelihood on well-conditioned models.  An operand beyond the fp16 range
 *           (|v| > 65504) cannot be represented: the kernel marks such samples and a bf16x6 repair pass behind every
 *           f16x3 launch re-evaluates them (same stream, no host synchronisation), so results are range-safe;
 *   BF16X6  three bf16 pieces per operand (>= 24 bits, f32 range), six products: f32-faithful for every finite input;
 *           ~2x the matrix work of F16X3 (same shapes as F16X3);
 *   DEFAULT per component: both split packings are built and a probe batch (128 rows ~ N(0,1) / N(0,4)) is evaluated
 *           on both at creation; F16X3 if they agree to 2.5e-6 relative in the log-likelihood, else BF16X6 (ill-conditioned
 *           models: e.g. un-normalised ReLU RealNVPs); F32 where no split kernel applies (two-block ResidualNets wider than 256).
 *           Env GBNF_MATH=f32|f16x3|bf16x6 overrides DEFAULT in gbnf_flow_create. */
enum { GBNF_MATH_DEFAULT = -1, GBNF_MATH_F32 = 0, GBNF_MATH_F16X3 = 1, GBNF_MATH_BF16X6 = 2 };

/* nn.Linear: y = x W^T + b, W row-major (out_features, in_features).
 * TanhNet / ReLUNet layers, models/layers.py:208-243. */
typedef struct gbnf_linear {
  const float* weight;
  const float* bias;
  int32_t out_features;
  int32_t in_features;
} gbnf_linear;

/* Coupling network: Linear -> [act, Linear] x depth -> act, Linear  (n_layers = depth + 2). */
typedef struct gbnf_net {
  int32_t activation; /* GBNF_ACT_* */
  int32_t n_layers;
  const gbnf_linear* layers;
} gbnf_net;

/* One tabular Glow FlowStep: ActNorm1d -> Permute1d -> coupling.  models/glow.py:317-342. */
typedef struct gbnf_glow_step {
  const float* actnorm_bias;   /* (d,)  _ActNorm.bias,  models/layers.py:467 */
  const float* actnorm_logs;   /* (d,)  _ActNorm.logs,  models/layers.py:468 */
  const int64_t* perm_indices; /* (d,)  PermuteNd.indices (NOT in state_dict), models/layers.py:636-651 */
  gbnf_net block;              /* in d/2 -> out 2*(d-d/2) (affine) or d-d/2 (additive) */
} gbnf_glow_step;

/* One RealNVP step: [BatchNorm eval] -> split/swap -> t,s nets -> affine.
 * models/transformations.py:560-579, models/layers.py:337-358. */
typedef struct gbnf_realnvp_step {
  int32_t flipped;             /* (k + flip_init) % 2, models/realnvp.py:38,118 */
  int32_t has_batch_norm;
  const float* bn_log_gamma;   /* (d,) each; ignored when !has_batch_norm */
  const float* bn_beta;
  const float* bn_running_mean;
  const float* bn_running_var;
  float bn_eps;
  gbnf_net t_net;              /* shift net */
  gbnf_net s_net;              /* log-scale net */
} gbnf_realnvp_step;

/* One boosted component = BoostedFlow.flows[c]  (models/boosted_flow.py:42-50). */
typedef struct gbnf_flow_desc {
  int32_t kind;      /* GBNF_KIND_* */
  int32_t d;         /* features (z_size) */
  int32_t n_steps;   /* K = num_flows */
  int32_t coupling;  /* GBNF_COUPLING_* (glow only) */
  const gbnf_glow_step* glow_steps;       /* n_steps entries when kind == GLOW */
  const gbnf_realnvp_step* realnvp_steps; /* n_steps entries when kind == REALNVP */
} gbnf_flow_desc;

typedef struct gbnf_flow gbnf_flow;       /* one component, packed on the device */
typedef struct gbnf_mixture gbnf_mixture; /* C same-architecture components      */

/* What a handle's kernel variant looks like (for roofline accounting in bench.py). */
typedef struct gbnf_kernel_info {
  int32_t hidden_tiles;        /* 16-unit MFMA tiles per hidden layer            */
  int32_t out_tiles;
  int32_t samples_per_wave;    /* 16 or 32                                        */
  int32_t n_steps;
  double macs_per_sample;        /* algorithmic multiply-adds per sample per component */
  double padded_macs_per_sample; /* what the MFMA tiles actually execute          */
  int64_t packed_bytes;          /* device bytes of packed parameters per component */
  int32_t math_mode;             /* GBNF_MATH_F32, _F16X3 or _BF16X6 actually used */
  float probe_rel_err;           /* DEFAULT mode: f16x3 vs bf16x6 on the creation-time probe batch (max relative
                                    log-likelihood difference; inf = a probe row left the fp16 range); -1 = no probe ran */
} gbnf_kernel_info;

int gbnf_version(void);
const char* gbnf_last_error(void);

/* The split-f16 kernels (evaluation, training) represent an f32 operand by two fp16 pieces: beyond +-65504 it cannot be
 * stored (the normalised input of a coupling net, a ReLU activation; in training also scaled gradients).  The EVALUATION
 * kernels repair such samples themselves (bf16x6 pass, see GBNF_MATH_F16X3).  What TRAINING does depends on the trainer's
 * math mode (gbnf_trainer_create_mode):
 *   GBNF_MATH_F16X3   the kernels saturate: the operand is clamped to +-65504, the step stays finite, the gradients of the
 *                     affected samples are wrong, and the wave is counted here (so is a WEIGHT beyond the range met by the
 *                     trainer's re-pack: it cannot be split at all).  What gbnf_trainer_create builds.
 *   GBNF_MATH_BF16X6  range-safe: every sweep, the re-pack and the weight gradients run on three bf16 pieces with the range
 *                     of f32; nothing is clamped and nothing is counted.
 *   GBNF_MATH_DEFAULT repairing: f16x3 first; a forward or backward call whose f16x3 launches met the range is re-run in bf16x6 within
 *                     the same call (decided on the device, no host read).  Such a step counts in gbnf_saturation_count like an
 *                     evaluation repair and in gbnf_trainer_repair_count, NOT in gbnf_training_saturation_count: its gradients are right.
 * This returns how many waves ran into the range since the last reset -- 0 for z-scored data on a trained flow -- and
 * optionally resets the counter.  One counter per device: this reports (and resets) the CURRENT device's, after a
 * hipDeviceSynchronize() (every stream of that device). */
int gbnf_saturation_count(int64_t* count, int32_t reset);
/* The part of that count that came from TRAINING launches of GBNF_MATH_F16X3 trainers (gbnf_trainer_forward / _backward: traced and
 * untraced sweeps, the weight re-pack): these saturate and are NOT repaired, so a non-zero value means steps with wrong gradients
 * (a GBNF_MATH_BF16X6 trainer never moves it) -- while the rest of
 * gbnf_saturation_count() (evaluation launches) was re-evaluated in the same call.  Same device, same synchronisation; `reset` clears
 * this part only.  (The drop-in module reads it when it leaves training mode: BoostedFlow.train / .eval.) */
int gbnf_training_saturation_count(int64_t* count, int32_t reset);

/* Numerics guard of a GBNF_MATH_DEFAULT handle that runs on f16x3 (round 3; what the creation-time probe cannot know is
 * the caller's data).  The library itself re-checks the choice on the data it is given: on the FIRST launch of a handle
 * and then on every `check_every`-th (tuning key below, default 256) it evaluates up to 256 rows of the launch's first
 * batch on f16x3 and on bf16x6 and compares the log-likelihoods ON THE DEVICE, in stream order behind the launch; if they
 * differ by more than `tolerance` (2.5e-6 relative, a quarter of the 1e-5 parity bar) the handle's guard word is set and
 *   - the bf16x6 pass that follows every f16x3 launch (the repair pass for out-of-range samples) re-evaluates the WHOLE
 *     work list from then on, starting with the launch that failed the check: no result of a failed mode reaches the caller;
 *   - the host sees the flag (pinned memory, no synchronisation) on a later call and launches bf16x6 directly.
 * Every entry point that evaluates a flow (gbnf_flow_forward, gbnf_mixture_component_log_prob*, gbnf_mixture_log_prob)
 * is covered, so C-ABI callers, sharded.GroupPipeline and bench.py get it like BoostedFlow does.  Handles created with
 * an explicit GBNF_MATH_F16X3 keep the caller's choice (range repair only).  These calls never synchronise: `checks`
 * and `worst_rel_err` are those of the checks that have COMPLETED on the device.
 * The z -> x direction (gbnf_flow_inverse) is checked the same way on a schedule of its OWN: the first inverse launch of a handle
 * and every `check_every`-th after it evaluate up to 256 leading rows of the launch's z on both packings and compare x and
 * log|det| on the device, per row  e_x = max_j |x16 - x6| / max(1, max_j |x6|)  and  e_l = |l16 - l6| / max(1, |l6|).  The check
 * fails when e_l > tolerance or e_x > 2 tolerance: a quarter of the direction's parity bars (1e-5 for log|det|, 2e-5 for x), as
 * the forward tolerance is a quarter of the log-likelihood's.  The verdict belongs to the handle: a failed check of either
 * direction re-evaluates ALL rows of the failing call on bf16x6 (x and log|det|) and sends both directions to bf16x6.
 * gbnf_flow_numerics reports the forward checks, gbnf_flow_numerics_inverse the z -> x ones: `math_mode` and `demoted` are shared,
 * `checks` and `worst_rel_err` (= max(e_l, e_x / 2), so that it compares with `tolerance`, the log|det| one) are that direction's.
 * A call that writes x over its own z buffer is not checked (and does not advance the schedule). */
typedef struct gbnf_numerics_status {
  int32_t math_mode;       /* GBNF_MATH_* the NEXT launch of this handle will run in                       */
  int32_t demoted;         /* 1 = a check failed: the handle left f16x3 for bf16x6                          */
  int64_t checks;          /* device-side checks completed so far                                           */
  float worst_rel_err;     /* largest relative log-likelihood difference f16x3 vs bf16x6 seen by a check    */
  float tolerance;
} gbnf_numerics_status;
int gbnf_flow_numerics(const gbnf_flow* flow, gbnf_numerics_status* out);
int gbnf_flow_numerics_inverse(const gbnf_flow* flow, gbnf_numerics_status* out);
int gbnf_mixture_numerics(const gbnf_mixture* mix, gbnf_numerics_status* out);

/* Launch-policy knobs (process-wide; tests, soak runs and tuning -- the defaults are what is measured and shipped):
 *   "force_nt"      0 = automatic | 1 | 2 : samples per wave = 16 x NT            (env GBNF_FORCE_NT at first use)
 *   "wg_pairs"      -1 = automatic (two 4-wave workgroups per CU whenever they fit -- small batches too, round 5 --, except LONG launches of
 *                   geometries with heavy weight stages, which run as one 8-wave workgroup per CU: +1.2 % on the headline, round 6) |
 *                   0 = never (always 8-wave workgroups) | 1 = pairs whenever they fit                (env GBNF_NO_WG_PAIRS=1 -> 0)
 *   "coop"          the LATENCY form of the f16x3 flow kernel (csrc/gbnf_flow_kernel_coop.hip.h, round 6: the waves of a workgroup share
 *                   ONE sample tile; one log_prob call at the reference's 512 / 1024-row batches 48 -> 29 / 37 us): -1 = automatic (taken
 *                   while every workgroup gets a CU to itself) | 0 = never | 1 / 2 / 3 = always form 1 / 2 / 3 (16-sample tiles on 4 waves,
 *                   32 on 4, 32 on 8) where the geometry has it.  Forward direction, depth-1 TanhNet / ReLUNet geometries listed as
 *                   `coop` lines in csrc/variants.list.  Results of the forms agree to 2e-6 (another summation order of the output layer):
 *                   a lone batch and the same batch inside a longer launch may differ in the last bits.
 *   "coop_max_wgs"  the latency form is taken while the call's sample tiles x components fill at most this many workgroups (default 256)
 *   "repair"        1 | 0 : the bf16x6 pass behind f16x3 launches                 (env GBNF_NO_REPAIR=1 -> 0)
 *   "nt2_min_waves" 32-sample waves from this many waves on (default 1024)        (env GBNF_NT2_MIN_WAVES)
 *   "check_every"   numerics guard: a check on launch 0 and every this many launches (default 256; 0 = first launch only;
 *                   -1 = never)
 *   "check_tolerance_e9"  numerics guard: tolerance of a check in units of 1e-9 relative (default 2500 = 2.5e-6; 0 makes
 *                   every check fail: how the tests exercise the demotion path)
 * Returns GBNF_ERR_INVALID for an unknown key. */
int gbnf_tuning_set(const char* key, int32_t value);
int gbnf_tuning_get(const char* key, int32_t* value);

/* Replaces: constructing flows[c] + .to(device)  (models/boosted_flow.py:42-50).
 * Packs (pads, tiles, folds slot maps) and uploads the parameters.
 * LIMITS (enforced: GBNF_ERR_UNSUPPORTED with the reason in gbnf_last_error; nothing falls back to a non-HIP path):
 *   features                1 <= d <= 64                 (a sample tile's features are LDS slots of one wave; the reference's five
 *                                                         tabular datasets have d = 6, 8, 21, 43, 63)
 *   coupling-net input      <= 32 features               (d / 2, or d - d / 2 for a flipped RealNVP step: one k = 32 MFMA chunk)
 *   hidden width            1 <= h <= 512                (TanhNet / ReLUNet at coupling_network_depth 0, 1, 2 and ResidualNets of one or two
 *                                                         blocks: all on the split kernels at every width -- two-block ResidualNets above
 *                                                         256 since round 6, evaluation; their TRAINING keeps the per-step kernels)
 *   coupling_network_depth  0, 1, 2; ResidualNet blocks 1, 2 (RealNVP only, as in the reference)
 *   flow steps              any K (per-step tables are staged in LDS up to K = 24 where they fit, read from the blob beyond; the chained
 *                                                         training sweeps take K <= 24)
 *   activations             tanh / relu, also drawn per step or per net (`--coupling_network random`) */
int gbnf_flow_create(const gbnf_flow_desc* desc, gbnf_flow** out);
/* Same with an explicit GBNF_MATH_* mode (gbnf_flow_create uses GBNF_MATH_DEFAULT, or env GBNF_MATH=f32|f16x3|bf16x6). */
int gbnf_flow_create_mode(const gbnf_flow_desc* desc, int32_t math_mode, gbnf_flow** out);
/* ... and creation flags.  A component whose coupling nets do not all use the same activation (the reference's
 * `--coupling_network random` draws TanhNet / ReLUNet per step, models/glow.py:295-296, or per net,
 * models/realnvp.py:59-60) runs on kernel variants that read the activation per step from the packed blob; that choice
 * is automatic.  GBNF_CREATE_PER_STEP_ACTIVATION asks for those variants although this component is uniform, so that it
 * can share a mixture (one launch, gbnf_mixture_create wants one kernel for all components) with components that are not. */
enum { GBNF_CREATE_PER_STEP_ACTIVATION = 1 };
int gbnf_flow_create_ex(const gbnf_flow_desc* desc, int32_t math_mode, int32_t flags, gbnf_flow** out);
int gbnf_flow_destroy(gbnf_flow* flow);
int gbnf_flow_info(const gbnf_flow* flow, gbnf_kernel_info* info);

/* Replaces: z, _, _, ldj, _ = self.flows[c](x)   (models/boosted_flow.py:220-222 ->
 * Glow.encode models/glow.py:92-110 / RealNVPFlow.encode models/realnvp.py:115-127).
 * x (n,d) -> z (n,d), ldj (n,), ll (n,) = log N(z;0,I) + ldj  (utils/distributions.py:44-60,
 * density_experiment.py:565).  Any of z / ldj / ll may be NULL to skip that output. */
int gbnf_flow_forward(const gbnf_flow* flow, const float* x, int64_t n,
                      float* z, float* ldj, float* ll, void* stream);

/* The flow backwards, z (n,d) -> x (n,d) and log|det dx/dz| (n,) (= -ldj of the forward pass at x): what
 * BoostedFlow.decode / Glow.decode / FlowStep.decode (models/boosted_flow.py:209-218, models/glow.py:112-123, 344-366)
 * and RealNVPFlow.decode (models/realnvp.py:97-113) are meant to do.  In the reference this direction is dead or wrong
 * on tabular data, so parity is defined by inverse(forward(x)) == x (and the one case the reference can
 * decode, additive Glow, fixture g9).  Any math mode (the split kernels run backwards since round 3; ResidualNets: f32).
 * An f16x3 launch is followed by its bf16x6 range-repair pass like a forward one, and a GBNF_MATH_DEFAULT handle re-checks the
 * f16x3 choice on the caller's z on this direction's own schedule (gbnf_numerics_status, gbnf_flow_numerics_inverse): a call whose
 * check fails returns the bf16x6 x and log|det| for every row. */
int gbnf_flow_inverse(const gbnf_flow* flow, const float* z, int64_t n, float* x, float* ldj, void* stream);

/* Replaces: the nn.ModuleList of components (models/boosted_flow.py:42).  All flows must
 * share one architecture (they do: every component is built from the same args) and one math mode -- except that
 * DEFAULT-created components which came out of their probes as a mix of F16X3 and BF16X6 are accepted: the mixture
 * then runs every component on its bf16x6 packing.
 * The mixture does NOT take ownership of the flows; they must outlive it. */
int gbnf_mixture_create(gbnf_flow* const* flows, int32_t n_flows, gbnf_mixture** out);
int gbnf_mixture_destroy(gbnf_mixture* mix);

/* Optional base density N(mean_j, std_j) per feature instead of N(0,1): the toy driver's
 * model.base_dist (models/generative_flow.py:22-23,38-42; toy_experiment.py:424).
 * HOST pointers (d,), or NULL/NULL to restore the standard normal. */
int gbnf_mixture_set_base(gbnf_mixture* mix, const float* mean, const float* std);

/* Replaces: the loop  for c in range(...): model(x=x, components=c); log_normal_standard(z)+ldj
 * (density_experiment.py:562-565) for components [c_begin, c_end) in ONE launch.
 * ll is (c_end - c_begin, n) row-major. */
int gbnf_mixture_component_log_prob(const gbnf_mixture* mix, const float* x, int64_t n,
                                    int32_t c_begin, int32_t c_end, float* ll, void* stream);
/* Same, writing row c of ll at ll + (c - c_begin) * ll_row_stride (>= n): lets several batches share one
 * (components, batches*n) table so that ONE all-gather / ONE recursion launch serves a group of batches. */
int gbnf_mixture_component_log_prob_strided(const gbnf_mixture* mix, const float* x, int64_t n,
                                            int32_t c_begin, int32_t c_end, float* ll, int64_t ll_row_stride,
                                            void* stream);
/* Same for a GROUP of up to 32 independent batches in ONE launch: xs is a HOST array of n_batches DEVICE pointers to
 * (n,d) inputs; batch b's log-densities go to columns [b*n, (b+1)*n) of the (c_end-c_begin, >= n_batches*n) table.
 * (A rank that holds few components does not fill the GPU with one batch; serving several batches per launch does,
 * and one all-gather + one recursion launch then cover the whole group.) */
int gbnf_mixture_component_log_prob_multi(const gbnf_mixture* mix, const float* const* xs, int32_t n_batches,
                                          int64_t n, int32_t c_begin, int32_t c_end, float* ll,
                                          int64_t ll_row_stride, void* stream);

/* Replaces: the calls  z, _, _, ldj, _ = model(x=x, components=c)  of the reference's evaluate loop
 * (density_experiment.py:562-563; models/boosted_flow.py:220-228) for ALL components [c_begin, c_end) of one batch in ONE
 * launch: z is (c_end - c_begin, n, d), ldj and ll are (c_end - c_begin, n) row-major; any of the three may be NULL (not all).
 * The host mirror answers the loop's per-component calls from this table (BoostedFlow.encode in eval mode). */
int gbnf_mixture_component_forward(const gbnf_mixture* mix, const float* x, int64_t n, int32_t c_begin, int32_t c_end,
                                   float* z, float* ldj, float* ll, void* stream);

/* Replaces: the recursive prefix-normalised 2-way logsumexp (density_experiment.py:567-571):
 *   G_0 = ll_0;  r_c = rho_c / sum(rho[0..c]);  G_c = LSE(log(1-r_c)+G_{c-1}, log(r_c)+ll_c).
 * ll is (n_components, n) with row stride `ll_row_stride` floats; rho_dev is the DEVICE
 * `rho` buffer (models/boosted_flow.py:32-39), at least n_components long. */
int gbnf_mixture_lse(const float* ll, int64_t ll_row_stride, const float* rho_dev,
                     int32_t n_components, int64_t n, float* out, void* stream);

/* The measured path: component_log_prob for components [0, n_used) + mixture_lse.
 * ll_workspace is (n_used, n) floats of caller-owned device scratch (also an output). */
int gbnf_mixture_log_prob(const gbnf_mixture* mix, const float* x, int64_t n, int32_t n_used,
                          const float* rho_dev, float* ll_workspace, float* out, void* stream);

/* ---- the component-sharded group inside the library (multi-GPU, round 4) -------------------------------------------------
 * Replaces: the serial component loop + recursion of density_experiment.py:561-573 when the C components are sharded over W
 * GPUs (BASELINE.json north star: one component block per GPU, an RCCL all-gather of log p_c(x), then the mixture recursion).
 * RCCL is bound directly (librccl.so is loaded at first use: no torch.distributed on the data path):
 *   gbnf_comm_unique_id   rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the other ranks through the caller's
 *                         own rendezvous (the host mirror uses the torch.distributed store);
 *   gbnf_comm_create      every rank of the group, collectively (ncclCommInitRank); world = 1 is allowed.
 * gbnf_mixture_group_log_prob: ONE call = flow launch of this rank's components (the mixture holds exactly its block, in global
 * component order rank by rank) over n_batches batches -> ncclAllGather of its (C/W, n_batches n) table into ll_full
 * (C, n_batches n), component order -> recursion -> G (n_batches n), all on `stream`.  comm NULL: one rank, no exchange (ll_full
 * unused).  All buffers are caller-owned device memory.
 * gbnf_group_graph_*: the same sequence captured ONCE into a HIP graph (bound to these very buffers; an un-captured warm-up call
 * runs first) and replayed with one hipGraphLaunch per group.  A capture that the runtime or RCCL refuses is reported as an
 * error: the caller keeps gbnf_mixture_group_log_prob. */
typedef struct gbnf_comm gbnf_comm;
typedef struct gbnf_group_graph gbnf_group_graph;
int gbnf_comm_unique_id(uint8_t* id128);
int gbnf_comm_create(const uint8_t* id128, int32_t rank, int32_t world, gbnf_comm** out);
int gbnf_comm_destroy(gbnf_comm* comm);
int gbnf_comm_info(const gbnf_comm* comm, int32_t* rank, int32_t* world);
int gbnf_mixture_group_log_prob(const gbnf_mixture* mix, gbnf_comm* comm, const float* const* xs, int32_t n_batches, int64_t n,
                                int32_t n_components, const float* rho_dev, float* ll_local, float* ll_full, float* G,
                                void* stream);
int gbnf_group_graph_create(const gbnf_mixture* mix, gbnf_comm* comm, const float* const* xs, int32_t n_batches, int64_t n,
                            int32_t n_components, const float* rho_dev, float* ll_local, float* ll_full, float* G,
                            gbnf_group_graph** out);
int gbnf_group_graph_launch(gbnf_group_graph* graph, void* stream);
int gbnf_group_graph_destroy(gbnf_group_graph* graph);

/* Replaces: _ActNorm.initialize_parameters (models/layers.py:473-486), the data-dependent initialisation the
 * reference runs on the first training batches (density_experiment.py:346-356):
 *   bias = -mean_0(z);  logs = log(scale / (sqrt(mean_0((z + bias)^2)) + 1e-6)).
 * z is the (n,d) DEVICE input of the ActNorm layer (the output of the preceding flow steps); bias_out / logs_out
 * are (d,) DEVICE buffers.  The first call allocates a small internal workspace. */
int gbnf_actnorm_init(const float* z, int64_t n, int32_t d, float scale, float* bias_out, float* logs_out,
                      void* stream);

/* Replaces: the boosting sample weights of compute_kl_pq_loss (density_experiment.py:624-640), computed from the
 * mixture log-density G (n,) of the fixed components:
 *   w = softmax(-G) (utils/utilities.py:12-14);  w = w^beta;  if max(w) > 0.1: w = clamp(w, 0.01, 0.1);
 *   if sum(w) != 1: w /= sum(w).
 * G and w_out are DEVICE buffers of n floats.  (The multinomial resampling that follows: gbnf_resample_rows, on the caller's
 * uniforms.) */
int gbnf_boosting_weights(const float* G, int64_t n, float beta, float* w_out, void* stream);

/* Replaces: reweighted_idx = torch.multinomial(weights, N, replacement=True) of compute_kl_pq_loss (density_experiment.py:643) --
 * m draws with replacement from n rows in proportion to w, by inverse CDF on the CALLER's uniforms u (m values in [0,1): the RNG
 * stays outside the library like `eps` of gbnf_image_flow_inverse, so a draw is reproducible and testable):
 *   cdf_j = sum_{k <= j} max(w_k, 0)  (a non-finite w_k counts 0), summed in double precision in a fixed order -- no atomics,
 *   bit-identical from run to run --;  T = cdf_{n-1};  rows[i] = the smallest j with (double)u[i] * T < cdf_j.
 * A row of zero weight is never drawn, and every index written lies in [0, n) whatever u and w hold: out of contract (u[i] >= 1 or
 * NaN) a draw takes the last row of positive weight, and row i % n when no row has any (T == 0).  w (n), u (m): DEVICE floats; rows (m):
 * DEVICE int64, what gbnf_trainer_nll_step takes; workspace: gbnf_resample_workspace_bytes(n) of DEVICE memory (the n-entry double
 * cdf, 8 n rounded up to 256), 8-byte aligned.  Two launches: a one-workgroup scan, a binary search per draw.
 * GBNF_ERR_INVALID (nothing launched): a null pointer, n < 1, m < 1, a workspace that is too small. */
int gbnf_resample_workspace_bytes(int64_t n, int64_t* bytes);
int gbnf_resample_rows(const float* w, int64_t n, const float* u, int64_t m, int64_t* rows, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Training path: what loss.backward() / optimizer.step() of density_experiment.py:366-374 do
 * to ONE component -- the forward on the LIVE parameters and its backward pass.
 *
 * A trainer binds the DEVICE addresses of the caller's parameter tensors: the descriptor has the same shape as for
 * gbnf_flow_create, but every float pointer (weights, biases, ActNorm / BatchNorm arrays) is a DEVICE pointer to the
 * tensor in its reference layout (nn.Linear.weight (out,in) row-major, ...) and stays owned by the caller;
 * perm_indices stay HOST pointers.  Nothing is packed or copied, so parameters updated in place by an optimiser are
 * seen by the next call; re-create the trainer only when a tensor is re-allocated.  RealNVP BatchNorm is differentiated
 * in its running-statistics (eval) form, models/layers.py:347-358, unless gbnf_trainer_set_batch_stats(1).
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct gbnf_trainer gbnf_trainer;

/* The descriptor checks gbnf_flow_create applies (reads sizes and perm_indices, never the parameter arrays). */
int gbnf_flow_validate(const gbnf_flow_desc* desc);

int gbnf_trainer_create(const gbnf_flow_desc* desc_device_params, gbnf_trainer** out);
/* ... with an explicit GBNF_MATH_* mode.  GBNF_MATH_F16X3: what gbnf_trainer_create does (that function is this call).
 * GBNF_MATH_BF16X6: the RANGE-SAFE trainer -- every forward and backward call of it, with and without a trace buffer, on running
 * and on batch statistics, runs the bf16x6 forms of the register-chained sweeps (three pieces per operand, six products), the
 * bf16x6 re-pack of the live weights and the bf16 weight-gradient kernel: f32 range throughout, no clamp, and
 * gbnf_training_saturation_count does not move.  A call without a trace runs the traced pair on a trace buffer the trainer owns
 * (it grows on demand; gbnf_trainer_trace_floats says how much); the per-step kernels never run.  Covered geometries, K <= 24:
 *   Glow and RealNVP with TanhNet / ReLUNet coupling nets (any mix per step and net) of coupling_network_depth 0, 1, 2, h <= 256;
 *   RealNVP with one-block ResidualNets, h <= 256;  d <= 64 as everywhere.
 * Everything else -- 256 < h <= 512, two-block ResidualNets, K > 24, a flow whose backward tables do not fit a CU's LDS --
 * answers GBNF_ERR_UNSUPPORTED with the reason in gbnf_last_error(): nothing falls back to a saturating kernel.
 * GBNF_MATH_DEFAULT: the REPAIRING trainer, for the same geometries (anything else: GBNF_ERR_UNSUPPORTED with the reason, K > 24
 * included).  A call launches the f16x3 kernels as ever; their range events go to a counter of the trainer; one thread on the device
 * turns it into the call's decision word; the bf16x6 form of the same call follows in stream order, every launch gated on that word
 * (a launch with nothing to do returns at once; the forward sweep's grid is capped like an evaluation repair launch).  No host read, no
 * synchronisation.  False positives are possible (an extra re-run is still right), false negatives are not.
 *   forward   the re-run overwrites z, ldj, the trace and the operand workspace.
 *   backward  both forms accumulate into zeroed scratch of the trainer (grad_floats floats each; it grows at the first call of a
 *             size, which synchronises once); a commit kernel adds the one that counts into `grads` and selects g_x the same way.
 *             It is re-run when its own f16x3 launches met the range OR the forward call that wrote `trace` was re-run.  That
 *             fact is trainer state keyed to the trace POINTER of the last forward call (a trace the trainer does not know counts as
 *             re-run).  The f16x3 and bf16x6 forms may run variants of different widths, i.e. different operand layouts behind the
 *             trace, so a backward re-run first writes its own forward sweep into the trace buffer (gbnf_trainer_trace_floats and
 *             gbnf_trainer_workspace_bytes return the larger of the two forms' sizes).
 *   re-pack   a weight beyond the range met by the f16x3 re-pack counts as "met the range".
 * The backward sweep's and the weight gradients' re-run launches are gated but not capped: their workgroups return at once.
 * GBNF_MATH_F32: GBNF_ERR_UNSUPPORTED, there is no exact-f32 trainer.
 * Calls of ONE trainer are not safe to issue concurrently from two threads or streams: the untraced entries of a range-safe trainer
 * and the backward of a repairing one use buffers the trainer owns, which grow (hipFree + hipMalloc: a device synchronisation) when
 * a call needs more than any call before it. */
int gbnf_trainer_create_mode(const gbnf_flow_desc* desc_device_params, int32_t math_mode, gbnf_trainer** out);
int gbnf_trainer_destroy(gbnf_trainer* trainer);
/* Forward and backward calls of this trainer whose bf16x6 re-run actually ran (a GBNF_MATH_DEFAULT trainer); synchronises like
 * gbnf_saturation_count.  Always 0 for GBNF_MATH_F16X3 and GBNF_MATH_BF16X6 trainers. */
int gbnf_trainer_repair_count(const gbnf_trainer* trainer, int64_t* calls, int32_t reset);

/* z, ldj = flows[c](x) on the live parameters (same semantics and outputs as gbnf_flow_forward).  `trace` (optional,
 * gbnf_trainer_trace_floats(n) floats of DEVICE memory) receives every step's normalised state; handing it to
 * gbnf_trainer_backward saves that call the forward sweep and the re-splitting of the weights (valid only while the
 * parameters are unchanged and no other forward call of this trainer ran on changed parameters in between).
 * Since round 3 the trace buffer of a flow that runs on the register-chained kernels (TanhNet / ReLUNet coupling nets of
 * coupling_network_depth 0, 1, 2 and RealNVP ResidualNets of one or two blocks -- all but depth 1 since round 5 -- of a compiled width)
 * is also the OPERAND WORKSPACE of the step: behind the states the forward call stores the coupling nets' inputs, hidden
 * activations and outputs.  gbnf_trainer_trace_floats returns the whole buffer, in rows of np = n-rounded-up-to-32 floats:
 * (K + 1) * d rows of states (K normalised ones and the running state), and for such a flow K * nets * (ip + 2 L hp + 2 op)
 * operand rows, L = hidden layers per net, + 320 slack rows -- 20 KB per sample for MINIBOONE, K = 5, depth 1.
 * gbnf_trainer_backward WRITES the gradient-side operands of the weight gradients into the same buffer (its `trace`
 * argument is const for the states only).  One trace buffer therefore serves one forward + one backward call. */
int gbnf_trainer_trace_floats(const gbnf_trainer* trainer, int64_t n, int64_t* n_floats);
int gbnf_trainer_forward(const gbnf_trainer* trainer, const float* x, int64_t n, float* z, float* ldj, float* trace,
                         void* stream);

/* RealNVP BatchNorm in the reference's train() form (models/layers.py:338-346): normalise with the BATCH mean and the
 * unbiased batch variance of every step's input, differentiate through them.  bind: DEVICE (d,) buffers that receive a
 * step's batch mean / variance at every forward call (the reference keeps them as BatchNorm.batch_mean / batch_var; the
 * running-statistics update with momentum stays with the caller).  set(1) switches forward / backward to one launch per
 * step (the statistics need the whole batch); it requires the trace buffer in both calls and n >= 2. */
int gbnf_trainer_bind_batch_stats(gbnf_trainer* trainer, int32_t step, float* mean_dev, float* var_dev);
int gbnf_trainer_set_batch_stats(gbnf_trainer* trainer, int32_t on);

/* Size of the flat parameter-gradient buffer, in floats.  Layout, step by step in descriptor order:
 *   glow:    [actnorm bias (d)] [actnorm logs (d)]  then per Linear of the block:   [weight (out*in)] [bias (out)]
 *   realnvp: [bn log_gamma (d)] [bn beta (d)]  (left zero without batch norm)  then t_net's Linears, then s_net's. */
int gbnf_trainer_grad_floats(const gbnf_trainer* trainer, int64_t* n_floats);
/* Bytes of caller-owned DEVICE scratch one backward call over n samples needs (larger in deterministic mode, below: ask again
 * after switching it). */
int gbnf_trainer_workspace_bytes(const gbnf_trainer* trainer, int64_t n, int64_t* bytes);

/* Backward of (z, ldj) = flows[c](x): given g_z = dL/dz (n,d) and g_ldj = dL/dldj (n,) (either may be NULL = zero),
 * ACCUMULATES dL/dparameters into `grads` (the caller zeroes it; layout above) and writes dL/dx to g_x (n,d) unless
 * NULL.  `trace` is the forward call's trace buffer or NULL.  With it, a flow on the register-chained kernels (above)
 * recomputes nothing: the backward kernel chains W3^T -> W2^T -> W1^T on the saved activations, ActNorm / BatchNorm
 * gradients are summed per workgroup and added in a fixed order (bit-identical from run to run).  By default the weight
 * gradients are added with float atomics across sample blocks: their last bits depend on the order; deterministic mode
 * (below): every sample block stores its partial and the partials are added in block order.  Other flows recompute the
 * coupling nets' activations from the trace, and with NULL the whole forward sweep from x.
 * Batch-statistics mode (gbnf_trainer_set_batch_stats): the BatchNorm entries of `grads` (log_gamma, beta of every step) MUST
 * be zero on entry -- the correction for the statistics' dependence on every sample reads THIS call's two batch sums from
 * them; accumulate several calls by adding up separately zeroed buffers (what the Python mirror does: a fresh buffer per
 * call).  That mode needs n >= 2 (unbiased variance) and K <= 32. */
int gbnf_trainer_backward(const gbnf_trainer* trainer, const float* x, int64_t n, const float* trace, const float* g_z,
                          const float* g_ldj, float* g_x, float* grads, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* Deterministic mode, a property of the trainer like gbnf_trainer_set_batch_stats (off at creation; the default path,
 * its kernels and its results do not change).  While it is on, for a fixed trainer, fixed inputs, fixed parameter
 * values, a fixed n and fixed tuning keys, gbnf_trainer_backward, gbnf_trainer_nll_step and gbnf_boosted_nll_step write
 * bit-identical `grads`, g_x, parameters, exp_avg, exp_avg_sq, stats_dev and rows_out on every call, in every math mode
 * (a repairing trainer decides from the data, so its decision repeats too).  How: sample chunk y of a weight-gradient
 * block stores its dW tile and db rows to partials[y][..] in the backward workspace (plain stores, no atomics), and a
 * second launch adds the Y partials of every entry in chunk order into `grads`; Y is a function of the trainer's layer
 * shapes and of n only.  Everything else in those calls is ordered already.  Cost: Y x gbnf_trainer_grad_floats floats
 * of workspace -- gbnf_trainer_workspace_bytes, gbnf_trainer_step_workspace_bytes and gbnf_boosted_step_workspace_bytes
 * report the larger sizes while the mode is on, and a workspace sized before switching it on is refused with
 * GBNF_ERR_INVALID ("workspace too small"), never overrun. Limits: a call that would run the per-step kernels, whose
 * gradients are added with unordered float atomics -- a flow of more than 24 steps, a two-block ResidualNet wider than
 * 256, any geometry without a register-chained backward sweep, an f16x3 call without the forward call's trace --
 * returns GBNF_ERR_UNSUPPORTED with the reason and launches nothing.  (A GBNF_MATH_BF16X6 trainer has no per-step
 * kernels: a call it cannot serve is refused as ever, with its own reason, behind the launch that finds the scale of
 * the upstream gradient; it never gives an unordered result either.)  Nothing is promised across different n, tuning
 * keys, math modes or builds.  The image trainer has a mode of its own, gbnf_image_trainer_set_deterministic (below):
 * this call does not reach it. */
int gbnf_trainer_set_deterministic(gbnf_trainer* trainer, int32_t on);
int gbnf_trainer_get_deterministic(const gbnf_trainer* trainer, int32_t* on);

/* ---- the rest of the step: loss seed, gradient-norm clip and the optimiser, on the device -------------------------------
 * Between and behind the two calls above the reference's driver runs eager PyTorch: the NLL and its autograd seed, clip_grad_norm_,
 * optimizer.step() (density_experiment.py:340-374).  These calls do that on the trainer's stream, on the LIVE tensors the trainer
 * binds: the next gbnf_trainer_forward sees the updated parameters with no host work.  No call reads the device or synchronises.
 * The optimiser state is caller-owned like every buffer of this ABI: two flat DEVICE buffers of gbnf_trainer_grad_floats floats in the
 * layout of the gradient buffer (they map one to one onto torch.optim.AdamW's exp_avg / exp_avg_sq), and the update's index `step`.
 * It survives re-creating the trainer.  Replaces: optim.AdamW(lr, weight_decay) with default betas / eps or optim.SGD(lr,
 * weight_decay) without momentum (optimization/optimizers.py:54-65); a component that is not being trained gets lr = 0
 * (update_learning_rates, density_experiment.py:511-513): its parameters stay bit-identical while its moments move, as in torch. */
enum { GBNF_OPT_SGD = 0, GBNF_OPT_ADAMW = 1 };
typedef struct gbnf_opt_hyper {      /* 48 bytes; passed by pointer, read on the host at call time */
  int32_t kind;                      /* GBNF_OPT_*                                                   */
  int32_t reserved0;
  int64_t step;                      /* 1-based index of THIS update (AdamW bias correction)         */
  float lr, beta1, beta2, eps;       /* each taken as the shortest decimal that rounds to the float: 0.999f means 0.999, */
                                     /* so that 1 - beta2 is torch's (computed from the Python float) to the last bit    */
  float weight_decay;                /* AdamW: decoupled (p *= 1 - lr wd); SGD: g += wd p            */
  float max_grad_norm;               /* <= 0: no clipping                                            */
  float bn_momentum;                 /* < 0: running statistics untouched (see nll_step)             */
  float reserved1;
} gbnf_opt_hyper;
/* stats_dev: 4 floats of DEVICE memory: [0] nll (nll_step only; apply_update leaves it alone), [1] total gradient 2-norm,
 * [2] clip coefficient applied, [3] 0 */

/* Replaces: torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm) + optimizer.step() (density_experiment.py:363-364,
 * 374) for this component, from a flat gradient buffer in the gbnf_trainer_grad_floats layout (reserved RealNVP regions: zero, no
 * tensor behind them, skipped):
 *   norm = ||grads||_2 over all entries -> stats[1];  coef = min(1, max_grad_norm / (norm + 1e-6)) (1 without clipping) -> stats[2];
 *   g = coef * grads[i], then in torch's order
 *     AdamW  p *= 1 - lr wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
 *            p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)      (bias corrections: host, double precision)
 *     SGD    p -= lr (g + wd p)                                                      (exp_avg / exp_avg_sq may be NULL)
 * `grads` is read only: it holds the unclipped gradient afterwards.  The norm is summed per workgroup and re-added in a fixed order in
 * double precision: bit-identical from run to run for the same buffer.  GBNF_ERR_INVALID (nothing launched): unknown kind, AdamW with
 * step <= 0 or without state.  Two calls on ONE trainer must not run concurrently (the partial sums live in the trainer). */
int gbnf_trainer_apply_update(const gbnf_trainer* trainer, const float* grads, float* exp_avg, float* exp_avg_sq,
                              const gbnf_opt_hyper* hyper, float* stats_dev, void* stream);
/* Bytes of caller-owned DEVICE scratch one gbnf_trainer_nll_step over n rows needs: the gathered rows, z, ldj, the trace, g_z, g_ldj,
 * the backward workspace and the reductions' partial sums. */
int gbnf_trainer_step_workspace_bytes(const gbnf_trainer* trainer, int64_t n, int64_t* bytes);
/* Replaces: one iteration of density_experiment.py:340-374 for this component -- compute_kl_pq_loss (:606-674), loss.backward(),
 * clip_grad_norm_, optimizer.step() -- for a trainer of any math mode:
 *   1. rows != NULL: the batch is x[rows] (:643-644; `rows`: n int64 DEVICE indices into the n_x rows of x, repeats allowed, an index
 *      outside [0, n_x) is clamped); rows == NULL: x itself, n == n_x required;
 *   2. gbnf_trainer_forward on the live parameters with the trace in `workspace`;
 *   3. nll = mean_i(0.5 sum_j z_ij^2 + 0.5 d log 2 pi - ldj_i)  (:647-649, utils/distributions.py:44-60) and its seed g_z = z / n,
 *      g_ldj = -1 / n;
 *   4. `grads` is zeroed, then gbnf_trainer_backward with that trace (no g_x): it holds this step's unclipped gradient afterwards;
 *   5. gbnf_trainer_apply_update;  6. stats_dev[0] = nll.
 * Batch-statistics mode (gbnf_trainer_set_batch_stats(1), n >= 2) with bn_momentum >= 0: behind the forward every step with bound
 * statistics gets  running = bn_momentum * running + (1 - bn_momentum) * batch  on its bound running mean and variance
 * (models/layers.py:339-344).  GBNF_ERR_INVALID (nothing launched): the cases of apply_update, a workspace smaller than
 * gbnf_trainer_step_workspace_bytes(n), rows == NULL with n != n_x, n < 1. */
int gbnf_trainer_nll_step(const gbnf_trainer* trainer, const float* x, int64_t n_x, const int64_t* rows, int64_t n,
                          float* grads, float* exp_avg, float* exp_avg_sq, const gbnf_opt_hyper* hyper,
                          float* stats_dev, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- boosting: the step of a component beyond the first, and the mixture weight behind it --------------------------------------
 * Replaces: compute_kl_pq_loss for a boosted component (density_experiment.py:609-653) followed by loss.backward(), clip_grad_norm_
 * and optimizer.step() (:361-374) for the component being trained, in ONE call on `stream`, with no host read and no synchronisation:
 *   1. gbnf_mixture_log_prob over components [0, n_fixed) of `fixed` (:612-622; numerics guard and repair pass included) -> G;
 *   2. the gbnf_boosting_weights arithmetic on G (:624-640) -> w;
 *   3. gbnf_resample_rows of w on the caller's uniforms u (n DEVICE floats in [0,1)) (:643) -> rows;
 *   4. gbnf_trainer_nll_step on x (n rows) with those rows (:644-653, :361-374).
 * stats_dev: 8 floats of DEVICE memory: [0..3] as gbnf_trainer_nll_step writes them; [4] G_nll = -mean(G) and [5] the effective sample
 * size (sum w)^2 / sum w^2, both summed in double precision in a fixed order; [6] how many weights were negative or non-finite (0 on
 * healthy input); [7] 0.  rows_out: n DEVICE int64 that receive the drawn rows, or NULL.  workspace: caller-owned DEVICE scratch of
 * gbnf_boosted_step_workspace_bytes bytes -- the nll_step workspace, the (n_fixed, n) log-likelihood table, G, w, the cdf and the rows,
 * each 256-byte aligned.  GBNF_ERR_INVALID (nothing launched): everything gbnf_trainer_nll_step refuses, n_fixed < 1 or more than
 * `fixed` holds, a mixture whose d differs from the trainer's, a null u, x or rho_dev, a short workspace.  The FIRST component has no
 * fixed mixture (:655-661): it keeps gbnf_trainer_nll_step. */
int gbnf_boosted_step_workspace_bytes(const gbnf_mixture* fixed, int32_t n_fixed, const gbnf_trainer* trainer, int64_t n,
                                      int64_t* bytes);
int gbnf_boosted_nll_step(const gbnf_mixture* fixed, int32_t n_fixed, const float* rho_dev, float beta, const gbnf_trainer* trainer,
                          const float* x, int64_t n, const float* u, float* grads, float* exp_avg, float* exp_avg_sq,
                          const gbnf_opt_hyper* hyper, float* stats_dev, int64_t* rows_out, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* Replaces: ONE iteration of BoostedFlow.update_rho (models/boosted_flow.py:119-207, the approximate branch) for `component` >= 1 of a
 * mixture that holds at least components [0, component]: one gbnf_mixture_component_log_prob launch for all of them into
 * ll_workspace ((component + 1, n) DEVICE floats, also an output), then per row
 *   fixed_ll = ll_0;  for c = 1 .. component - 1:  fixed_ll = LSE(log(1 - rho[c]) + fixed_ll, log(rho[c]) + ll_c)
 * -- the reference's UN-normalised recursion (:124-137), NaN for rho[c] > 1 included --, new_ll = ll_component,
 *   grad = mean(fixed_ll - new_ll)                                        (summed per workgroup, re-added in a fixed order in double)
 *   rho[component] = min(max(rho[component] - step_size * grad, 0.01), 100)   (:193-199), written in place on the DEVICE buffer.
 * Only entry `component` of rho_dev is written, and the recursion never reads it.  stats_dev: 4 DEVICE floats [grad, rho before,
 * rho after, |after - before|].  No host read, no synchronisation; the step-size schedule and the stopping rule (:193, :200-204) stay with
 * the caller.  The partial sums live in a per-device buffer of the library: two calls on one device must not run concurrently. */
int gbnf_mixture_rho_step(const gbnf_mixture* mix, const float* x, int64_t n, int32_t component, float* rho_dev, float step_size,
                          float* ll_workspace, float* stats_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Image components (BASELINE.json configs[3]): density evaluation of one multi-scale image
 * Glow, models/glow.py:92-110 with the image branches of FlowNet / FlowStep (:192-252, :317-342).  All arrays are HOST
 * pointers read at creation (the handle is immutable, like gbnf_flow).
 * --------------------------------------------------------------------------------------------------------------- */
/* Conv2d (+ its ActNorm2d) or Conv2dZeros, models/layers.py:577-630: stride 1, 'same' zero padding. */
typedef struct gbnf_conv {
  const float* weight;        /* (out, in, k, k) = nn.Conv2d.weight                                      */
  const float* bias;          /* (out,) or NULL (a Conv2d followed by ActNorm2d has none)                 */
  const float* actnorm_bias;  /* (out,) ActNorm2d.bias after the convolution, or NULL                     */
  const float* actnorm_logs;  /* (out,)                                                                   */
  const float* logs;          /* (out,) Conv2dZeros.logs (output scale exp(3 logs)), or NULL              */
  int32_t out_channels, in_channels, kernel_size;
} gbnf_conv;

/* One image FlowStep: ActNorm2d -> InvertibleConv1x1 | Permute2d -> ConvNet coupling. */
typedef struct gbnf_image_step {
  const float* actnorm_bias;    /* (C,) */
  const float* actnorm_logs;    /* (C,) */
  const float* perm_weight;     /* (C,C) the matrix InvertibleConv1x1.get_weight returns (models/layers.py:751-776,
                                   either parameterisation), or NULL for a channel permutation */
  const int64_t* perm_indices;  /* (C,) Permute2d.indices when perm_weight is NULL */
  int32_t n_convs;              /* coupling_network_depth + 2: 3x3 (+ActNorm2d), 1x1 (+ActNorm2d) x depth, Conv2dZeros 3x3 */
  const gbnf_conv* convs;
} gbnf_image_step;

typedef struct gbnf_image_level {   /* SqueezeLayer(2), n_steps FlowSteps, Split2d (all levels but the last) */
  int32_t n_steps;
  const gbnf_image_step* steps;
  const gbnf_conv* split_prior;     /* Split2d.conv (Conv2dZeros C/2 -> C), NULL on the last level */
} gbnf_image_level;

typedef struct gbnf_image_flow_desc {
  int32_t channels, height, width;  /* input_size, e.g. 3, 32, 32 */
  int32_t n_levels;                 /* L = num_blocks */
  int32_t coupling;                 /* GBNF_COUPLING_* */
  int32_t hidden;                   /* h_size (width of the coupling ConvNets) */
  float bounds;                     /* Glow.bounds, models/glow.py:50 (0.9) */
  const gbnf_image_level* levels;
  const gbnf_conv* learn_top;       /* Glow.learn_top_fn (Conv2dZeros 2Cz -> 2Cz) or NULL: zero-mean unit-variance prior */
} gbnf_image_flow_desc;

typedef struct gbnf_image_flow gbnf_image_flow;

/* LIMITS of the image path (enforced with GBNF_ERR_UNSUPPORTED): inputs of at most 32 x 32 pixels with even sides at every squeeze,
 * 1 to 3 levels -- the reference's CIFAR-10 / SVHN (3 x 32 x 32), MNIST / Omniglot / Caltech (1 x 28 x 28) and Frey faces (1 x 28 x 20)
 * loaders, utils/load_data.py:389-529.  The kernels work on 16- and 8-wide square maps; a smaller map (a 14 x 14 first level, the
 * 4 x 4 map of a third level) lives in the top-left corner of that storage, zero outside (x, z, eps and noise at the boundary
 * always have the map's own size);
 * <= 64 channels per level; coupling ConvNets of hidden width <= 512 with 2 .. 5 convolutions (coupling_network_depth 0 .. 3);
 * the split-f16 kernels serve depth 1 at every hidden width (above 256 the fused kernel works in two halves of the hidden
 * channels), depth 0 and 2 to hidden width 256 (round 6), and <= 24 input channels of the first 3 x 3 (the 48-channel third level of a
 * 3 x 32 x 32 input); everything else runs on the exact-f32 convolution kernels.  Class conditioning (`--y_condition`) is the
 * gbnf_image_flow_set_ycond family below: at most 256 classes, the cross_entropy branch of the reference's class loss only (its
 * `multi_class` branch is reachable from no option of the reference and applies a sigmoid twice: left out).  Not built: learned
 * dequantisation flows. */
int gbnf_image_flow_create(const gbnf_image_flow_desc* desc, gbnf_image_flow** out);
/* ... with an explicit GBNF_MATH_* mode: DEFAULT (what gbnf_image_flow_create does: split-f16 coupling nets if the create-time
 * probe passes), F32 (exact-f32 convolutions everywhere, no probe), F16X3. */
int gbnf_image_flow_create_mode(const gbnf_image_flow_desc* desc, int32_t math_mode, gbnf_image_flow** out);
int gbnf_image_flow_destroy(gbnf_image_flow* flow);
/* Shape of z (per image) and the algorithmic multiply-adds per image; any pointer may be NULL. */
int gbnf_image_flow_info(const gbnf_image_flow* flow, int32_t* z_channels, int32_t* z_height, int32_t* z_width,
                         double* macs_per_image);
int gbnf_image_flow_workspace_bytes(const gbnf_image_flow* flow, int64_t n, int64_t* bytes);
/* Replaces: z, z_mu, z_var, logdet, _ = self.flows[c](x) for image input (models/glow.py:92-110) and
 * ll = log_normal_diag(z, z_mu, z_var) + logdet (image_experiment.py:227).  x (n,C,H,W) in [0,1]; noise (n,C,H,W) is the
 * U(0,1) dequantisation noise of models/glow.py:135 (NULL = none); z (n,Cz,Hz,Wz) and ll (n,) may be NULL; ldj (n,) is
 * required (it is also the accumulator).  z_mu / z_var are per-channel constants: gbnf_image_flow_prior. */
int gbnf_image_flow_forward(const gbnf_image_flow* flow, const float* x, const float* noise, int64_t n, float* z,
                            float* ldj, float* ll, void* workspace, int64_t workspace_bytes, void* stream);
/* The top prior per channel: mean (Cz,) then log-variance (Cz,) into a HOST buffer of 2 Cz floats. */
int gbnf_image_flow_prior(const gbnf_image_flow* flow, float* mean_logvar_host);
/* Deterministic mode of an evaluation handle, a property of the handle like gbnf_image_trainer_set_deterministic of the
 * trainer (off at creation; with it off the launches, the results and the workspace sizes are what they always were: the
 * coupling / Split2d epilogues add their per-wave log-det partials into ldj[n] with float atomics in no fixed order, and
 * ldj / ll of identical calls may differ in the last bit; z never does).  While it is on, for a fixed handle and fixed
 * inputs, z, ldj, ll (and y_logits) of gbnf_image_flow_forward / gbnf_image_flow_forward_y are bit-identical on every
 * call, and ldj / ll of an image do not depend on n or on the image's place in the batch.  So are the outputs built on
 * them: stats_dev[4..6] of gbnf_image_boosted_nll_step / _y and what gbnf_image_mixture_rho_step writes, when every handle
 * of the call has the mode on.
 * How: every wave of a log-det-carrying launch STORES its partial (zero if it ran no epilogue) to a slot of its image --
 * slot = (launch in the chain, strip / workgroup of the image, wave), a function of the handle's geometry and of the
 * kernels its math mode runs, never of n -- in ONE (n, S) array in the workspace, and one small launch in front of the
 * last kernel adds an image's slots in slot order onto ldj[n].  The same-call repair of a split-f16 handle adds a repaired
 * image's slots in the order an exact-f32 handle does: its ldj / ll equal those of a GBNF_MATH_F32 handle in this mode bit
 * for bit.  z is untouched by the mode.  gbnf_image_flow_inverse writes no log-det and is unchanged.
 * gbnf_image_flow_workspace_bytes (and gbnf_image_rho_step_workspace_bytes / gbnf_image_boosted_step_workspace_bytes over
 * such handles) report the larger size while the mode is on: ask again after switching.  A call whose workspace_bytes is
 * short answers GBNF_ERR_INVALID ("deterministic mode is on") before anything is launched.  gbnf_image_flow_actnorm_stats
 * reads nobody's log-det, keeps the atomic form and needs the mode-off size only.
 * A captured graph keeps the mode the handle had at capture time: switching the mode afterwards does not change that graph
 * (re-capture to change it).  Nothing is promised across different handles' math modes, builds or devices. */
int gbnf_image_flow_set_deterministic(gbnf_image_flow* flow, int32_t on);
int gbnf_image_flow_get_deterministic(const gbnf_image_flow* flow, int32_t* on);
/* ---- class-conditional components (Glow with y_condition, models/glow.py:36-39, 62-84, 105-106) --------------------------------
 * Y = y_classes, (Cz, Hz, Wz) the top latent, HW = Hz * Wz (the map proper), top_h = what gbnf_image_flow_prior returns.
 *   prior:  u = y W_c^T + b_c (n, 2Cz);  h_i = top_h + u_i exp(3 l_c);  z_mu[i,c] = h_i[c], z_var[i,c] = h_i[Cz + c], constant over the map;
 *           ll_i = sum -0.5 (lv + (z - mu)^2 e^-lv) + ldj_i  (no 2 pi term, as everywhere on the image path);
 *   head:   zbar[i,c] = mean of z[i,c] over the map;  y_logits_i = (zbar_i W_k^T + b_k) exp(3 l_k)  (n, Y).
 * y (n, Y) is used as given: its rows need not be one-hot.
 * gbnf_image_flow_set_ycond: project_ycond (cond_w (2Cz, Y), cond_b (2Cz,), cond_logs (2Cz,)) and project_class (class_w (Y, Cz),
 * class_b (Y,), class_logs (Y,); all three NULL: no class head, no logits) as HOST pointers, copied at the call (it allocates and
 * may be repeated).  1 <= Y <= 256 (GBNF_ERR_UNSUPPORTED above).  From then on the handle is class-conditional:
 * gbnf_image_flow_forward and gbnf_image_flow_prior answer GBNF_ERR_INVALID ("needs y"), as do the calls built on them
 * (gbnf_image_mixture_rho_step, gbnf_image_boosted_nll_step), and gbnf_image_flow_workspace_bytes reports a larger size (a compact z
 * and a scratch ll behind the plain call's workspace).  gbnf_image_flow_inverse is unchanged: it starts from z.
 * gbnf_image_flow_forward_y: x, noise, z, ldj as gbnf_image_flow_forward; y (n, Y) DEVICE; ll (n,) and y_logits (n, Y) may be NULL
 * (y_logits on a handle without a class head: GBNF_ERR_INVALID).  The plain forward runs first with the y-free prior, its ll kept in
 * the workspace, so the numerics protocol (range marks, the same-call repair launch, the on-data check) acts exactly as on a plain
 * call; ONE more launch behind the repair launch in stream order then computes ll under the image's own prior and the logits from
 * the (repaired) z and ldj: one workgroup per image, sums in double precision in a fixed order, no atomics.  No host read, no
 * synchronisation, no allocation.
 * gbnf_image_flow_prior_y: mean_logvar (n, 2Cz) DEVICE (mean half, log-variance half per image) and / or, with e (n, Cz, Hz, Wz)
 * standard-normal draws, the top latent of a class-conditional sample z_out = mu + exp(lv) * temperature * e -- the reference's
 * torch.normal(z_mu, exp(z_var) * temperature) as written (models/glow.py:116; note exp(lv), not exp(lv / 2)).  Either output may be
 * NULL; z_out needs e.  gbnf_image_flow_y_classes: 0 for a plain handle. */
int gbnf_image_flow_set_ycond(gbnf_image_flow* flow, int32_t y_classes, const float* cond_w, const float* cond_b,
                              const float* cond_logs, const float* class_w_or_null, const float* class_b, const float* class_logs);
int gbnf_image_flow_y_classes(const gbnf_image_flow* flow, int32_t* y_classes);
int gbnf_image_flow_forward_y(const gbnf_image_flow* flow, const float* x, const float* noise, const float* y_dev, int64_t n,
                              float* z, float* ldj, float* ll, float* y_logits_or_null, void* workspace, int64_t workspace_bytes,
                              void* stream);
int gbnf_image_flow_prior_y(const gbnf_image_flow* flow, const float* y_dev, int64_t n, const float* e_or_null, float temperature,
                            float* mean_logvar_dev_or_null, float* z_out_or_null, void* stream);
/* Label-free evaluation of a class-conditional handle: the log-density of every image under EVERY class from ONE pass of the flow.
 * In the reference's Glow the class enters the top prior only (models/glow.py:62-84): x -> (z, ldj) does not depend on y.  So
 *   table[i, k] = sum_{c,p} -0.5 (lv_c + (z[i,c,p] - mu_c)^2 e^-lv_c) + ldj[i],   h = (mu | lv) = top_h + (W_c[:, k] + b_c) exp(3 l_c)
 * -- the ll gbnf_image_flow_forward_y writes for row i with y = the one-hot row of class k, within 1 float32 ulp (both are double
 * sums rounded once) -- for all Y classes costs one flow pass and one small launch instead of Y calls of gbnf_image_flow_forward_y.
 * x, noise, z, ldj, y_logits, workspace as gbnf_image_flow_forward_y (the logits do not depend on y either: they are that call's to
 * the bit); table (n, Y) DEVICE.  The plain forward runs first with the handle's numerics protocol unchanged (range marks, same-call
 * repair, on-data check); ONE launch behind the repair in stream order then reads the compact (repaired) z: per image and channel the
 * mean and the centred second moment of z over the map, in double precision, then per class Cz terms -- sum (z - mu)^2 =
 * M2 + HW (zbar - mu)^2, two non-negative terms.  Every sum runs in an order the sizes alone decide, no atomics: with the handle in
 * deterministic mode (gbnf_image_flow_set_deterministic) table is bit-identical across calls and a row does not depend on n or on
 * its position in the batch.  GBNF_ERR_INVALID (nothing launched): a handle without conditioning, a null x / ldj / table / workspace,
 * a short workspace (gbnf_image_flow_workspace_bytes), y_logits on a handle without a class head.  n == 0: GBNF_OK.  No host read,
 * no synchronisation, no allocation. */
int gbnf_image_flow_forward_classes(const gbnf_image_flow* flow, const float* x, const float* noise, int64_t n, float* z_or_null,
                                    float* ldj, float* table, float* y_logits_or_null, void* workspace, int64_t workspace_bytes,
                                    void* stream);
/* Bayes' rule on such a table (of one component, or of the boosted mixture: gbnf_mixture_lse over the (C, n Y) view of the components'
 * tables): class_ll (n, Y) DEVICE, log_prior (Y,) DEVICE log-probabilities or NULL for the uniform prior -log Y;
 *   log_px[i] = LSE_k(log_prior[k] + class_ll[i, k])  (n,)       the label-free log-density
 *   log_post[i, k] = log_prior[k] + class_ll[i, k] - log_px[i]   (n, Y), or NULL
 *   pred[i] = the first largest entry of row i of log_post as float32 (n,) int32, or NULL (a NaN never wins; a row of NaNs: 0)
 * in double precision in a fixed order, rounded once, with torch.logsumexp's treatment of infinities (a row of -inf: log_px = -inf, and
 * log_post = NaN as in torch).  1 <= Y <= 256 (GBNF_ERR_INVALID below, GBNF_ERR_UNSUPPORTED above); a null class_ll or log_px:
 * GBNF_ERR_INVALID; n == 0: GBNF_OK.  One launch, no host read. */
int gbnf_class_posterior(const float* class_ll, const float* log_prior_or_null, int64_t n, int32_t Y, float* log_px,
                         float* log_post_or_null, int32_t* pred_or_null, void* stream);
/* State of the image path's numerics protocol (the tabular one: gbnf_flow_numerics).  The coupling nets run on
 * split-f16 MFMA (GBNF_MATH_F16X3) when the create-time probe -- 4 synthetic images through both arithmetic paths --
 * agrees with the exact-f32 kernels to `tolerance` (worst_rel_err = what it measured), else the handle runs on exact f32
 * (math_mode GBNF_MATH_F32, demoted = 1).  On split-f16 every operand is range-watched, and what the watch finds is dealt
 * with IN THE SAME CALL, on the same stream, for every image concerned (round 5: no capacity, no "from the next call on"):
 *   - range: an image that met a value beyond +-65504 is counted (gbnf_saturation_count) and marked; ONE repair launch behind
 *     the split-f16 pass (it returns at once when no image of the call is marked) walks every marked image through the
 *     exact-f32 sequence and overwrites its z / ldj / ll (x on the way back): the caller sees what a GBNF_MATH_F32 handle
 *     returns, never NaN and never a clamped value.  Slow per image (one workgroup each), rare by construction.
 *   - precision on the caller's data: on a handle's first forward launch and every `check_every`-th after it (gbnf_tuning_set;
 *     counted on the device, so HIP-graph replays are covered) up to 2 unmarked images are evaluated on exact f32 as well and
 *     compared with the split-f16 result on the device (`check_tolerance_e9`).  A failed check makes the repair launch of that
 *     very call -- and of every later one -- re-evaluate ALL images, and raises a pinned word: later (non-captured) calls run
 *     the exact-f32 kernels directly (math_mode reads GBNF_MATH_F32, demoted = 1).  gbnf_image_flow_inverse does the same on a
 *     device-side launch count of its own: up to 2 unmarked images are walked through the exact-f32 z -> x sequence and their x
 *     compared in place,  err = max |x16 - x32| / max(1, max |x32|)  over the image, failing when err > 2 `check_tolerance_e9`
 *     (x is held to twice the log-likelihood's bar, as on the tabular path).  A failure of either direction demotes both;
 *     its counters: gbnf_image_flow_inverse_check_counts.
 * Environment GBNF_IMAGE_REPAIR=0: nothing behind the split-f16 pass (timing only: out-of-range images keep clamped values).
 * `checks` = calls that marked an image so far; gbnf_image_flow_repair_counts has the rest.  Never synchronises. */
int gbnf_image_flow_numerics(const gbnf_image_flow* flow, gbnf_numerics_status* out);
/* Counters of that protocol (pinned host words the device updates; no synchronisation; any pointer may be NULL): calls that
 * marked an image, images re-evaluated on exact f32, on-data checks completed / failed, the worst relative log-likelihood
 * difference a check has seen. */
int gbnf_image_flow_repair_counts(const gbnf_image_flow* flow, int64_t* marked_calls, int64_t* repaired_images,
                                  int64_t* data_checks, int64_t* failed_checks, float* worst_check_rel_err);
/* The on-data checks of the z -> x direction (gbnf_image_flow_inverse): images checked / failed and the worst relative difference of
 * x a check has seen.  data_checks / failed_checks of gbnf_image_flow_repair_counts count the forward direction only.  Pinned
 * host words, no synchronisation; any pointer may be NULL. */
int gbnf_image_flow_inverse_check_counts(const gbnf_image_flow* flow, int64_t* data_checks, int64_t* failed_checks,
                                         float* worst_rel_err);
/* Replaces (one layer at a time): _ActNorm.initialize_parameters for ActNorm2d (models/layers.py:473-486, 548-557), the
 * data-dependent initialisation the first training-mode forward of an image Glow performs layer by layer.  ActNorm2d number
 * `index` of the component in module order -- per FlowStep its own ActNorm2d, then the one behind each Conv2d of its coupling
 * net (models/glow.py:283-308, models/layers.py:577-606) -- sees a tensor (n, channels, H, W); this call evaluates the component
 * on (x, noise) up to that tensor with the exact-f32 kernels and writes mean_dev[c] = mean over (n, H, W) and var_dev[c] =
 * mean((t - mean)^2) (device, `channels` floats each; *channels is set).  The caller sets bias = -mean,
 * logs = log(scale / (sqrt(var) + 1e-6)), re-creates the handle and moves to the next index: the reference's sequence.  Valid for
 * a layer whose bias and logs are still zero (an un-initialised ActNorm2d is the identity).  index past the last layer:
 * GBNF_ERR_INVALID.  workspace: gbnf_image_flow_workspace_bytes(flow, n). */
int gbnf_image_flow_actnorm_stats(const gbnf_image_flow* flow, const float* x, const float* noise, int64_t n, int32_t index,
                                  float* mean_dev, float* var_dev, int32_t* channels, void* workspace, int64_t workspace_bytes,
                                  void* stream);
/* The z -> x direction.  Replaces: x = self.flows[c].decode(z, None, temperature) for image input (models/glow.py:112-123):
 * FlowNet.decode (models/glow.py:254-260) = per level, last first: Split2d reverse (models/layers.py:695-699: the dropped
 * half is re-drawn as Normal(mean, exp(log-var) * temperature) with (mean, log-var) = conv(z1)), the FlowSteps backwards
 * (FlowStep.decode, models/glow.py:344-366: coupling^-1, torch.inverse of the 1x1 weight or indices_inverse, ActNorm2d
 * reverse), unsqueeze2d (utils/utilities.py:121-135); then to_logits(reverse=True) (models/glow.py:151-158).
 * z (n,Cz,Hz,Wz); x (n,C,H,W).  eps: the standard-normal draws behind Split2d's samples (the caller's RNG, so that
 * sampling is reproducible and testable): level 0 first, each level a contiguous (n, C_l/2, H_l, W_l) array,
 * gbnf_image_flow_eps_floats() floats per image in all (= C*H*W - Cz*Hz*Wz); may be NULL for a one-level flow.
 * The coupling networks run on the fused split-f16 kernel like the forward where the handle does; an image whose hidden
 * activation leaves the fp16 range is re-evaluated on the exact-f32 sequence by the repair launch behind the pass, in this
 * call, and the on-data precision check runs on this direction's first launch and every `check_every`-th after it: a call whose
 * check fails returns the exact-f32 x for every image (see gbnf_image_flow_numerics).  A handle created with GBNF_MATH_F32, demoted
 * by the probe or by an on-data check of either direction runs the exact-f32 convolution kernels.  workspace as for
 * gbnf_image_flow_forward. */
int gbnf_image_flow_eps_floats(const gbnf_image_flow* flow, int64_t* per_image);
int gbnf_image_flow_inverse(const gbnf_image_flow* flow, const float* z, const float* eps, float temperature, int64_t n,
                            float* x, void* workspace, int64_t workspace_bytes, void* stream);
/* The full-latent x -> (z, eps) direction: gbnf_image_flow_forward that KEEPS the half each Split2d level drops instead of only
 * folding its density into ldj.  x, noise, z, ldj, ll, the workspace (gbnf_image_flow_workspace_bytes: unchanged, eps goes straight
 * to the caller's buffer) and the numerics protocol are those of gbnf_image_flow_forward; z and ldj are required here.
 * eps: gbnf_image_flow_eps_floats() floats per image in the layout gbnf_image_flow_inverse reads -- level 0 first, each level a
 * contiguous (n, C_l/2, H_l, W_l) array of the map's own size -- holding eps = (z2 - mean) * exp(-log-var) with (mean, log-var) =
 * split_prior(z1) (models/layers.py:689-703), the exact algebraic inverse of Split2d's reverse at temperature 1; may be NULL
 * only for a one-level flow.  Contract: gbnf_image_flow_inverse(z, eps, temperature = 1) on this call's outputs returns the
 * dequantised input u = (255 x + noise) / 256 (to the rounding of the two passes).  A caller who wants another temperature
 * divides eps.  An image that the split-f16 pass marks out of range, and every image of a call whose on-data check failed, gets its
 * eps from the exact-f32 sequence in the same call, like its z / ldj / ll.  Deterministic mode (gbnf_image_flow_set_deterministic)
 * is honoured (ordered log-det sums); z and eps are identical in both modes.  A class-conditional handle is accepted, since
 * x -> (z, eps, ldj) does not depend on y; on such a handle ll must be NULL (it needs y: GBNF_ERR_INVALID otherwise).
 * GBNF_ERR_INVALID before any launch: null flow / x / z / ldj / workspace, null eps on a multi-level flow, a short workspace,
 * n < 0.  n == 0: GBNF_OK.  No host read, no synchronisation, no allocation: the call can be captured in a graph. */
int gbnf_image_flow_encode(const gbnf_image_flow* flow, const float* x, const float* noise, int64_t n, float* z, float* eps,
                           float* ldj, float* ll_or_null, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Training path of ONE image Glow component: the forward on the LIVE parameters and its backward pass, exact f32
 * (the image counterpart of gbnf_trainer_*).  The descriptor is the evaluation one, but every float pointer is a DEVICE
 * pointer to the caller's live tensor in its reference layout (perm_indices stay HOST pointers, read at creation).
 * Nothing is copied: every forward call re-derives the kernels' weight tiles from the tensors on the device (one launch),
 * so parameters an optimiser updates in place are seen by the next call; re-create the trainer only when a tensor is
 * re-allocated.  `learn_top` is ignored: the top prior is the caller's (a Conv2dZeros of a zero input is
 * bias * exp(3 logs), differentiable in closed form).  The limits are those of gbnf_image_flow_create with 1 to 3 levels
 * and the same depth and width in every coupling net; anything else answers GBNF_ERR_UNSUPPORTED with the reason.
 * Calls on one trainer must not run concurrently (the weight tiles are the trainer's).
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct gbnf_image_trainer gbnf_image_trainer;
int gbnf_image_trainer_create(const gbnf_image_flow_desc* desc_device_params, gbnf_image_trainer** out);
int gbnf_image_trainer_destroy(gbnf_image_trainer* trainer);
/* Floats of the trace buffer / bytes of the workspace (forward and backward share one size; larger in deterministic mode,
 * below) at a batch of n images. */
int gbnf_image_trainer_trace_floats(const gbnf_image_trainer* trainer, int64_t n, int64_t* floats);
int gbnf_image_trainer_workspace_bytes(const gbnf_image_trainer* trainer, int64_t n, int64_t* bytes);
/* x, noise, z as gbnf_image_flow_forward (z may be NULL); the same values as a GBNF_MATH_F32 evaluation handle with ONE
 * difference: ldj (n,) EXCLUDES the log-determinants of the 1 x 1 `perm_weight` matrices.  The caller adds
 * sum over the steps of H_l * W_l * log|det W| (H_l x W_l: the map of the step's level): a per-component scalar,
 * differentiable in closed form on C x C matrices.  trace (required) receives what the backward needs: per level the
 * level's input and, per FlowStep, the state behind its ActNorm2d + 1 x 1 (the coupling's input) and the step's output
 * (the last one is the Split2d's input).  Hidden activations are not kept: the backward recomputes them. */
int gbnf_image_trainer_forward(gbnf_image_trainer* trainer, const float* x, const float* noise, int64_t n, float* z,
                               float* ldj, float* trace, void* workspace, int64_t workspace_bytes, void* stream);
/* Floats of the flat gradient buffer.  Layout, in descriptor order:  per level, per step:
 *   [actnorm bias (C)] [actnorm logs (C)] [perm_weight (C*C), when not NULL]
 *   then per convolution of the step, those arrays that are present: [weight] [bias] [actnorm_bias] [actnorm_logs] [logs];
 * behind a level's steps, the level's split_prior convolution in the same form. */
int gbnf_image_trainer_grad_floats(const gbnf_image_trainer* trainer, int64_t* floats);
/* trace: what gbnf_image_trainer_forward left at the same n, parameters unchanged since.  g_z (n,Cz,Hz,Wz) and g_ldj (n,)
 * may each be NULL, meaning zero.  ACCUMULATES into grads (the caller zeroes it).  The ActNorm2d `logs` gradients include
 * the H*W * sum_n g_ldj[n] term of their own log-determinant; the `perm_weight` gradient is the data path only, consistent
 * with the forward.  This call returns no gradient with respect to x (gbnf_image_trainer_backward_x does).  By default the weight
 * gradients are summed with float atomics across the (image, strip) slices of a layer: their last bits depend on the order; in
 * deterministic mode (below) every slice stores its partial and the partials are added in slice order. */
int gbnf_image_trainer_backward(gbnf_image_trainer* trainer, const float* trace, int64_t n, const float* g_z,
                                const float* g_ldj, float* grads, void* workspace, int64_t workspace_bytes, void* stream);
/* gbnf_image_trainer_backward with the gradient with respect to the input: x and noise (NULL = none) as the forward that left
 * `trace` took them, g_x (n, C, Hi, Wi) DEVICE, accumulate != 0: g_x += the gradient, else it is stored (every pixel is written).
 * The state gradient goes through the first step's ActNorm2d + 1 x 1 like through every other step (the same convolution kernel),
 * then one elementwise launch applies the adjoint of dequantise + logit + first squeeze: with v the forward's pre-logit value,
 * recomputed in f32 from x and noise,
 *   g_x = (g_logit + g_ldj[n] (2v - 1)) / (v (1 - v)) * bounds * 255 / 256
 * on the Hi x Wi image proper (storage outside it carries no gradient).  noise is held fixed: this is the gradient of the
 * dequantised density at that noise.  No atomics on the data path: g_x repeats bit for bit in either mode.
 * grads non-NULL: the weight gradients are ACCUMULATED as gbnf_image_trainer_backward does (bit-equal to it in deterministic
 * mode).  grads NULL: the data-gradient-only form -- no weight-gradient launch, no scratch memset, no partial-sum reduce, no
 * unfold; g_x is bit-equal to the call with grads.  GBNF_ERR_INVALID (nothing launched): a null trainer / trace / x / g_x, n < 0,
 * a workspace below gbnf_image_trainer_workspace_bytes(n); GBNF_ERR_UNSUPPORTED: more than 65535 images.  n == 0: GBNF_OK. */
int gbnf_image_trainer_backward_x(gbnf_image_trainer* trainer, const float* trace, const float* x, const float* noise, int64_t n,
                                  const float* g_z, const float* g_ldj, float* grads_or_null, float* g_x, int32_t accumulate,
                                  void* workspace, int64_t workspace_bytes, void* stream);
/* The autograd seed of  r[i] * (log_normal_diag(z_i, mu, logvar) + ldj_i)  (no 2 pi term; image_experiment.py:227):
 *   g_z = -r (z - mu) exp(-logvar)  (n, Cz, HW),   g_ldj = r  (n,).
 * z (n, Cz, HW) compact as gbnf_image_trainer_forward writes it; prior: (mu | logvar), 2 Cz floats per row with a row stride of 0
 * (one prior for all rows) or 2 Cz (a class-conditional component's per-image prior, gbnf_image_flow_prior_y's layout); r (n,)
 * DEVICE or NULL = 1.  One elementwise launch.  GBNF_ERR_INVALID: a null z / prior / g_z / g_ldj, n < 0, Cz < 1, HW < 1, another
 * stride. */
int gbnf_image_score_seed(const float* z, const float* prior, int64_t prior_stride, const float* r_or_null, int64_t n, int32_t Cz,
                          int32_t HW, float* g_z, float* g_ldj, void* stream);
/* Responsibilities of a mixture: ll (C, N) and log_w (C,) DEVICE ->
 *   G[n] = LSE_c(log_w[c] + ll[c][n])  (N,),    r[c][n] = exp(log_w[c] + ll[c][n] - G[n])  (C, N): softmax over c.
 * One thread per column, double precision, component order, rounded once.  A column of -inf: G = -inf and r = 0 (no NaN out of
 * inf - inf; torch.logsumexp's value); a NaN entry makes its column NaN.  Where ll came from does not matter: an image table and
 * a tabular gbnf_mixture_component_log_prob table are both (C, N).  GBNF_ERR_INVALID: a null pointer, n_components < 1, n < 0. */
int gbnf_mixture_responsibilities(const float* ll, const float* log_w, int32_t n_components, int64_t n, float* r, float* G,
                                  void* stream);
/* The score of the boosted image mixture in ONE call:  log p(x) = LSE_c(log_w[c] + ll_c(x))  over the trainers of components
 * 0 .. n_components - 1 and  g_x = grad_x log p(x) = sum_c r_c grad_x ll_c,  with no host read, no synchronisation, no allocation:
 *   1. per component: the 1 x 1 log-dets (LU matrices composed, as gbnf_image_trainer_nll_step's first launch),
 *      gbnf_image_trainer_forward, and ll_c = log_normal_diag(z, top prior) + ldj + the log-dets (double sums, fixed order);
 *   2. gbnf_mixture_responsibilities -> G (n,), r (C, n) (copied to r_or_null when given);
 *   3. per component, in order: gbnf_image_score_seed with row c of r, then the data-gradient-only gbnf_image_trainer_backward_x
 *      into g_x (n, C, Hi, Wi) -- stored by component 0, added by the others.  The backward is linear in its seeds, so no
 *      (C, n, C Hi Wi) buffer exists.
 * The trainers carry what the one-call step binds: gbnf_image_trainer_bind_lu, _bind_top (none: the zero-mean unit prior) and, for
 * a class-conditional model, _bind_ycond on every one with y (n, Y) DEVICE given.  noise (NULL = none) is shared by all components
 * and held fixed.  With every trainer in deterministic mode g_x, G and r are bit-identical across calls; otherwise only the
 * forward's log-det atomics can move their last bits.
 * workspace: gbnf_image_mixture_score_workspace_bytes -- per component z, ldj, prior and trace; ll, r, the seed, and the largest
 * gbnf_image_trainer_workspace_bytes.  GBNF_ERR_INVALID (nothing launched): a null trainers / log_w / x / g_x / G / workspace or
 * entry of trainers, n_components < 1, n < 0, trainers of different input shapes or class counts, a trainer whose last bind
 * failed, y missing on conditioned trainers or given to plain ones, a short workspace; GBNF_ERR_UNSUPPORTED: more than 65535
 * images.  n == 0: GBNF_OK. */
int gbnf_image_mixture_score_workspace_bytes(gbnf_image_trainer* const* trainers, int32_t n_components, int64_t n, int64_t* bytes);
int gbnf_image_mixture_score(gbnf_image_trainer* const* trainers, int32_t n_components, const float* log_w, const float* x,
                             const float* noise, const float* y_or_null, int64_t n, float* g_x, float* G, float* r_or_null,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The score of the tabular path: grad_x log p(x) of a flow component and of the boosted mixture ----
 * gbnf_trainer_backward_x: the data-gradient-only form of gbnf_trainer_backward.  g_x (n, d) is required and is STORED, or ADDED
 * to when accumulate != 0; there is no `grads`.  The sweeps of gbnf_trainer_backward run on the launch parameters they always get,
 * so with accumulate == 0 g_x is bit-equal to what that call writes for the same inputs -- on the register-chained sweep, the
 * per-step kernels, a GBNF_MATH_BF16X6 and a repairing trainer, with the forward call's `trace` or NULL (as there: the trace is
 * const for the states only).  What serves the weight gradients alone does not run: no weight-gradient launch, no partial-sum
 * reduce (the chained sweep's ActNorm / BatchNorm partials stay in the slack rows behind the trace), no gradient memset or commit
 * of a repairing trainer; the per-step kernels add their normalisation sums into a discard region of the workspace.  `accumulate`
 * is a temporary (n, d) plus one elementwise launch: the backward kernels only store.
 * workspace: gbnf_trainer_backward_x_workspace_bytes(n) -- gbnf_trainer_workspace_bytes(n) without the weight-gradient partials of
 * deterministic mode (nothing here touches them: the size does not depend on that mode) + the discard region
 * (gbnf_trainer_grad_floats floats) + the g_x of both forms of a repairing trainer (which gbnf_trainer_backward keeps in memory
 * of its own) + the temporary, last: a call with accumulate == 0 is served by a workspace n d floats (rounded up to 256 bytes)
 * shorter.
 * Refused before any launch -- GBNF_ERR_INVALID: a null trainer / x / g_x / workspace, n < 0, a short workspace;
 * GBNF_ERR_UNSUPPORTED: a trainer in batch-statistics mode (gbnf_trainer_set_batch_stats: its input gradient needs the batch
 * sums that only the full backward forms), and the deterministic-mode refusals of gbnf_trainer_backward, unchanged.  n == 0:
 * GBNF_OK. */
int gbnf_trainer_backward_x_workspace_bytes(const gbnf_trainer* trainer, int64_t n, int64_t* bytes);
int gbnf_trainer_backward_x(const gbnf_trainer* trainer, const float* x, int64_t n, const float* trace, const float* g_z,
                            const float* g_ldj, float* g_x, int32_t accumulate, void* workspace, int64_t workspace_bytes,
                            void* stream);
/* The autograd seed of  r[i] * (sum_j log N(z_ij; mean_j, std_j) + ldj_i)  and that sum, in one elementwise launch (one wave per
 * 64 rows, no LDS):
 *   g_z = -r (z - mean) / std^2  (n, d),   g_ldj = r  (n,),   ll[i] = sum_j log N(z_ij; mean_j, std_j)  (n,) unless NULL.
 * mean / std (d,) DEVICE, both or neither; NULL = the standard normal.  r (n,) DEVICE or NULL = 1.  The constant is that of
 * gbnf_mixture_component_log_prob, 2 pi term included; the per-row sum runs in double, in feature order, and is rounded once;
 * the caller adds ldj.  GBNF_ERR_INVALID: a null z / g_z / g_ldj, n < 0, d < 1, exactly one of mean / std. */
int gbnf_score_seed(const float* z, const float* base_mean_or_null, const float* base_std_or_null, const float* r_or_null, int64_t n,
                    int32_t d, float* g_z, float* g_ldj, float* ll_or_null, void* stream);
/* The score of the boosted tabular mixture in ONE call:  log p(x) = LSE_c(log_w[c] + ll_c(x))  over the trainers of components
 * 0 .. n_components - 1 (the closed form of gbnf_mixture_lse's recursion: log_w[c] = log(rho[c] / sum(rho[0:n_components]))) and
 * g_x = grad_x log p(x) = sum_c r_c grad_x ll_c  (n, d),  with no host read, no synchronisation, no allocation:
 *   1. the table ll (C, n): ll_or_null as it is (DEVICE; e.g. gbnf_mixture_component_log_prob's, one launch for all components),
 *      else per component gbnf_trainer_forward into one reused (n, d) buffer and gbnf_score_seed's ll + ldj.  (That forward gets
 *      the call's trace buffer as scratch: every math mode then stays on its register-chained sweep and a range-safe trainer
 *      allocates nothing.)  n_components == 1 without a table: skipped, the ll of step 3's forward is what G is made of;
 *   2. gbnf_mixture_responsibilities -> G (n,), r (C, n) (copied to r_or_null when given);
 *   3. per component, in order: a traced gbnf_trainer_forward, gbnf_score_seed with row c of r, gbnf_trainer_backward_x into g_x
 *      -- stored by component 0, added by the others.
 * base mean / std (d,) DEVICE, both or neither (NULL: N(0, I)); the table given must have been made with the same base.  The
 * workspace (gbnf_mixture_score_workspace_bytes) holds ONE trace, sized for the widest component, not C of them: the price is a
 * second forward per component when no table is given.  On the chained sweeps nothing on the data path is atomic: g_x, G and r
 * repeat bit for bit.
 * Refused with nothing launched -- GBNF_ERR_INVALID: a null trainers / entry of trainers / log_w / x / g_x / G / workspace,
 * n_components < 1, n < 0, trainers of different d, exactly one of mean / std, a short workspace; GBNF_ERR_UNSUPPORTED: a trainer
 * in batch-statistics mode, and gbnf_trainer_backward's deterministic-mode refusals.  n == 0: GBNF_OK. */
int gbnf_mixture_score_workspace_bytes(gbnf_trainer* const* trainers, int32_t n_components, int64_t n, int64_t* bytes);
int gbnf_mixture_score(gbnf_trainer* const* trainers, int32_t n_components, const float* log_w, const float* base_mean_or_null,
                       const float* base_std_or_null, const float* ll_or_null, const float* x, int64_t n, float* g_x, float* G,
                       float* r_or_null, void* workspace, int64_t workspace_bytes, void* stream);

/* Deterministic mode of an image trainer, a property of the trainer like gbnf_trainer_set_deterministic of the tabular one
 * (off at creation; with it off the kernels, the launches, the results and the workspace sizes are what they always were).
 * While it is on, for a fixed trainer, fixed inputs, fixed parameter values, a fixed n and a fixed process environment
 * (GBNF_IMG_WGRAD_ITEMS), these outputs are bit-identical on every call:
 *   gbnf_image_trainer_forward:   z, ldj, trace;
 *   gbnf_image_trainer_backward:  grads (it still ACCUMULATES into them);
 *   gbnf_image_trainer_nll_step:  grads, the parameters, exp_avg, exp_avg_sq, stats_dev[0..3];
 *   gbnf_image_boosted_nll_step:  the same, for the step it contains.
 * How: slice y of a weight-gradient launch stores its dW' tile entries and db' rows to partials[y][..] in the workspace
 * (plain stores, no atomics) and a second launch adds the partials of every entry in slice order; the slice count is a
 * function of the layer's shape, of n and of GBNF_IMG_WGRAD_ITEMS only.  Every wave of a coupling / Split2d epilogue stores
 * its log-det partial to a slot of its image, and a small launch adds an image's slots in slot order onto ldj[n].
 * Everything else in those calls is ordered already.  There are no refusals: every geometry the trainer accepts runs in
 * this mode.  Cost: the largest slices x (cout cin k^2 + cout) floats over the trainer's convolutions and a few dozen
 * floats per image of workspace -- gbnf_image_trainer_workspace_bytes, gbnf_image_trainer_step_workspace_bytes and
 * gbnf_image_boosted_step_workspace_bytes report the larger sizes while the mode is on (ask again after switching it), and
 * a workspace sized before switching it on is refused with GBNF_ERR_INVALID ("workspace too small") before the first
 * launch, never overrun.
 * stats_dev[4..6] of gbnf_image_boosted_nll_step and everything gbnf_image_mixture_rho_step writes come from evaluation
 * handles (gbnf_image_flow_*), which have a deterministic mode of their own: gbnf_image_flow_set_deterministic (above).
 * With it on for every handle of the call, those outputs repeat bit for bit too; with it off their last bit may differ.
 * Nothing is promised across different n, environments, builds or devices. */
int gbnf_image_trainer_set_deterministic(gbnf_image_trainer* trainer, int32_t on);
int gbnf_image_trainer_get_deterministic(const gbnf_image_trainer* trainer, int32_t* on);

/* ---- data-dependent ActNorm2d initialisation of the whole component in ONE pass, on the live tensors ------------------------
 * Replaces: what the reference's FIRST training-mode forward does to every ActNorm2d (models/layers.py:473-486 reached through
 * models/glow.py:92-110), for all layers at once -- gbnf_image_flow_actnorm_stats (above) answers one layer per call on a packed
 * copy and stays as it is.
 * Layers are numbered in module order, as there: per FlowStep its own ActNorm2d, then the one behind each Conv2d of its
 * coupling net (Conv2dZeros, Split2d and the top prior have none); gbnf_image_trainer_actnorm_count gives their number.
 * skip_or_null: a HOST array of `count` bytes, non-zero = this layer is initialised already: its live values are used and
 * not written; NULL = every layer is initialised here.
 * The call walks the forward once on `stream` (x, noise, perm_weight as gbnf_image_trainer_forward reads them; with LU
 * factors bound the matrices are composed first, as step 1 of gbnf_image_trainer_nll_step does).  At a layer to initialise
 * it takes t = the tensor that reaches the layer with every earlier layer as it NOW stands -- a step's own ActNorm2d: the
 * step's input state; a coupling-net layer: the raw output of its convolution, the layer itself treated as the identity
 * whatever its tensors hold --, mean_c and var_c = mean((t - mean_c)^2) over (n, the map proper), and writes
 *   bias_c = -mean_c,   logs_c = log(scale / (sqrt(var_c) + 1e-6))
 * INTO THE LIVE TENSORS, re-derives that layer's weight tiles and goes on with the initialised layer.  The sums are taken in
 * double precision in a fixed order (lane, wave, workgroup, chunk of images; per-chunk partials are stored and added in chunk
 * order, no float atomics): the result is bit-identical from run to run, in and out of deterministic mode.  No z, ldj or
 * trace comes back (run a forward afterwards); the trainer's tiles are left packed for the new values.  No host read, no
 * synchronisation, no allocation.  workspace: caller-owned DEVICE scratch of gbnf_image_trainer_actnorm_init_workspace_bytes(n)
 * bytes; nothing is assumed about what it holds on entry.
 * GBNF_ERR_INVALID (nothing launched): a null trainer / x / count / bytes, n < 1, a scale that is not finite or not > 0, a
 * workspace that is null or too small.  GBNF_ERR_UNSUPPORTED: more than 65535 images. */
int gbnf_image_trainer_actnorm_count(const gbnf_image_trainer* trainer, int32_t* count);
int gbnf_image_trainer_actnorm_init_workspace_bytes(const gbnf_image_trainer* trainer, int64_t n, int64_t* bytes);
int gbnf_image_trainer_actnorm_init(gbnf_image_trainer* trainer, const float* x, const float* noise, int64_t n, float scale,
                                    const uint8_t* skip_or_null, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- one image training step in one call: loss, 1x1 log-determinants, clip, AdamW / SGD -----------------------------------
 * Replaces: one iteration of image_experiment.py:378-419 for the component being trained -- the loss (:227-229)
 *   nll_i = -(log_normal_diag(z, z_mu, z_var) + logdet),  loss = loss_scale * mean_i(nll_i)   (the reference: 1 / (ln 2 C H W)),
 * loss.backward(), clip_grad_norm_ and optimizer.step() (optimization/optimizers.py:54-65) -- on the trainer's live tensors, with no
 * host read and no synchronisation.  The boosted image loss (:247-261) differs from this one by a term that does not depend on the
 * trained component: its gradient is this one, and there is no resampling on the image path (gbnf_image_boosted_nll_step reports
 * that term next to this step).
 *
 * The calls below add what gbnf_image_trainer_forward / _backward leave to the caller:
 *   - the log-determinants of the 1 x 1 matrices, sum over the steps of hw * log|det W| (hw: pixels of the step's level), and their
 *     gradient -loss_scale * hw * W^-T (Gauss-Jordan with partial pivoting in f64; a singular W gives a non-finite nll, as torch);
 *   - the LU form of a 1 x 1 (models/layers.py:757-768): W = p (lower . m + I)(upper . m^T + diag(sign_s e^log_s)), m the strict lower
 *     triangle.  gbnf_image_trainer_bind_lu names the live factors of one step (DEVICE pointers; p and sign_s are buffers); the step's
 *     perm_weight of the descriptor is then the persistent (C, C) tensor the matrix is composed into before each forward of nll_step
 *     (gbnf_image_trainer_forward itself does not compose).  GBNF_ERR_INVALID: a step outside the component or without perm_weight.
 *   - the learned top prior (gbnf_image_trainer_bind_top: learn_top_fn's weight (may be NULL), bias and logs, 2 Cz channels):
 *     h = bias * exp(3 logs), z_mu = h[:Cz], z_var = h[Cz:].  The weight gets a zero gradient but is a region of the update (weight
 *     decay acts on it, as in torch).  Never bound: the zero-mean unit-variance prior.
 * Both bind calls rebuild the trainer's tables (they allocate and synchronise; nll_step does neither).
 *
 * STEP gradient layout (gbnf_image_trainer_step_grad_floats): the gbnf_image_trainer_grad_floats layout unchanged, followed by, per
 * bound LU step in bind order, [lower C*C] [upper C*C] [log_s C], then [top weight] [top bias 2Cz] [top logs 2Cz] when bound.  The
 * perm_weight region of an LU step is reserved: zero behind a step, no tensor behind it, skipped by the update.  The optimiser state
 * (exp_avg / exp_avg_sq) has this layout too. */
int gbnf_image_trainer_bind_lu(gbnf_image_trainer* trainer, int32_t level, int32_t step, const float* p, const float* sign_s,
                               float* lower, float* upper, float* log_s);
int gbnf_image_trainer_bind_top(gbnf_image_trainer* trainer, float* weight_or_null, float* bias, float* logs);
int gbnf_image_trainer_step_grad_floats(const gbnf_image_trainer* trainer, int64_t* floats);
/* Bytes of caller-owned DEVICE scratch of one gbnf_image_trainer_nll_step over n images: z, ldj, the trace, g_z, g_ldj, the
 * forward / backward workspace and the reductions' partial sums. */
int gbnf_image_trainer_step_workspace_bytes(const gbnf_image_trainer* trainer, int64_t n, int64_t* bytes);
/* gbnf_trainer_apply_update for an image trainer: clip_grad_norm_ + the optimiser step from a flat gradient buffer in the STEP
 * layout, same kernels, same stats_dev.  Bit-identical from run to run for the same buffer. */
int gbnf_image_trainer_apply_update(gbnf_image_trainer* trainer, const float* grads, float* exp_avg, float* exp_avg_sq,
                                    const gbnf_opt_hyper* hyper, float* stats_dev, void* stream);
/* The whole step:  1. compose the LU matrices and take every bound 1 x 1's log-det;  2. gbnf_image_trainer_forward (x, noise as
 * there), trace in `workspace`;  3. + 4. the loss with the log-dets added and its seed g_z = k (z - mu) e^-lv / n, g_ldj = -k / n,
 * k = loss_scale;  5. `grads` (STEP layout) is zeroed;  6. gbnf_image_trainer_backward;  7. the log-det, LU and prior gradients are
 * added;  8. gbnf_image_trainer_apply_update.
 * stats_dev (4 floats): [0] mean nll in nats, UNSCALED; [1] the 2-norm of the SCALED gradient (what the reference clips); [2] the clip
 * coefficient; [3] 0.  `grads` holds the unclipped scaled gradient afterwards.  hyper.bn_momentum is ignored.
 * GBNF_ERR_INVALID (nothing launched): the cases of gbnf_trainer_apply_update, n < 1 (or more than 65535 images), a workspace
 * smaller than gbnf_image_trainer_step_workspace_bytes(n), a null x / grads / stats_dev / workspace. */
int gbnf_image_trainer_nll_step(gbnf_image_trainer* trainer, const float* x, const float* noise, int64_t n, float loss_scale,
                                float* grads, float* exp_avg, float* exp_avg_sq, const gbnf_opt_hyper* hyper,
                                float* stats_dev, void* workspace, int64_t workspace_bytes, void* stream);
/* ---- the class-conditional step (image_experiment.py:227-239 with args.y_condition; the cross_entropy branch) ---------------------
 *   loss = loss_scale * mean_i(nll_i) + y_weight * mean_i CE(y_logits_i, t_i),  t_i = the index of the largest entry of y_i (the
 *   lowest index on a tie), nll_i under the per-image prior and y_logits as at gbnf_image_flow_set_ycond.
 * gbnf_image_trainer_bind_ycond names the six live tensors of project_ycond and project_class (DEVICE pointers, all required,
 * 1 <= Y <= 256) and rebuilds the tables as gbnf_image_trainer_bind_top does.  The STEP gradient layout gains, behind the top
 * prior's regions and all subject to the update:
 *   [cond weight 2Cz*Y] [cond bias 2Cz] [cond logs 2Cz] [class weight Y*Cz] [class bias Y] [class logs Y].
 * From then on gbnf_image_trainer_nll_step answers GBNF_ERR_INVALID ("needs y"), gbnf_image_trainer_step_workspace_bytes reports a
 * larger size (the per-image terms), and a workspace sized before binding is refused before the first launch.
 * gbnf_image_trainer_nll_step_y: the eight steps of gbnf_image_trainer_nll_step with y (n, Y) DEVICE, used as given by the prior.
 * Steps 3 + 4 are one launch, one workgroup per image: the prior, the head, a max-subtracted log-softmax, nll_i, CE_i, the seed
 *   g_z = kn (z - mu) e^-lv + ((gl_i * e^{3 l_k}) W_k) / HW,  g_ldj = -kn,  kn = loss_scale / n,  gl_i = (y_weight / n)(softmax - onehot(t_i)),
 * and the image's terms of the gradients of the top prior (now a sum over per-image priors), project_ycond and project_class.  Step 7
 * gains one launch, one thread per parameter entry, that adds those terms in image order in double precision and WRITES the
 * regions.  Neither launch uses an atomic: these regions, stats[4] and stats[5] are bit-identical from run to run in and out of
 * deterministic mode; deterministic mode covers the whole call as it covers gbnf_image_trainer_nll_step.
 * stats_dev (8 floats): [0] mean nll in nats, unscaled, under the y-conditioned prior; [1] [2] norm and clip coefficient of the whole
 * scaled gradient; [3] 0; [4] mean cross-entropy, unweighted; [5] rows whose largest logit (f32, lowest index on a tie) is at t_i;
 * [6] [7] 0.  GBNF_ERR_INVALID (nothing launched): what gbnf_image_trainer_nll_step refuses, a null y, a trainer without
 * conditioning bound. */
int gbnf_image_trainer_bind_ycond(gbnf_image_trainer* trainer, int32_t y_classes, float* cond_w, float* cond_b, float* cond_logs,
                                  float* class_w, float* class_b, float* class_logs);
int gbnf_image_trainer_y_classes(const gbnf_image_trainer* trainer, int32_t* y_classes);
int gbnf_image_trainer_nll_step_y(gbnf_image_trainer* trainer, const float* x, const float* noise, const float* y_dev, int64_t n,
                                  float loss_scale, float y_weight, float* grads, float* exp_avg, float* exp_avg_sq,
                                  const gbnf_opt_hyper* hyper, float* stats_dev, void* workspace, int64_t workspace_bytes,
                                  void* stream);

/* ---- boosting for image components: the mixture weight of a component, and the boosted step's fixed-mixture term -----------------
 * Replaces: ONE iteration of BoostedFlow.update_rho (models/boosted_flow.py:119-207, the approximate branch) for image components --
 * the image counterpart of gbnf_mixture_rho_step -- in one call on `stream`, with no host read and no synchronisation.
 * flows: a HOST array of component + 1 evaluation handles in component order.  x, noise as gbnf_image_flow_forward (noise may be
 * NULL); every component sees the same noise.  For c = 0 .. component the component's forward runs through the code path of
 * gbnf_image_flow_forward -- each handle keeps its own numerics protocol (range marks, the same-call repair launch, the on-data check;
 * a demoted or GBNF_MATH_F32 handle is fine) -- and row c of ll_workspace ((component + 1, n) contiguous DEVICE floats, also an
 * output) receives its ll.  The chains are launched on the caller's stream one after another: the call forks no stream of its own.
 * Then, on that table, exactly what gbnf_mixture_rho_step does: the un-normalised recursion (:124-137), grad = mean(fixed_ll - new_ll),
 *   rho[component] = min(max(rho[component] - step_size * grad, 0.01), 100)   (:193-199), in place on the DEVICE buffer.
 * Only entry `component` of rho_dev is written, and the recursion never reads it.  stats_dev: 4 DEVICE floats [grad, rho before,
 * rho after, |after - before|].  The step-size schedule and the stopping rule (:193, :200-204) stay with the caller.
 *
 * What `ll` means here: the reference's _rho_gradients applies log_normal_standard(z, dim=-1) to z, which for a 4-D image z raises a
 * shape error (and would ignore the learned top prior): that method has never run for images.  This call uses the image path's own
 * log-likelihood, ll = log_normal_diag(z, z_mu, z_var) + logdet (image_experiment.py:227), what gbnf_image_flow_forward writes to `ll`.
 * The update rule, the un-normalised recursion and the clamp are the reference's.  A constant added to every component's ll cancels in
 * fixed_ll - new_ll (every recursion stage weighs with 1 - rho[c] and rho[c]), so the 2 pi term that log_normal_diag leaves out
 * changes nothing.
 *
 * workspace: caller-owned DEVICE scratch of gbnf_image_rho_step_workspace_bytes(flows, component + 1, n) bytes -- the largest
 * gbnf_image_flow_workspace_bytes of the handles and the call's ldj accumulator, each 256-byte aligned.  GBNF_ERR_INVALID (nothing
 * launched): a null flows / x / rho_dev / ll_workspace / stats_dev / workspace or a null entry of flows, component < 1, n < 1, handles
 * whose input shape (channels, height, width) differs, a class-conditional handle anywhere in flows (it needs y: gbnf_image_mixture_rho_step_y), a
 * short workspace.  The partial sums live in the per-device buffer of
 * gbnf_mixture_rho_step: two rho calls on one device must not run concurrently. */
int gbnf_image_rho_step_workspace_bytes(const gbnf_image_flow* const* flows, int32_t n_flows, int64_t n, int64_t* bytes);
int gbnf_image_mixture_rho_step(const gbnf_image_flow* const* flows, int32_t component, const float* x, const float* noise,
                                int64_t n, float* rho_dev, float step_size, float* ll_workspace, float* stats_dev,
                                void* workspace, int64_t workspace_bytes, void* stream);
/* The same iteration for class-conditional components: gbnf_image_mixture_rho_step with y (n, Y) DEVICE, the rows' labels as
 * gbnf_image_flow_forward_y takes them.  Row c of ll_workspace is component c's ll under its prior of each row's y (the code path of
 * gbnf_image_flow_forward_y: the plain chain, the repair, one more launch); the recursion, the update and stats_dev[4] are the plain
 * call's.  Every handle of flows[0 .. component] must be conditioned, all with the same Y: a plain handle among them, a second class
 * count or a null y is GBNF_ERR_INVALID before the first launch, as is everything the plain call refuses.  The workspace is that of
 * gbnf_image_rho_step_workspace_bytes: a conditioned handle's gbnf_image_flow_workspace_bytes already holds its compact z. */
int gbnf_image_mixture_rho_step_y(const gbnf_image_flow* const* flows, int32_t component, const float* x, const float* noise,
                                  const float* y_dev, int64_t n, float* rho_dev, float step_size, float* ll_workspace,
                                  float* stats_dev, void* workspace, int64_t workspace_bytes, void* stream);

/* Replaces: one iteration of image_experiment.py:398-419 for the component being trained, the fixed-mixture term of
 * compute_boosted_loss (:247-261) included -- the image counterpart of gbnf_boosted_nll_step -- in one call on `stream`, with no host
 * read and no synchronisation:
 *   1. gbnf_image_flow_forward of `fixed` (the component the reference draws with _sample_component, :400-401) on (x, noise), ll only;
 *   2. G_nll = mean_i(-max(ll_G,i, g_floor))  (:252-254; the reference's G_MAX_LOSS is -10; g_floor = -INFINITY: no clamp), summed per
 *      workgroup in double precision and re-added in a fixed order; a NaN ll stays NaN, as torch.max keeps it.  The same pass counts
 *      the rows with ll_G < g_floor or a non-finite ll_G;
 *   3. gbnf_image_trainer_nll_step on the same (x, noise), unchanged;
 *   4. stats[5] = stats[0] - stats[4].
 * The G term does not depend on the trained parameters, and this call NEVER differentiates it: in the reference a gradient could flow
 * through max only for rows above the floor of a fixed component that is also the one being trained (the first component, all_trained
 * False); the gradient here is that of gbnf_image_trainer_nll_step in every case.
 * stats_dev: 8 DEVICE floats: [0..3] as gbnf_image_trainer_nll_step writes them; [4] G_nll in nats; [5] stats[0] - stats[4], the
 * reference's `nll` (:256), unscaled; [6] the row count of step 2 (the batch size when every image lies below the floor); [7] 0.
 * workspace: caller-owned DEVICE scratch of gbnf_image_boosted_step_workspace_bytes bytes -- the nll_step workspace, the fixed
 * component's forward workspace, its ldj and ll, the partial sums, each 256-byte aligned.  GBNF_ERR_INVALID (nothing launched):
 * everything gbnf_image_trainer_nll_step refuses, a null `fixed`, a `fixed` whose input shape differs from the trainer's, a short
 * workspace. */
int gbnf_image_boosted_step_workspace_bytes(const gbnf_image_flow* fixed, const gbnf_image_trainer* trainer, int64_t n,
                                            int64_t* bytes);
int gbnf_image_boosted_nll_step(const gbnf_image_flow* fixed, float g_floor, gbnf_image_trainer* trainer, const float* x,
                                const float* noise, int64_t n, float loss_scale, float* grads, float* exp_avg, float* exp_avg_sq,
                                const gbnf_opt_hyper* hyper, float* stats_dev, void* workspace, int64_t workspace_bytes,
                                void* stream);
/* The class-conditional form: gbnf_image_flow_forward_y of `fixed` in step 1, gbnf_image_trainer_nll_step_y in step 3; both must be
 * conditioned on the same number of classes (GBNF_ERR_INVALID otherwise; the plain call refuses conditioned ones).
 * stats_dev: 12 DEVICE floats: [0..7] as gbnf_image_trainer_nll_step_y writes them; [8] G_nll; [9] stats[0] - stats[8]; [10] the row
 * count of step 2; [11] 0 -- what the plain call keeps at [4..7]. */
int gbnf_image_boosted_step_workspace_bytes_y(const gbnf_image_flow* fixed, const gbnf_image_trainer* trainer, int64_t n,
                                              int64_t* bytes);
int gbnf_image_boosted_nll_step_y(const gbnf_image_flow* fixed, float g_floor, gbnf_image_trainer* trainer, const float* x,
                                  const float* noise, const float* y_dev, int64_t n, float loss_scale, float y_weight, float* grads,
                                  float* exp_avg, float* exp_avg_sq, const gbnf_opt_hyper* hyper, float* stats_dev, void* workspace,
                                  int64_t workspace_bytes, void* stream);

/* ---- drawing from the mixture ----------------------------------------------------------------------------------------------------
 * Replaces: BoostedFlow.decode (models/boosted_flow.py:209-218), which sends ALL rows of a call through ONE component drawn on the
 * host by _sample_component("1:c") (:61-96: torch.multinomial(rho[0:c] / sum, 1).item()) and says so itself ("rewrite this so that
 * samples can be taking from all components, not just many samples from a randomly chosen component") -- and what a user writes in
 * eager PyTorch to get samples of the density gbnf_mixture_log_prob evaluates: a per-row draw, a boolean-mask loop over the
 * components, a scatter back.  Every row gets a component of its OWN, the rows are partitioned by component on the device, and each
 * component's rows go through gbnf_flow_inverse as one contiguous batch: that call's math mode, repair pass and z -> x guard apply to
 * a segment exactly as to a caller's batch of the same rows, and no flow kernel knows about any of this.
 *
 * The draw is gbnf_resample_rows on w = rho_dev[0:n_used] and the CALLER's uniforms u (n DEVICE floats in [0,1)):
 *   cdf_c = sum_{k <= c} max(rho_k, 0) in double precision, in index order;  T = cdf_{n_used-1};
 *   comp[i] = the smallest c with (double)u[i] * T < cdf_c.
 * A component of zero weight is never drawn; out-of-contract u (>= 1, NaN) and T == 0 behave as documented there, so every comp[i]
 * lies in [0, n_used).  The partition is a stable counting sort without float arithmetic (per-chunk integer histograms, a
 * one-workgroup scan, ranks by wave ballot): comp, order and counts are bit-identical from run to run.
 *
 * Two phases, neither of which waits for the device (both can be captured): the segment sizes have to reach the HOST between them,
 * because gbnf_flow_inverse takes its row count by value -- the one host read of the path, where the reference has its .item().
 *
 * gbnf_mixture_sample_begin   the draw, the partition and the gather.  Outputs, all DEVICE memory:
 *     comp (n int32)        the component of row i;
 *     order (n int64)       position -> caller's row: the rows of component 0 in ascending caller index, then those of component 1, ...
 *                           (while the call runs, `order` also holds the draw's int64 result);
 *     counts_dev (n_used int64)  rows per component.
 *   z_or_null: (n,d) latent rows, copied into the workspace segment by segment; NULL skips that (the image path partitions with this
 *   call and runs its own inverses): d then only sizes the workspace, 1 will do.
 * gbnf_mixture_sample_finish  for every component with counts_host[c] > 0: gbnf_flow_inverse(flows[c]) on its segment; then the scatter,
 *   x[order[q]] / ldj[order[q]] = the sorted rows.  counts_host: the HOST copy of counts_dev; order: as begin left it; the SAME
 *   workspace, untouched in between; n_flows must equal begin's n_used (the first n_used handles): the workspace is laid out by it.
 *   x may be the buffer z was (the gather has consumed it in stream order); ldj_or_null NULL: no log|det dx/dz|.
 *
 * Segment c starts at row start_c of the sorted buffers, start_0 = 0, start_c = roundup64(start_{c-1} + counts[c-1]): a 256-byte
 * boundary for every d, what the flow kernels have always been handed.  Padding rows are never read back.
 * workspace: gbnf_mixture_sample_workspace_bytes(n_flows, n, d) of DEVICE memory, 256-byte aligned: with R = n + 64 n_flows rows and
 * B = ceil(n / 1024) chunks, in this order, each rounded up to 256 bytes:  sorted z (4 R d) | sorted x (4 R d) | sorted ldj (4 R) |
 * chunk histograms (8 B n_flows) | the draw's cdf (8 n_flows; later the segments' padding).
 * GBNF_ERR_INVALID (nothing launched): a null pointer (z_or_null / ldj_or_null excepted), n < 1, n_used < 1, n_flows < 1, d < 1,
 * counts_host that do not sum to n (or hold a negative entry), flows whose d differ, a short workspace.  GBNF_ERR_UNSUPPORTED: more
 * than 1024 components (the partition keeps one counter per component and wave in LDS). */
int gbnf_mixture_sample_workspace_bytes(int32_t n_flows, int64_t n, int32_t d, int64_t* bytes);
int gbnf_mixture_sample_begin(const float* rho_dev, int32_t n_used, const float* u, const float* z_or_null, int64_t n, int32_t d,
                              int32_t* comp, int64_t* order, int64_t* counts_dev, void* workspace, int64_t workspace_bytes,
                              void* stream);
int gbnf_mixture_sample_finish(gbnf_flow* const* flows, int32_t n_flows, const int64_t* counts_host, const int64_t* order, int64_t n,
                               float* x, float* ldj_or_null, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the validation pass ---------------------------------------------------------------------------------------------------------
 * Replaces: evaluate(model, data_loader, args) of both drivers -- density_experiment.py:544-603 (per batch component + 1 module
 * forwards for G, one more for g, then torch.cat over the whole set and .mean().item()) and image_experiment.py:296-337 (per batch
 * 3 C forwards of randomly drawn components and one .item()) -- by running sums that stay on the device across the batches of a
 * loader and are read once after the last one.
 *
 * The evaluation state: GBNF_EVAL_STATE_DOUBLES doubles of caller-owned DEVICE memory.  The caller zeroes it before the first batch
 * and reads it after the last; the library only ever ADDS to it:
 *   [0] rows seen                          [1] batches seen (calls with n >= 1)
 *   [2] sum G_ll     [3] sum g_ll          [4] sum (G_ll - g_ll)          [5] sum E_ll
 *   [6] [7] [8]  the sums over batches of the batch means of G_ll, g_ll, E_ll
 *   [9] rows where G_ll, g_ll or E_ll is not finite (they are still added: a NaN reaches the mean as it does in the reference)
 *   [10] sum over rows of w_c CE           [11] sum over batches of w_c (batch-mean CE)     [12] sum over rows of w_c [pred == label]
 *   [13..15] 0 (reserved)
 * with, per row i of a (n_used, n) table ll of per-component log-likelihoods,
 *   G_ll[i]  the recursion of density_experiment.py:561-573 over rows 0 .. n_used - 1: the float32 operations of gbnf_mixture_lse,
 *            bit for bit;
 *   g_ll[i]  ll[component][i];  G_ll - g_ll is formed in float32, as the reference forms g_nll - G_nll (:588);
 *   E_ll[i]  sum_c w_c ll[c][i] in double, w_c = rho[c] / sum_{k < n_used} rho[k]: the exact expectation of what the image driver
 *            estimates with 3 C draws of components="1:c" (every product and sum rounded on its own, in index order).
 * So  nll = -[2] / [0],  g_nll = -[3] / [0],  ratio = [4] / [0]  (:582-588), and  -[6] / [1]  is the mean of batch means of :594.
 * All sums run in double: per workgroup in an LDS tree (workgroup b of a grid of min(ceil(n / 1024), 256) takes rows
 * b * 256 + t, stepping by the grid), then over the workgroups' partial sums in index order.  No atomics: the same calls in the
 * same order give the same bits.  No host read, no synchronisation, no allocation.
 *
 * gbnf_eval_workspace_bytes: the size of the partial-sum scratch (DEVICE memory, 256-byte aligned) of the two accumulate calls.
 * gbnf_eval_accumulate: two launches (the partial sums, a one-workgroup finalise that adds into state_dev) on a table with row
 *   stride ll_row_stride floats; G_out_or_null: G_ll (n floats).  n == 0: GBNF_OK, nothing added (`batches` neither).
 *   GBNF_ERR_INVALID before any launch: a null ll / rho_dev / state_dev / workspace, n < 0, n_used < 1, component outside
 *   [0, n_used), ll_row_stride < n, a short workspace.
 * gbnf_eval_accumulate_class_loss: component c's share of the class loss of class-conditional image models into entries 10 - 12
 *   (rows and batches are not touched: the table's call counts them).  y_logits (n, Y), y (n, Y) DEVICE, 1 <= Y <= 256:
 *   CE_i = LSE(logits_i) - logits_i[first largest entry of y_i] -- F.cross_entropy(y_logits, argmax(y)), image_experiment.py:236 --
 *   in double; the prediction is the first largest logit, and a NaN never wins.  The refusals of gbnf_eval_accumulate, and Y outside
 *   [1, 256], c outside [0, n_used).
 * Two calls on one workspace must not run concurrently. */
#define GBNF_EVAL_STATE_DOUBLES 16
int gbnf_eval_workspace_bytes(int64_t n, int64_t* bytes);
int gbnf_eval_accumulate(const float* ll, int64_t ll_row_stride, int32_t n_used, int64_t n, const float* rho_dev, int32_t component,
                         float* G_out_or_null, double* state_dev, void* workspace, int64_t workspace_bytes, void* stream);
int gbnf_eval_accumulate_class_loss(const float* y_logits, const float* y, int64_t n, int32_t Y, const float* rho_dev, int32_t n_used,
                                    int32_t c, double* state_dev, void* workspace, int64_t workspace_bytes, void* stream);
/* Replaces: one batch of density_experiment.py:549-579 in one call: gbnf_mixture_component_log_prob(mix, x, n, 0, n_used,
 * ll_workspace) -- ONE flow launch for all components; the reference's extra forward of components="c" is row `component` of that
 * table and is not run again --, then gbnf_eval_accumulate on it.  ll_workspace: (n_used, n) DEVICE floats, also an output;
 * workspace: gbnf_eval_workspace_bytes.  Refused before any launch: everything gbnf_eval_accumulate refuses, a null mix or x,
 * n_used beyond the mixture's components. */
int gbnf_mixture_evaluate(const gbnf_mixture* mix, const float* x, int64_t n, int32_t n_used, int32_t component, const float* rho_dev,
                          float* ll_workspace, float* G_out_or_null, double* state_dev, void* workspace, int64_t workspace_bytes,
                          void* stream);
/* Replaces: one batch of image_experiment.py:302-334, built as gbnf_image_mixture_rho_step is: the forwards of flows[0 .. n_used - 1]
 * one after the other on the caller's stream (the same noise for all) into ll_workspace ((n_used, n) DEVICE floats, also an output),
 * then gbnf_eval_accumulate on that table.  With D = C H W pixels, the mixture's bits per dimension are -[2] / ([0] ln2 D) and the
 * expectation of the reference's avg_loss is -[8] / ([1] ln2 D) (+ y_weight [11] / [1] for the _y call).
 * workspace: gbnf_image_mixture_evaluate_workspace_bytes(flows, n_used, n) bytes -- the largest gbnf_image_flow_workspace_bytes of the
 * handles, the call's ldj accumulator, n Y floats of logits (Y: the classes of flows[0], 0 for a plain model), the partial sums, each
 * 256-byte aligned.  GBNF_ERR_INVALID (nothing launched): a null flows / x / rho_dev / ll_workspace / state_dev / workspace or a null
 * entry of flows, n < 1, n_used < 1, component outside [0, n_used), handles whose input shape differs, a class-conditional handle
 * (it needs y: the _y call), a short workspace.
 * gbnf_image_mixture_evaluate_y: the same over class-conditional components with y (n, Y) DEVICE: every forward is
 * gbnf_image_flow_forward_y under its prior of each row's y, with the logits into the workspace, and
 * gbnf_eval_accumulate_class_loss follows each component.  Every handle must be conditioned on the same Y and have a class head: a
 * plain handle, a second class count, a handle without a head or a null y is GBNF_ERR_INVALID before the first launch. */
int gbnf_image_mixture_evaluate_workspace_bytes(const gbnf_image_flow* const* flows, int32_t n_flows, int64_t n, int64_t* bytes);
int gbnf_image_mixture_evaluate(const gbnf_image_flow* const* flows, int32_t n_used, int32_t component, const float* x,
                                const float* noise, int64_t n, const float* rho_dev, float* ll_workspace, float* G_out_or_null,
                                double* state_dev, void* workspace, int64_t workspace_bytes, void* stream);
int gbnf_image_mixture_evaluate_y(const gbnf_image_flow* const* flows, int32_t n_used, int32_t component, const float* x,
                                  const float* noise, const float* y_dev, int64_t n, const float* rho_dev, float* ll_workspace,
                                  float* G_out_or_null, double* state_dev, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- all mixture weights at once: EM over a cached table of component log-likelihoods ---------------------------------------------
 * No reference counterpart.  Supersedes update_rho (models/boosted_flow.py:141-207; gbnf_mixture_rho_step here), which moves one
 * rho[component] at a time along mean(G_ll - g_ll) and never revisits earlier weights.  The recursion of gbnf_mixture_lse is the
 * plain normalised mixture G = LSE_c(log w_c + ll_c) with w_c = rho_c / sum_{k < C} rho_k; with the components fixed, the weights
 * that maximise the mean of G over a set of rows are a concave problem, and EM never decreases that mean.
 *
 * gbnf_weights_em: ll is a (C, n) DEVICE table with row stride ll_row_stride >= n floats (what
 * gbnf_mixture_component_log_prob[_strided] or an image call wrote).  Everything below is in double:
 *   w^(0)_c = rho_dev[c] / sum_k rho_dev[k], from the float32 entries, the sum in index order;
 *   evaluation t = 0 .. max_iters:  per row  G_i = LSE_c(log w^(t)_c + ll[c][i])  (the largest term subtracted first),
 *     L_t = (1 / N_used) sum_i G_i,   S_c = sum_i exp(log w^(t)_c + ll[c][i] - G_i);
 *   stop when t >= 1, tol > 0 and |L_t - L_{t-1}| <= tol (converged; the weights stay w^(t)), or when t == max_iters;
 *   otherwise w^(t+1)_c = S_c / N_used.   tol <= 0: no convergence test, exactly max_iters updates.
 * So L at the final weights is always evaluated.  A row is excluded, and counted, when it holds a NaN or +inf or when all its
 * entries are -inf; single -inf entries are legal and give r = 0 as in gbnf_mixture_responsibilities.  w_c = 0 is a legal fixed
 * point (log w = -inf, no NaN); a row whose every finite entry belongs to a component of weight 0 has G = -inf and adds no r.
 * Bad start -- N_used == 0, an entry of rho_dev[0..C) that is not finite or < 0, or a sum <= 0 --: [7] is set, no update is made,
 * [2] and [3] are counted, [4] and [5] are what one evaluation at rho_dev[c] / sum gives (NaN without a usable row or weight) and
 * [8..) hold those quotients as formed.
 * state_dev (GBNF_WEIGHTS_STATE_DOUBLES doubles, DEVICE) is overwritten, nothing is added to it:
 *   [0] updates applied   [1] converged (0 / 1)   [2] rows used   [3] rows excluded   [4] L_0   [5] L at the final weights
 *   [6] the last |L_t - L_{t-1}| (0 after a single evaluation)   [7] bad_start (0 / 1)   [8 .. 8 + C) the final weights
 * Sums: across the 64 rows of a wave in a fixed tree, over the rows a wave walks, over the 4 waves, then over the workgroups'
 * partial sums in index order (a grid of min(max(ceil(n / 1024), 1), 256) workgroups of 256 rows, stepping by the grid).  No
 * atomics: the same call gives the same bits.  max_iters + 2 launches are enqueued (evaluation k re-adds the partial sums of
 * evaluation k - 1 in every workgroup, through two alternating partial buffers; the last launch only finalises); "stopped" is a
 * DEVICE word, and every launch behind the stopping evaluation returns at once.  No host read, no synchronisation, no allocation.
 * workspace: gbnf_weights_em_workspace_bytes(C, n) bytes of DEVICE memory, 256-byte aligned; two calls on one workspace must not
 * run concurrently.  GBNF_ERR_INVALID before any launch: a null ll / rho_dev / state_dev / workspace, n < 0 (n == 0 is legal: a bad
 * start), C outside [1, GBNF_WEIGHTS_MAX_COMPONENTS], ll_row_stride < n, max_iters < 0, a NaN tol, a short workspace.
 *
 * gbnf_weights_to_rho: one launch.  rho_dev[c] = clamp(w_c * S, rho_min, rho_max) for c < C, with w_c = state_dev[8 + c] and S the
 * sum of the old rho_dev[0..C) (double, index order; the product is rounded to float32, then clamped): the total is kept, so
 * entries at and beyond C keep their relative standing.  In place.  Writes nothing when bad_start is set.  ADDS twice the number
 * of clamped entries into state_dev[7], so that word reads bad_start + 2 * clamped (hence state_dev is not const).  The reference's
 * range is [0.01, 100].  GBNF_ERR_INVALID: a null pointer, C outside [1, 64], rho_min > rho_max or a NaN bound. */
#define GBNF_WEIGHTS_MAX_COMPONENTS 64
#define GBNF_WEIGHTS_STATE_DOUBLES (8 + GBNF_WEIGHTS_MAX_COMPONENTS)
int gbnf_weights_em_workspace_bytes(int32_t n_components, int64_t n, int64_t* bytes);
int gbnf_weights_em(const float* ll, int64_t ll_row_stride, int32_t n_components, int64_t n, const float* rho_dev, int32_t max_iters,
                    double tol, double* state_dev, void* workspace, int64_t workspace_bytes, void* stream);
int gbnf_weights_to_rho(double* state_dev, int32_t n_components, float rho_min, float rho_max, float* rho_dev, void* stream);

/* ---- One joint likelihood step of the whole tabular mixture: every component moves on the mixture NLL ----
 * No reference counterpart: the reference trains one component at a time on its own NLL (density_experiment.py:340-374, the second
 * pass `all_trained` included).  Replaces the eager composition a joint fine-tune needs -- C recorded forwards, a logsumexp, C
 * backward passes, clip_grad_norm_(model.parameters()), C optimiser steps -- for the trainers of components 0 .. n_components - 1:
 *   L = -1/n sum_i G_i,   G_i = LSE_c(log_w[c] + ll_c(x_i)),   dL/dtheta_c = -1/n sum_i r_ic d ll_c(x_i) / dtheta_c,
 * so component c's backward runs unchanged on the seeds g_z = (r_c / n) z_c, g_ldj = -r_c / n.  log_w (C,) DEVICE is held fixed
 * (gbnf_mixture_score's closed form, or any other weights).  The call launches on `stream` in this order and never reads the
 * device, synchronises or allocates:
 *   1. per component, in order: gbnf_trainer_forward on the live parameters into the component's OWN trace, then
 *      ll_c = log N(z_c; 0, I) + ldj_c (gbnf_score_seed's per-row double sum, 2 pi term included);
 *   2. gbnf_mixture_responsibilities -> r (C, n), G (n,), copied to r_or_null / G_or_null (DEVICE) when given;
 *   3. per-workgroup double partial sums of sum_i G_i and of sum_i r_ci for every c (at most 256 workgroups, their number a
 *      function of n alone), re-added in step 5 in a fixed order; no float atomics;
 *   4. per component, in order: the seed with inv_n = 1.0f / n (s_i = r_c[i] * inv_n, g_z[i][j] = s_i * z_c[i][j], g_ldj[i] = -s_i),
 *      grads[c] zeroed, gbnf_trainer_backward with the component's trace (no g_x), the squared-norm partials of grads[c];
 *   5. one workgroup re-adds everything in component order and partial order, in double: nll = -sum G / n,
 *      rbar_c = sum_i r_ci / n, norm_c = ||grads[c]||_2, total = sqrt(sum_c norm_c^2);
 *   6. per component gbnf_trainer_apply_update's update kernel with the ONE clip coefficient min(1, max_grad_norm / (total + 1e-6))
 *      (1 without clipping), as clip_grad_norm_ over all components' parameters gives.
 * grads / exp_avg / exp_avg_sq: host arrays of C DEVICE buffers, each of its trainer's gbnf_trainer_grad_floats floats (entries of
 * exp_avg / exp_avg_sq may be NULL for SGD); grads[c] holds component c's unclipped gradient afterwards.  hypers: a host array of C
 * structs.  kind and max_grad_norm must agree across it; lr, weight_decay, the betas, eps and step are per component (components
 * boosted one after the other sit at different AdamW steps); a component with lr = 0 keeps its parameters bit for bit while its
 * moments move; bn_momentum is ignored (the step runs on the running statistics and leaves them alone).
 * stats_dev: 4 + 2 C floats of DEVICE memory: [0] nll, [1] total gradient norm, [2] clip coefficient, [3] 0, [4 + c] rbar_c (the EM
 * update of the weights on this batch), [4 + C + c] norm_c.
 * A non-finite G row is not masked: it reaches [0] and the gradients exactly as a non-finite z does in gbnf_trainer_nll_step.
 * With C = 1 and log_w = 0, r is exactly 1 and the parameters, moments and grads[0] are those of gbnf_trainer_nll_step bit for bit
 * on a deterministic trainer (nll agrees to rounding: f32 G summed here, f64 terms there).
 * workspace: gbnf_mixture_step_workspace_bytes of DEVICE memory, 256-byte aligned: per component z (n, d) and a trace of
 * gbnf_trainer_trace_floats -- C traces, not one: a single forward per component is bought with about 20 KB per sample and
 * component for MINIBOONE K = 5, depth 1 -- then ldj, ll (C, n), r (C, n), G, ONE g_z / g_ldj and ONE backward workspace (the
 * largest gbnf_trainer_workspace_bytes) reused across components, and the partial sums.  The size depends on the trainers'
 * deterministic mode as gbnf_trainer_workspace_bytes does.
 * With every trainer in deterministic mode (gbnf_trainer_set_deterministic) everything the call writes -- the parameters, the
 * moments, grads, stats_dev, G and r -- is bit-identical from run to run.
 * Refused with nothing launched -- GBNF_ERR_INVALID: a null array, a null entry of trainers or grads, a null log_w / x / stats_dev /
 * workspace, n_components outside [1, GBNF_WEIGHTS_MAX_COMPONENTS], n < 1, the same trainer twice, trainers of different d, what
 * gbnf_trainer_apply_update refuses of any hypers[c], differing kind or max_grad_norm, a short workspace; GBNF_ERR_UNSUPPORTED: a
 * trainer in batch-statistics mode (gbnf_trainer_set_batch_stats(0) first), and gbnf_trainer_backward's deterministic-mode refusals
 * for any trainer.  gbnf_mixture_step_workspace_bytes refuses the same handle array, a null bytes and n < 1. */
int gbnf_mixture_step_workspace_bytes(gbnf_trainer* const* trainers, int32_t n_components, int64_t n, int64_t* bytes);
int gbnf_mixture_nll_step(gbnf_trainer* const* trainers, int32_t n_components, const float* log_w, const float* x, int64_t n,
                          float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const gbnf_opt_hyper* hypers,
                          float* stats_dev, float* G_or_null, float* r_or_null, void* workspace, int64_t workspace_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GBNF_H_ */
