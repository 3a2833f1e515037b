// gbnf_image_train.hip -- training path of ONE image Glow component (gbnf_image_trainer_*): the forward on the caller's LIVE device
// parameters and its backward pass, exact f32.
//
//   pack      ONE launch re-derives, from the live parameters, the lane-order tiles img_conv_kernel reads ([OT][taps][KC][64][4], the
//             ActNorm2d / Conv2dZeros scales folded, a step's ActNorm2d + 1x1 collapsed into W_eff = W_perm . diag(exp(logs)),
//             b_eff = W_eff . bias) and a second, transposed and tap-flipped set: the convolution the data gradient is.
//   forward   the exact-f32 launch sequence of the evaluation path (gbnf_image.hip) on those tiles.  The trace IS the state storage:
//             per level the level's input, and per step the post-mix state P_k (the coupling's input) and the step's output O_k (the
//             next mix's input, the last one the Split2d's input).  Hidden activations are not kept.
//   backward  step by step from the top: the coupling net's activations are recomputed into the workspace (3x3 -> HBM -> 1x1 -> HBM),
//             an elementwise kernel turns the output gradient into the net's (the log-det term of g_ldj folded in), and every
//             convolution gives a weight gradient (img_train_wgrad_kernel, below) and a data gradient (img_conv_kernel on the
//             transposed tiles: the adjoint of a stride-1 'same' convolution is one; its Hv / Wv masking keeps the outside of the map
//             zero as the forward does).  gbnf_image_trainer_backward_x carries the state gradient through the first step's mix as well
//             and on to the image (img_pre_adjoint_kernel, gbnf_image_score.hip); without `grads` it skips every weight-gradient launch.
//   unfold   ONE launch maps (dW', db') of the folded convolutions and (dW_eff, db_eff) of the mixes to the descriptor's arrays.
//   init      gbnf_image_trainer_actnorm_init: the data-dependent ActNorm2d initialisation of every layer in ONE walk of the forward.
//             At a layer to initialise: (a coupling-net layer: its convolution once on identity tiles, store epilogue) -> per-channel
//             sums and centred squares over chunks of images in f64 (img_train_an_stats_kernel, grid chunks x channels) -> the finish
//             launch adds the chunks in order and writes bias / logs into the live tensors -> the pack kernel on that one entry.
//
// Weight gradient: dW'[o][i][tap] = sum_{n,p} G[o][n,p] A[i][n,p+tap] on v_mfma_f32_16x16x4_f32, contracting over pixels.  A workgroup
// owns a block of (output tile, input tile) pairs of dW' and a slice of the (image, strip) items: per item it stages the gradient strip
// and the padded input strip in LDS (a tap is an address offset, as in the forward), accumulates in registers over its whole slice and
// flushes ONCE with float atomics (as the tabular wgrad_kernel does); db' (the column sums of G) rides along in the blocks of input
// block 0.  Blocks x slices is a trade: a block re-reads its operands from L2 once per block of the other side, a slice adds one
// flush of the block; the launch gives a slice at least WGRAD_ITEMS items (measured per shape) and makes at
// most about 1024 workgroups.
//
// Deterministic mode (gbnf_image_trainer_set_deterministic): the slices STORE their blocks to per-slice partials in the workspace
// (img_train_wgrad_det_kernel) and img_train_wgrad_reduce_kernel adds them in slice order; the coupling / Split2d epilogues of the
// forward store per-wave log-det slots that img_ldj_reduce_kernel (gbnf_image.hip) adds in slot order.  Nothing else in the step adds
// floats in an unordered way.
//
// Reference semantics: as gbnf_image.hip (models/glow.py:92-110, 317-342; models/layers.py:488-533, 577-630, 685-705, 751-796).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/gbnf.h"
#include "gbnf_internal.h"
#include "gbnf_image_net.h"
#include "gbnf_image_train.h"

namespace gbnf {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int TR_R = 4;            // rows of a strip (IMG_R of gbnf_image.hip)
constexpr int WGRAD_ITEMS[3] = {6, 4, 2};     // least (image, strip) items per weight-gradient workgroup: first 3x3, last 3x3, 1x1 (launch_wgrad)

__device__ __forceinline__ float tconv_value(const TConv& e, int co, int ci, int tap) {
  const int taps = e.ks * e.ks;
  if (e.mix) return e.w[(size_t)co * e.cin + ci] * expf(e.an_logs[ci]);
  const float s = (e.an_logs ? e.an_logs[co] : 0.0f) + (e.logs ? 3.0f * e.logs[co] : 0.0f);
  return e.w[((size_t)co * e.cin + ci) * taps + tap] * expf(s);
}

// ---- pack: grid (blocks, entries) ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) img_train_pack_kernel(const TConv* __restrict__ table, float* __restrict__ blob) {
  const TConv e = table[blockIdx.y];
  const int taps = e.ks * e.ks;
  const int OT = (e.cout + 15) >> 4, KC = (e.cin + 15) >> 4;
  const int64_t nf = (int64_t)OT * taps * KC * 256;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < nf; idx += stride) {
    const int r = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    int64_t rest = idx >> 8;
    const int c = (int)(rest % KC); rest /= KC;
    const int tap = (int)(rest % taps), o = (int)(rest / taps);
    // forward tiles: rows = output channels, k = input channels
    {
      const int co = 16 * o + (lane & 15), ci = 16 * c + 4 * (lane >> 4) + r;
      blob[e.fwd_off + idx] = (co < e.cout && ci < e.cin) ? tconv_value(e, co, ci, tap) : 0.0f;
    }
  }
  // adjoint tiles: rows = INPUT channels, k = OUTPUT channels, taps mirrored
  const int64_t nb = (int64_t)KC * taps * OT * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < nb; idx += stride) {
    const int r = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    int64_t rest = idx >> 8;
    const int c = (int)(rest % OT); rest /= OT;
    const int tap = (int)(rest % taps), o = (int)(rest / taps);
    const int ci = 16 * o + (lane & 15), co = 16 * c + 4 * (lane >> 4) + r;
    blob[e.bwd_off + idx] = (co < e.cout && ci < e.cin) ? tconv_value(e, co, ci, taps - 1 - tap) : 0.0f;
  }
  for (int co = blockIdx.x * 256 + threadIdx.x; co < OT * 16; co += (int)stride) {
    float b = 0.0f;
    if (co < e.cout) {
      if (e.mix) {
        for (int m = 0; m < e.cin; ++m) b = fmaf(tconv_value(e, co, m, 0), e.an_bias[m], b);
      } else {
        const float s = (e.an_logs ? e.an_logs[co] : 0.0f) + (e.logs ? 3.0f * e.logs[co] : 0.0f);
        b = ((e.bias ? e.bias[co] : 0.0f) + (e.an_bias ? e.an_bias[co] : 0.0f)) * expf(s);
      }
    }
    blob[e.b_off + co] = b;
  }
}

// ldj[i] += sum over the mixes of hw * sum(logs): the ActNorm2d log-determinants of the steps (models/layers.py:506-508)
__global__ void __launch_bounds__(256) img_train_ldconst_kernel(const TConv* __restrict__ table, int n_entries, float* __restrict__ ldj, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float acc = 0.0f;
  for (int k = 0; k < n_entries; ++k) {
    if (!table[k].mix) continue;
    float s = 0.0f;
    for (int c = 0; c < table[k].cin; ++c) s += table[k].an_logs[c];
    acc = fmaf(table[k].hw, s, acc);
  }
  ldj[i] += acc;
}

// ---- elementwise backward -------------------------------------------------------------------------------------------
// Coupling (models/glow.py:326-338).  h (n, cout, H, W): the net's output on entry ("cross" rows: shift_j, raw_j), its gradient on
// exit.  z2: the coupled half BEFORE the coupling (the trace's P_k), gy: the gradient of the coupled half, replaced by z2's.
template <bool AFFINE>
__global__ void __launch_bounds__(256) img_train_couple_bwd_kernel(float* __restrict__ h, int64_t h_img, const float* __restrict__ z2, int64_t z2_img,
                                                                   float* __restrict__ gy, int64_t gy_img, const float* __restrict__ g_ldj, int c2,
                                                                   int H, int W, int Hv, int Wv, int64_t total /* n c2 H W */) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int HW = H * W;
  const int64_t n = t / ((int64_t)c2 * HW);
  const int rem = (int)(t - n * (int64_t)c2 * HW), j = rem / HW, pix = rem - j * HW;
  const bool valid = pix / W < Hv && pix % W < Wv;
  float* gp = gy + n * gy_img + (int64_t)j * HW + pix;
  const float g = *gp;
  if (AFFINE) {
    float* hp = h + n * h_img + (int64_t)(2 * j) * HW + pix;
    const float shift = hp[0], raw = hp[HW];
    const float sc = 1.0f / (1.0f + expf(-(raw + 2.0f)));
    const float zz = z2[n * z2_img + (int64_t)j * HW + pix] + shift;
    const float gz = g * sc;
    // y = (z2 + shift) sc, ldj += log sc;  d sc / d raw = sc (1 - sc), d log sc / d raw = 1 - sc
    hp[0] = valid ? gz : 0.0f;
    hp[HW] = valid ? (g * zz * sc + g_ldj[n]) * (1.0f - sc) : 0.0f;
    *gp = valid ? gz : 0.0f;
  } else {
    h[n * h_img + (int64_t)j * HW + pix] = valid ? g : 0.0f;
  }
}

// Split2d (models/layers.py:685-705): ldj += sum -0.5 (lv + (z2 - mean)^2 exp(-lv)).  h: (mean_j, lv_j) cross rows on entry, their
// gradients on exit; gz2 (the dropped half's gradient) is WRITTEN.
__global__ void __launch_bounds__(256) img_train_split_bwd_kernel(float* __restrict__ h, int64_t h_img, const float* __restrict__ z2, int64_t z2_img,
                                                                  float* __restrict__ gz2, int64_t gz2_img, const float* __restrict__ g_ldj, int c2,
                                                                  int H, int W, int Hv, int Wv, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int HW = H * W;
  const int64_t n = t / ((int64_t)c2 * HW);
  const int rem = (int)(t - n * (int64_t)c2 * HW), j = rem / HW, pix = rem - j * HW;
  const bool valid = pix / W < Hv && pix % W < Wv;
  float* hp = h + n * h_img + (int64_t)(2 * j) * HW + pix;
  const float mean = hp[0], lv = hp[HW];
  const float d = z2[n * z2_img + (int64_t)j * HW + pix] - mean, e = expf(-lv), g = g_ldj[n];
  hp[0] = valid ? g * d * e : 0.0f;
  hp[HW] = valid ? g * (0.5f * d * d * e - 0.5f) : 0.0f;
  gz2[n * gz2_img + (int64_t)j * HW + pix] = valid ? -g * d * e : 0.0f;
}

// g *= (a > 0): the ReLU in front of a convolution, on the data gradient that convolution's adjoint left
__global__ void __launch_bounds__(256) img_train_relu_mask_kernel(float* __restrict__ g, const float* __restrict__ a, int64_t total4) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total4) return;
  f32x4 gv = reinterpret_cast<f32x4*>(g)[t];
  const f32x4 av = reinterpret_cast<const f32x4*>(a)[t];
#pragma unroll
  for (int r = 0; r < 4; ++r) gv[r] = av[r] > 0.0f ? gv[r] : 0.0f;
  reinterpret_cast<f32x4*>(g)[t] = gv;
}

// ---- weight gradient -----------------------------------------------------------------------------------------------
struct WgradLaunch {
  const float* a; int64_t a_img;     // the convolution's input (n, cin.., H, W), first input channel of image 0
  const float* g; int64_t g_img;     // the gradient of its output (n, cout.., H, W); zero outside the map proper
  float* dw;                         // [cout][cin][taps], accumulated with atomics
  float* db;                         // [cout]
  int cin, cout, H, Hv, n_strips, n_items;      // n_items = n * n_strips
  int obt, ibt, n_ib;                // output / input tiles of a workgroup's block, input blocks (blockIdx.x = ob * n_ib + ib)
};

__device__ __forceinline__ f32x4 tr_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// The compiler pads the MFMA result hazard along fall-through paths only (tools/isa_hazard_lint.py; img_drain of gbnf_image.hip exists
// for the same reason): the accumulators are read behind wave-uniform branches here, so they are drained explicitly first.
__device__ __forceinline__ void tr_drain(f32x4& c) { asm volatile("s_nop 7\n\ts_nop 7" : "+a"(c)); }

// PT: pixel tiles of a strip (4: 16-wide maps, 2: 8-wide); KS: 1 | 3.  NP (block pairs per wave) = 2 (3x3) | 4 (1x1).
template <int PT, int KS>
__global__ void __launch_bounds__(256) img_train_wgrad_kernel(const WgradLaunch p) {
#define GBNF_IWG_DET 0
#include "gbnf_image_wgrad_kernel.inc"
#undef GBNF_IWG_DET
}

// Deterministic mode: the same text a second time (a shared `template <bool DET>` body is not guaranteed to leave the default
// kernel's code alone), the flush a plain store to slice blockIdx.y's copy of the convolution's (dW', db') region.  p.dw / p.db:
// slice 0's copy; part_stride = cout cin taps + cout floats.  Every valid entry is stored by exactly one workgroup of every slice:
// the blocks tile the (output tile, input tile) pairs, a block's pairs are dealt to its waves completely (npairs <= 4 NP).
template <int PT, int KS>
__global__ void __launch_bounds__(256) img_train_wgrad_det_kernel(const WgradLaunch p, const int64_t part_stride) {
#define GBNF_IWG_DET 1
#include "gbnf_image_wgrad_kernel.inc"
#undef GBNF_IWG_DET
}

// dst[e] = part[0][e] + part[1][e] + ... in slice order; one thread per entry of the convolution's (dW', db') region.  Eight loads
// in flight, added in order.
__global__ void __launch_bounds__(256) img_train_wgrad_reduce_kernel(const float* __restrict__ part, int64_t part_stride, int slices,
                                                                     float* __restrict__ dst) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= part_stride) return;
  const float* src = part + e;
  float acc = 0.0f;
  int y = 0;
  for (; y + 8 <= slices; y += 8) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = src[(int64_t)(y + q) * part_stride];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc += v[q];
  }
  for (; y < slices; ++y) acc += src[(int64_t)y * part_stride];
  dst[e] = acc;
}

// ---- data-dependent ActNorm2d initialisation (gbnf_image_trainer_actnorm_init; models/layers.py:473-486) ---------------------
// Per-channel statistics over (n, the map proper) of a tensor t (n, C.., H, W), H x W = 16 x 16 | 8 x 8 storage: grid (chunks,
// channels), a chunk = `per_chunk` consecutive images.  A wave reads whole channel maps, one float4 per lane: one 16 x 16 map or
// four 8 x 8 maps (of four images) at a time, the four waves of the workgroup on consecutive groups of images.  Only rows < Hv,
// columns < Wv count; nothing outside them is used.  Two passes, as the reference: PASS 0 the sums, PASS 1 the squares centred on
// the mean every workgroup re-adds from PASS 0's partials.  All sums are doubles in a fixed order -- a lane over its images, the
// xor tree of the wave, the four waves in order, the chunks in order (the consumer) --, every partial is a plain store.
constexpr int AN_MAX_CHUNKS = 64;
struct AnStats {
  const float* t; int64_t t_img;     // first channel of image 0, floats between images
  int64_t n;
  int HW, W, Hv, Wv;
  int per_chunk, chunks;
  double* sum;                       // [channel][chunk]: PASS 0 writes, PASS 1 reads
  double* sq;                        // [channel][chunk]: PASS 1 writes
};

template <int PASS>
__global__ void __launch_bounds__(256) img_train_an_stats_kernel(const AnStats p) {
  __shared__ double red[4];
  const int chunk = blockIdx.x, c = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lpm = p.HW >> 2, mpw = 64 / lpm;                 // lanes of a map (64 | 16), maps a wave reads at a time (1 | 4)
  const int sub = lane / lpm, e = (lane - sub * lpm) * 4;    // this lane's map of the group, its first element there
  const int y = e / p.W, x0 = e - y * p.W;                   // (W is a multiple of 4: the four elements share a row)
  double mean = 0.0;
  if (PASS == 1) {
    double s = 0.0;
    for (int k = 0; k < p.chunks; ++k) s += p.sum[(int64_t)c * p.chunks + k];
    mean = s / ((double)p.n * p.Hv * p.Wv);
  }
  const int64_t first = (int64_t)chunk * p.per_chunk, last = first + p.per_chunk < p.n ? first + p.per_chunk : p.n;
  double acc = 0.0;
  if (y < p.Hv) {
    for (int64_t i = first + wave * mpw + sub; i < last; i += 4 * mpw) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p.t + i * p.t_img + (int64_t)c * p.HW + e);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (x0 + r < p.Wv) {
          const double d = (double)v[r] - mean;              // (PASS 0: mean = 0)
          acc += PASS == 0 ? d : d * d;
        }
      }
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) (PASS == 0 ? p.sum : p.sq)[(int64_t)c * p.chunks + chunk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one thread per channel: the chunks' partials in chunk order -> bias = -mean, logs = log(scale / (sqrt(var) + 1e-6)) into the live tensors
__global__ void __launch_bounds__(256) img_train_an_finish_kernel(const double* __restrict__ sum, const double* __restrict__ sq, int chunks, int C,
                                                                  double total, float scale, float* __restrict__ bias, float* __restrict__ logs) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int k = 0; k < chunks; ++k) s += sum[(int64_t)c * chunks + k];
  for (int k = 0; k < chunks; ++k) q += sq[(int64_t)c * chunks + k];
  const double mean = s / total, var = q / total;
  bias[c] = (float)-mean;
  logs[c] = (float)log((double)scale / (sqrt(var) + 1e-6));
}

// ---- unfold: grid (512 / 4, entries); one WAVE per output channel (mix: per input channel), lanes along the row: coalesced ------
__device__ __forceinline__ float tr_wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__global__ void __launch_bounds__(256) img_train_unfold_kernel(const TConv* __restrict__ table, const float* __restrict__ gscr,
                                                               const float* __restrict__ g_ldj, int64_t n, float* __restrict__ grads) {
  const TConv e = table[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);         // (wave-uniform)
  const float* gw = gscr + e.gw_off;
  const float* gb = gscr + e.gb_off;
  if (!e.mix) {
    if (o >= e.cout) return;
    const int row = e.cin * e.ks * e.ks;
    const float s = (e.an_logs ? e.an_logs[o] : 0.0f) + (e.logs ? 3.0f * e.logs[o] : 0.0f), es = expf(s);
    float dot = 0.0f;
    for (int t = lane; t < row; t += 64) {
      const float v = gw[(int64_t)o * row + t];
      dot = fmaf(v, e.w[(int64_t)o * row + t], dot);
      grads[e.g_w + (int64_t)o * row + t] += es * v;                        // W' = e^s W
    }
    dot = tr_wave_sum(dot);
    if (lane != 0) return;
    const float gbo = gb[o];
    const float bsum = (e.bias ? e.bias[o] : 0.0f) + (e.an_bias ? e.an_bias[o] : 0.0f);
    const float dlog = es * (dot + gbo * bsum);                           // sum gW'[o,.] W'[o,.] + gb'[o] b'[o]
    if (e.g_bias >= 0) grads[e.g_bias + o] += es * gbo;
    if (e.g_an_bias >= 0) grads[e.g_an_bias + o] += es * gbo;
    if (e.g_an_logs >= 0) grads[e.g_an_logs + o] += dlog;
    if (e.g_logs >= 0) grads[e.g_logs + o] += 3.0f * dlog;
  } else {
    const int C = e.cin, j = o;                              // C <= 64: lane r holds row r of column j
    if (j >= C) return;
    const float el = expf(e.an_logs[j]);
    float s_ww = 0.0f, s_bw = 0.0f;
    if (lane < C) {
      const int r = lane;
      const float gv = gw[(int64_t)r * C + j], weff = e.w[(int64_t)r * C + j] * el;
      s_ww = gv * weff;
      s_bw = gb[r] * weff;
      // W_eff = W_perm diag(e^logs) and b_eff = W_eff bias: out_r = sum_j W_perm[r][j] e^logs[j] (x_j + bias[j])
      if (e.g_w >= 0) grads[e.g_w + (int64_t)r * C + j] += (gv + gb[r] * e.an_bias[j]) * el;
    }
    float sl = 0.0f;
    if (g_ldj != nullptr)
      for (int64_t k = lane; k < n; k += 64) sl += g_ldj[k];
    s_ww = tr_wave_sum(s_ww); s_bw = tr_wave_sum(s_bw); sl = tr_wave_sum(sl);
    if (lane != 0) return;
    grads[e.g_an_logs + j] += s_ww + s_bw * e.an_bias[j] + e.hw * sl;
    grads[e.g_an_bias + j] += s_bw;
  }
}

}  // namespace gbnf

using namespace gbnf;

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
namespace {

int64_t tile_floats(int cout, int cin, int ks) { return (int64_t)((cout + 15) / 16) * ((cin + 15) / 16) * ks * ks * 256; }

// workspace (floats): activations A[0..3] | GA | GB (hidden-wide, n images each) | HO (64 channels) | GS0 | GS1 (state) | zero g_ldj (n)
// | (dW', db') scratch; deterministic mode appends | log-det slots of one launch (n x the most slots of a coupling / Split2d launch)
// | weight-gradient partials [slices][dW', db'] of the largest launch at this n
struct TrainSpace {
  float* A[4]; float* GA; float* GB; float* HO; float* GS0; float* GS1; float* gl0; float* scr;
  float* ldp; float* wpart;          // null unless the trainer is deterministic
  int64_t total;
};
int64_t det_ldj_floats(const gbnf_image_trainer* t, int64_t n);
int64_t det_wgrad_floats(const gbnf_image_trainer* t, int64_t n);
TrainSpace train_space(const gbnf_image_trainer* t, float* ws, int64_t n) {
  TrainSpace s{};
  const int64_t hid = (int64_t)((t->hidden + 15) / 16 * 16) * 256 * n, ho = (int64_t)64 * 256 * n, st = t->state_img * n;
  float* p = ws;
  for (int k = 0; k < 4; ++k) { s.A[k] = p; p += hid; }
  s.GA = p; p += hid; s.GB = p; p += hid;
  s.HO = p; p += ho;
  s.GS0 = p; p += st; s.GS1 = p; p += st;
  s.gl0 = p; p += (n + 63) / 64 * 64;
  s.scr = p; p += (t->scratch_floats + 63) / 64 * 64;
  if (t->deterministic) {
    s.ldp = p; p += (det_ldj_floats(t, n) + 63) / 64 * 64;
    s.wpart = p; p += (det_wgrad_floats(t, n) + 63) / 64 * 64;
  }
  s.total = p - ws;
  return s;
}

int check_tconv(const gbnf_conv& c, int cin, int cout, int ks, bool want_an, bool want_zeros, const char* what) {
  if (!c.weight) return fail(GBNF_ERR_INVALID, "%s: null weight", what);
  if (c.in_channels != cin || c.out_channels != cout || c.kernel_size != ks)
    return fail(GBNF_ERR_INVALID, "%s: is %dx%d k=%d, expected %dx%d k=%d", what, c.out_channels, c.in_channels, c.kernel_size, cout, cin, ks);
  if (want_an && (!c.actnorm_bias || !c.actnorm_logs)) return fail(GBNF_ERR_INVALID, "%s: needs its ActNorm2d arrays", what);
  if (want_zeros && (!c.bias || !c.logs)) return fail(GBNF_ERR_INVALID, "%s: Conv2dZeros needs bias and logs", what);
  return GBNF_OK;
}

// appends a convolution's entry; its gradient arrays take their places in the flat buffer in the documented order
void add_conv(gbnf_image_trainer* t, const gbnf_conv& c) {
  TConv e{};
  e.w = c.weight; e.bias = c.bias; e.an_bias = c.actnorm_bias; e.an_logs = c.actnorm_logs; e.logs = c.logs;
  e.cout = c.out_channels; e.cin = c.in_channels; e.ks = c.kernel_size; e.mix = 0;
  const int64_t wn = (int64_t)e.cout * e.cin * e.ks * e.ks;
  e.g_w = t->grad_floats; t->grad_floats += wn;
  e.g_bias = e.g_an_bias = e.g_an_logs = e.g_logs = -1;
  if (c.bias) { e.g_bias = t->grad_floats; t->grad_floats += e.cout; }
  if (c.actnorm_bias) { e.g_an_bias = t->grad_floats; t->grad_floats += e.cout; }
  if (c.actnorm_logs) { e.g_an_logs = t->grad_floats; t->grad_floats += e.cout; }
  if (c.logs) { e.g_logs = t->grad_floats; t->grad_floats += e.cout; }
  t->table.push_back(e);
}

void place(gbnf_image_trainer* t) {          // pack blob and scratch offsets of every entry
  int64_t off = 0, scr = 0;
  for (TConv& e : t->table) {
    const int64_t tf = tile_floats(e.cout, e.cin, e.ks);
    e.fwd_off = off; off += tf;
    e.bwd_off = off; off += tf;
    e.b_off = off; off += (e.cout + 15) / 16 * 16;
    e.gw_off = scr; scr += (int64_t)e.cout * e.cin * e.ks * e.ks;
    e.gb_off = scr; scr += e.cout;
  }
  t->zero_off = off; off += 1024;
  t->blob_floats = off;
  t->scratch_floats = scr;
}

// the shape of entry e's weight-gradient launch on H-row maps at a batch of n: p's block / item fields, -> the slice count.  A function
// of the layer's shape, n and WGRAD_ITEMS only (deterministic mode sizes its partials with it and adds them in slice order).
int wgrad_shape(const TConv& e, int H, int64_t n, WgradLaunch& p, int* blocks_out) {
  p.cin = e.cin; p.cout = e.cout; p.H = H; p.n_strips = H / TR_R; p.n_items = (int)(n * p.n_strips);
  const int OT = (e.cout + 15) / 16, IT = (e.cin + 15) / 16, NP = e.ks == 3 ? 2 : 4;
  p.obt = OT >= 4 ? 4 : (OT >= 2 ? 2 : 1);
  p.ibt = std::min(std::min(4 * NP / p.obt, 8), IT);
  const int n_ob = (OT + p.obt - 1) / p.obt;
  p.n_ib = (IT + p.ibt - 1) / p.ibt;
  const int blocks = n_ob * p.n_ib;
  // Slices: every workgroup flushes its whole block of dW' once, so a slice should hold SEVERAL (image, strip) items -- but the chip
  // wants many workgroups.  WGRAD_ITEMS[shape] = the least items of a slice for the first 3x3 (few input tiles), the last 3x3 (few
  // output tiles) and the 1x1 layers (measured: DESIGN.md section 4.7); GBNF_IMG_WGRAD_ITEMS="a,b,c" overrides them (tuning knob, read once).
  static const struct Items { int v[3]; } items = [] {
    Items r{{WGRAD_ITEMS[0], WGRAD_ITEMS[1], WGRAD_ITEMS[2]}};
    if (const char* e = getenv("GBNF_IMG_WGRAD_ITEMS")) {
      int a = 0, b = 0, c = 0;
      if (sscanf(e, "%d,%d,%d", &a, &b, &c) == 3 && a > 0 && b > 0 && c > 0) r = Items{{a, b, c}};
    }
    return r;
  }();
  const int min_items = items.v[e.ks == 1 ? 2 : (OT >= IT ? 0 : 1)];
  *blocks_out = blocks;
  return std::max(1, std::min((p.n_items + min_items - 1) / min_items, 1024 / blocks));
}

// part: null = the flush adds into scr with float atomics; else (deterministic mode) the slices store to part[slice][dW', db'] and a
// second launch adds them in slice order into scr
bool launch_wgrad(const TConv& e, const float* a, int64_t a_img, const float* g, int64_t g_img, float* scr, float* part, int H, int W, int Hv,
                  int64_t n, hipStream_t s) {
  WgradLaunch p{};
  int blocks = 0;
  const int slices = wgrad_shape(e, H, n, p, &blocks);
  p.a = a; p.a_img = a_img; p.g = g; p.g_img = g_img; p.dw = scr + e.gw_off; p.db = scr + e.gb_off;
  p.Hv = Hv;
  const int halo = e.ks >> 1, cs = ((TR_R + 2 * halo) * (W + 2 * halo)) | 1, npix = TR_R * W;
  const size_t lds = ((size_t)p.obt * 16 * (npix + 1) + (size_t)p.ibt * 16 * cs) * 4;
  const dim3 grid((unsigned)blocks, (unsigned)slices), blk(256);
  if (part != nullptr) {
    const int64_t wn = (int64_t)e.cout * e.cin * e.ks * e.ks, stride = wn + e.cout;       // (gb_off = gw_off + wn: place())
    p.dw = part; p.db = part + wn;
    if (W == 16 && e.ks == 3) hipLaunchKernelGGL((img_train_wgrad_det_kernel<4, 3>), grid, blk, lds, s, p, stride);
    else if (W == 16) hipLaunchKernelGGL((img_train_wgrad_det_kernel<4, 1>), grid, blk, lds, s, p, stride);
    else if (e.ks == 3) hipLaunchKernelGGL((img_train_wgrad_det_kernel<2, 3>), grid, blk, lds, s, p, stride);
    else hipLaunchKernelGGL((img_train_wgrad_det_kernel<2, 1>), grid, blk, lds, s, p, stride);
    hipLaunchKernelGGL(img_train_wgrad_reduce_kernel, dim3((unsigned)((stride + 255) / 256)), blk, 0, s, (const float*)part, stride, slices,
                       scr + e.gw_off);
    return true;
  }
  if (W == 16 && e.ks == 3) hipLaunchKernelGGL((img_train_wgrad_kernel<4, 3>), grid, blk, lds, s, p);
  else if (W == 16) hipLaunchKernelGGL((img_train_wgrad_kernel<4, 1>), grid, blk, lds, s, p);
  else if (e.ks == 3) hipLaunchKernelGGL((img_train_wgrad_kernel<2, 3>), grid, blk, lds, s, p);
  else hipLaunchKernelGGL((img_train_wgrad_kernel<2, 1>), grid, blk, lds, s, p);
  return true;
}

// deterministic mode's workspace pieces at a batch of n.  Both walk the launches the backward / forward make: per level its steps'
// mix and net convolutions and its split prior, all on the level's H-row maps.
int64_t det_wgrad_floats(const gbnf_image_trainer* t, int64_t n) {
  int64_t worst = 0;
  for (size_t l = 0; l < t->levels.size(); ++l) {
    auto one = [&](const TConv& e) {
      WgradLaunch p{};
      int blocks = 0;
      const int slices = wgrad_shape(e, t->levels[l].H, n, p, &blocks);
      worst = std::max(worst, (int64_t)slices * ((int64_t)e.cout * e.cin * e.ks * e.ks + e.cout));
    };
    for (int first : t->step_first[l])
      for (int q = 0; q <= t->n_net; ++q) one(t->table[first + q]);
    if (t->split_entry[l] >= 0) one(t->table[t->split_entry[l]]);
  }
  return worst;
}
int64_t det_ldj_floats(const gbnf_image_trainer* t, int64_t n) {
  int slots = 0;
  for (size_t l = 0; l < t->levels.size(); ++l) {
    const int n_strips = t->levels[l].H / TR_R;
    for (int first : t->step_first[l]) slots = std::max(slots, img_ldj_slots(t->table[first + t->n_net].cout, n_strips, n));
    if (t->split_entry[l] >= 0) slots = std::max(slots, img_ldj_slots(t->table[t->split_entry[l]].cout, n_strips, n));
  }
  return (int64_t)slots * n;
}

}  // namespace

extern "C" {

int gbnf_image_trainer_set_deterministic(gbnf_image_trainer* t, int32_t on) {
  if (!t) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_set_deterministic: trainer is null");
  t->deterministic = on ? 1 : 0;
  return GBNF_OK;
}

int gbnf_image_trainer_get_deterministic(const gbnf_image_trainer* t, int32_t* on) {
  if (!t || !on) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_get_deterministic: bad argument");
  *on = t->deterministic;
  return GBNF_OK;
}

int gbnf_image_trainer_destroy(gbnf_image_trainer* t) {
  if (!t) return GBNF_OK;
  if (t->table_dev) (void)hipFree(t->table_dev);
  if (t->ident_dev) (void)hipFree(t->ident_dev);
  if (t->blob_dev) (void)hipFree(t->blob_dev);
  if (t->perm_dev) (void)hipFree(t->perm_dev);
  image_step_state_destroy(t->step);
  delete t;
  return GBNF_OK;
}

int gbnf_image_trainer_create(const gbnf_image_flow_desc* d, gbnf_image_trainer** out) {
  if (!out) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_create: out is null");
  *out = nullptr;
  if (!d || !d->levels) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_create: null descriptor");
  if (d->n_levels < 1 || d->n_levels > 3) return fail(GBNF_ERR_UNSUPPORTED, "n_levels=%d outside [1,3]", d->n_levels);
  if (d->coupling != GBNF_COUPLING_AFFINE && d->coupling != GBNF_COUPLING_ADDITIVE) return fail(GBNF_ERR_INVALID, "unknown coupling %d", d->coupling);
  int C = d->channels, H = 32, W = 32, Hv = d->height, Wv = d->width;
  if (C < 1 || Hv < 2 || Wv < 2 || Hv > H || Wv > W) return fail(GBNF_ERR_UNSUPPORTED, "input %dx%dx%d: at most 32 x 32 pixels", C, Hv, Wv);
  if (!(d->bounds > 0.5f && d->bounds < 1.0f)) return fail(GBNF_ERR_INVALID, "bounds must be in (0.5, 1)");
  auto* t = new gbnf_image_trainer();
  t->C = C; t->Hi = Hv; t->Wi = Wv; t->L = d->n_levels; t->additive = d->coupling == GBNF_COUPLING_ADDITIVE; t->bounds = d->bounds;
  t->hidden = 0;
  t->ld_const = -std::log(256.0) * C * Hv * Wv;                  // dequantisation, models/glow.py:137
  t->state_img = (int64_t)C * H * W;
  std::vector<float> perm_host;
  std::vector<std::pair<size_t, size_t>> perm_fix;               // (entry, float offset into perm_host)
  char what[96];
  int rc = GBNF_OK;
  for (int l = 0; l < d->n_levels && rc == GBNF_OK; ++l) {
    const gbnf_image_level& lv = d->levels[l];
    if (Hv % 2 || Wv % 2) { rc = fail(GBNF_ERR_INVALID, "level %d: odd spatial size %d x %d", l, Hv, Wv); break; }
    C *= 4; H /= 2; W /= 2; Hv /= 2; Wv /= 2;
    if (H < 8) H = W = 8;
    if (C > 64) { rc = fail(GBNF_ERR_UNSUPPORTED, "level %d: %d channels > 64", l, C); break; }
    if (lv.n_steps < 1 || !lv.steps) { rc = fail(GBNF_ERR_INVALID, "level %d: no steps", l); break; }
    t->state_img = std::max(t->state_img, (int64_t)C * H * W);
    t->levels.push_back({C, H, W, Hv, Wv, lv.n_steps});
    t->step_first.emplace_back();
    const int c1 = C / 2, c2 = C - c1;
    for (int k = 0; k < lv.n_steps && rc == GBNF_OK; ++k) {
      const gbnf_image_step& st = lv.steps[k];
      if (!st.actnorm_bias || !st.actnorm_logs || (!st.perm_weight && !st.perm_indices)) {
        rc = fail(GBNF_ERR_INVALID, "level %d step %d: null actnorm / permutation", l, k); break;
      }
      TConv m{};
      m.mix = 1; m.cin = m.cout = C; m.ks = 1; m.an_bias = st.actnorm_bias; m.an_logs = st.actnorm_logs; m.hw = (float)(Hv * Wv);
      m.g_bias = m.g_logs = -1;
      m.g_an_bias = t->grad_floats; t->grad_floats += C;
      m.g_an_logs = t->grad_floats; t->grad_floats += C;
      if (st.perm_weight) {
        m.w = st.perm_weight;
        m.g_w = t->grad_floats; t->grad_floats += (int64_t)C * C;
      } else {
        m.g_w = -1;
        std::vector<char> seen(C, 0);
        const size_t off = perm_host.size();
        perm_host.resize(off + (size_t)C * C, 0.0f);
        for (int j = 0; j < C; ++j) {
          const int64_t src = st.perm_indices[j];
          if (src < 0 || src >= C || seen[src]) { rc = fail(GBNF_ERR_INVALID, "level %d step %d: perm_indices is not a permutation", l, k); break; }
          seen[src] = 1;
          perm_host[off + (size_t)j * C + src] = 1.0f;             // z[:, j] = y[:, indices[j]], models/layers.py:675-677
        }
        if (rc) break;
        perm_fix.emplace_back(t->table.size(), off);
      }
      t->step_first.back().push_back((int)t->table.size());
      t->table.push_back(m);
      if (st.n_convs < 2 || st.n_convs > 5 || !st.convs) { rc = fail(GBNF_ERR_INVALID, "level %d step %d: needs 2..5 convolutions", l, k); break; }
      const int hdim = st.convs[0].out_channels;
      if (hdim < 1 || hdim > 512) { rc = fail(GBNF_ERR_UNSUPPORTED, "hidden width %d outside [1,512]", hdim); break; }
      if (t->n_net != 0 && (t->n_net != st.n_convs || t->hidden != hdim)) {
        rc = fail(GBNF_ERR_UNSUPPORTED, "level %d step %d: every coupling net of a component has the same depth and width", l, k); break;
      }
      t->n_net = st.n_convs; t->hidden = hdim;
      for (int q = 0; q < st.n_convs && rc == GBNF_OK; ++q) {
        const bool first = q == 0, last = q == st.n_convs - 1;
        snprintf(what, sizeof(what), "level %d step %d conv %d", l, k, q);
        rc = check_tconv(st.convs[q], first ? c1 : hdim, last ? (t->additive ? c2 : 2 * c2) : hdim, (first || last) ? 3 : 1, !last, last, what);
        if (rc == GBNF_OK) add_conv(t, st.convs[q]);
      }
    }
    if (rc) break;
    if (l < d->n_levels - 1) {
      if (!lv.split_prior) { rc = fail(GBNF_ERR_INVALID, "level %d: missing Split2d prior", l); break; }
      if (C % 2) { rc = fail(GBNF_ERR_UNSUPPORTED, "Split2d on an odd channel count"); break; }
      snprintf(what, sizeof(what), "level %d split prior", l);
      rc = check_tconv(*lv.split_prior, C / 2, C, 3, false, true, what);
      if (rc) break;
      t->split_entry.push_back((int)t->table.size());
      add_conv(t, *lv.split_prior);
      C /= 2;
    } else {
      t->split_entry.push_back(-1);
    }
  }
  if (rc == GBNF_OK) {
    t->zC = C; t->zH = Hv; t->zW = Wv;
    for (const auto& lv : t->levels) t->trace_img += (int64_t)(2 * lv.K + 1) * lv.C * lv.H * lv.W;
    place(t);
    hipError_t e = hipSuccess;
    if (!perm_host.empty()) {
      e = hipMalloc((void**)&t->perm_dev, perm_host.size() * 4);
      if (e == hipSuccess) e = hipMemcpy(t->perm_dev, perm_host.data(), perm_host.size() * 4, hipMemcpyHostToDevice);
      for (const auto& f : perm_fix) t->table[f.first].w = t->perm_dev + f.second;
    }
    if (e == hipSuccess) e = hipMalloc((void**)&t->table_dev, t->table.size() * sizeof(TConv));
    if (e == hipSuccess) e = hipMemcpy(t->table_dev, t->table.data(), t->table.size() * sizeof(TConv), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      std::vector<TConv> ident(t->table);
      for (TConv& c : ident)
        if (!c.mix) c.an_bias = c.an_logs = nullptr;
      e = hipMalloc((void**)&t->ident_dev, ident.size() * sizeof(TConv));
      if (e == hipSuccess) e = hipMemcpy(t->ident_dev, ident.data(), ident.size() * sizeof(TConv), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMalloc((void**)&t->blob_dev, (size_t)t->blob_floats * 4);
    if (e == hipSuccess) e = hipMemset(t->blob_dev, 0, (size_t)t->blob_floats * 4);
    if (e == hipSuccess) e = img_allow_lds();
    if (e != hipSuccess) rc = fail(GBNF_ERR_HIP, "gbnf_image_trainer_create: %s", hipGetErrorString(e));
    if (rc == GBNF_OK) rc = image_step_state_create(t);
  }
  if (rc != GBNF_OK) {
    gbnf_image_trainer_destroy(t);
    return rc;
  }
  *out = t;
  return GBNF_OK;
}

int gbnf_image_trainer_trace_floats(const gbnf_image_trainer* t, int64_t n, int64_t* floats) {
  if (!t || !floats || n < 0) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_trace_floats: bad argument");
  *floats = t->trace_img * n;
  return GBNF_OK;
}

int gbnf_image_trainer_workspace_bytes(const gbnf_image_trainer* t, int64_t n, int64_t* bytes) {
  if (!t || !bytes || n < 0) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_workspace_bytes: bad argument");
  *bytes = train_space(t, nullptr, n).total * 4 + 256;
  return GBNF_OK;
}

int gbnf_image_trainer_grad_floats(const gbnf_image_trainer* t, int64_t* floats) {
  if (!t || !floats) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_grad_floats: bad argument");
  *floats = t->grad_floats;
  return GBNF_OK;
}

// the trace slots of level l: slot 0 = the level's input, 1 + 2k = P_k, 2 + 2k = O_k
static float* trace_slot(const gbnf_image_trainer* t, float* trace, int64_t n, int l, int slot) {
  int64_t off = 0;
  for (int q = 0; q < l; ++q) off += (int64_t)(2 * t->levels[q].K + 1) * t->levels[q].C * t->levels[q].H * t->levels[q].W;
  const auto& lv = t->levels[l];
  return trace + (off + (int64_t)slot * lv.C * lv.H * lv.W) * n;
}

static ConvLaunch conv_base(const gbnf_image_trainer::Level& lv, float* ldj) {
  ConvLaunch p{};
  p.H = lv.H; p.W = lv.W; p.Hv = lv.Hv; p.Wv = lv.Wv; p.n_strips = lv.H / TR_R; p.ldj = ldj;
  return p;
}

// the coupling net's hidden activations of one step into A[0 .. n_net - 2] (forward: ping-pong over two of them)
static void net_hidden(const gbnf_image_trainer* t, const gbnf_image_trainer::Level& lv, int first, const float* z1, int64_t img, float* const* A,
                       bool keep, int64_t n, hipStream_t s, const float** hin_out, int64_t* hin_img_out) {
  const float* hin = z1;
  int64_t hin_img = img;
  for (int q = 0; q + 1 < t->n_net; ++q) {
    const TConv& c = t->table[first + 1 + q];
    ConvLaunch p = conv_base(lv, nullptr);
    p.in = hin; p.in_img = hin_img; p.wp = t->blob_dev + c.fwd_off; p.bias = t->blob_dev + c.b_off;
    p.out = A[keep ? q : (q & 1)]; p.out_img = (int64_t)c.cout * lv.H * lv.W; p.cin = c.cin; p.cout = c.cout; p.ks = c.ks;
    img_launch_conv(EPI_RELU, p, (int)n, s);
    hin = p.out; hin_img = p.out_img;
  }
  *hin_out = hin; *hin_img_out = hin_img;
}

int gbnf_image_trainer_forward(gbnf_image_trainer* t, const float* x, const float* noise, int64_t n, float* z, float* ldj, float* trace,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (!t || !x || !ldj || !trace) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_forward: null argument (x, ldj and trace are required)");
  if (n <= 0) return n == 0 ? GBNF_OK : fail(GBNF_ERR_INVALID, "gbnf_image_trainer_forward: n < 0");
  if (n > 65535) return fail(GBNF_ERR_UNSUPPORTED, "gbnf_image_trainer_forward: at most 65535 images per call");
  const TrainSpace sp = train_space(t, (float*)workspace, n);
  if (!workspace || workspace_bytes < sp.total * 4) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int n_entries = (int)t->table.size();
  hipLaunchKernelGGL(img_train_pack_kernel, dim3(64, (unsigned)n_entries), dim3(256), 0, s, (const TConv*)t->table_dev, t->blob_dev);
  img_launch_pre(x, noise, trace_slot(t, trace, n, 0, 0), ldj, t->C, t->H, t->W, t->Hi, t->Wi, t->bounds, (float)t->ld_const, n, s);
  hipLaunchKernelGGL(img_train_ldconst_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const TConv*)t->table_dev, n_entries, ldj, n);
  for (int l = 0; l < t->L; ++l) {
    const auto& lv = t->levels[l];
    const int64_t img = (int64_t)lv.C * lv.H * lv.W;
    const int c1 = lv.C / 2;
    for (int k = 0; k < lv.K; ++k) {
      const int first = t->step_first[l][k];
      const float* prev = trace_slot(t, trace, n, l, 2 * k);
      float* P = trace_slot(t, trace, n, l, 1 + 2 * k);
      float* O = trace_slot(t, trace, n, l, 2 + 2 * k);
      const TConv& m = t->table[first];
      ConvLaunch p = conv_base(lv, ldj);
      p.in = prev; p.in_img = img; p.wp = t->blob_dev + m.fwd_off; p.bias = t->blob_dev + m.b_off; p.out = P; p.out_img = img;
      p.cin = lv.C; p.cout = lv.C; p.ks = 1;
      img_launch_conv(EPI_STORE, p, (int)n, s);
      if (hipMemcpyAsync(O, P, (size_t)img * n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(GBNF_ERR_HIP, "gbnf_image_trainer_forward: state copy failed");
      const float* hin; int64_t hin_img;
      net_hidden(t, lv, first, O, img, sp.A, false, n, s, &hin, &hin_img);
      const TConv& c = t->table[first + t->n_net];
      ConvLaunch q = conv_base(lv, ldj);
      q.in = hin; q.in_img = hin_img; q.wp = t->blob_dev + c.fwd_off; q.bias = t->blob_dev + c.b_off;
      q.st = O + (int64_t)c1 * lv.H * lv.W; q.st_img = img; q.cin = c.cin; q.cout = c.cout; q.ks = c.ks;
      if (t->deterministic && !t->additive) {
        // the waves store their log-det partials to the launch's slots; one thread per image adds them onto ldj in slot order
        q.ldj = sp.ldp;
        img_launch_conv(EPI_COUPLE_AFFINE_ORD, q, (int)n, s);
        img_launch_ldj_reduce(sp.ldp, img_ldj_slots(c.cout, q.n_strips, n), ldj, n, s);
      } else {
        img_launch_conv(t->additive ? EPI_COUPLE_ADD : EPI_COUPLE_AFFINE, q, (int)n, s);
      }
    }
    if (l < t->L - 1) {
      float* O = trace_slot(t, trace, n, l, 2 * lv.K);
      const TConv& c = t->table[t->split_entry[l]];
      ConvLaunch p = conv_base(lv, ldj);
      p.in = O; p.in_img = img; p.wp = t->blob_dev + c.fwd_off; p.bias = t->blob_dev + c.b_off;
      p.st = O + (int64_t)c1 * lv.H * lv.W; p.st_img = img; p.cin = c.cin; p.cout = c.cout; p.ks = c.ks;
      if (t->deterministic) {
        p.ldj = sp.ldp;
        img_launch_conv(EPI_SPLIT_ORD, p, (int)n, s);
        img_launch_ldj_reduce(sp.ldp, img_ldj_slots(c.cout, p.n_strips, n), ldj, n, s);
      } else {
        img_launch_conv(EPI_SPLIT, p, (int)n, s);
      }
      const auto& nx = t->levels[l + 1];
      img_launch_squeeze(O, img, trace_slot(t, trace, n, l + 1, 0), c1, lv.H, lv.W, nx.H, nx.W, n, s);
    }
  }
  if (z != nullptr) {
    const auto& lv = t->levels[t->L - 1];
    img_launch_final(trace_slot(t, trace, n, t->L - 1, 2 * lv.K), (int64_t)lv.C * lv.H * lv.W, t->blob_dev + t->zero_off, ldj, nullptr, z, lv.C,
                     lv.H, lv.W, lv.Hv, lv.Wv, n, s);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "gbnf_image_trainer_forward: %s", hipGetErrorString(e));
  return GBNF_OK;
}

// ---- gbnf_image_trainer_actnorm_init ------------------------------------------------------------------------------------------
// workspace: state S0 | S1 | hidden A0 | A1 (n images each) | a log-det sink (n; the epilogues add into it, nobody reads it) |
// doubles: the statistics partials [2][widest layer][AN_MAX_CHUNKS]
struct AnSpace {
  float* S[2]; float* A[2]; float* ldj; double* part;
  int64_t part_each;                 // doubles of one of the two partial arrays
  int64_t bytes;
};
static AnSpace an_space(const gbnf_image_trainer* t, void* ws, int64_t n) {
  AnSpace s{};
  const int64_t hid = (int64_t)((t->hidden + 15) / 16 * 16) * 256 * n, st = t->state_img * n;
  float* base = reinterpret_cast<float*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  float* p = base;
  for (int k = 0; k < 2; ++k) { s.S[k] = p; p += (st + 63) / 64 * 64; }
  for (int k = 0; k < 2; ++k) { s.A[k] = p; p += hid; }
  s.ldj = p; p += (n + 63) / 64 * 64;
  s.part = reinterpret_cast<double*>(p);
  s.part_each = (int64_t)std::max(t->hidden, 64) * AN_MAX_CHUNKS;
  s.bytes = (p - base) * 4 + 2 * s.part_each * 8 + 256;
  return s;
}

// t (n, C.., H, W of lv) -> bias / logs (the live tensors): sums, centred squares, finish
static void an_launch_stats(const gbnf_image_trainer::Level& lv, const float* tin, int64_t t_img, int C, int64_t n, float scale, const AnSpace& sp,
                            const float* bias, const float* logs, hipStream_t s) {
  AnStats p{};
  p.t = tin; p.t_img = t_img; p.n = n; p.HW = lv.H * lv.W; p.W = lv.W; p.Hv = lv.Hv; p.Wv = lv.Wv;
  const int64_t group = 4 * (256 / p.HW);                      // images the four waves of a workgroup read at a time
  const int64_t want = std::min<int64_t>(AN_MAX_CHUNKS, (n + group - 1) / group);
  p.per_chunk = (int)(((n + want - 1) / want + group - 1) / group * group);
  p.chunks = (int)((n + p.per_chunk - 1) / p.per_chunk);       // (<= want: a function of n and the map's storage only)
  p.sum = sp.part; p.sq = sp.part + sp.part_each;
  const dim3 grid((unsigned)p.chunks, (unsigned)C), blk(256);
  hipLaunchKernelGGL((img_train_an_stats_kernel<0>), grid, blk, 0, s, p);
  hipLaunchKernelGGL((img_train_an_stats_kernel<1>), grid, blk, 0, s, p);
  hipLaunchKernelGGL(img_train_an_finish_kernel, dim3((unsigned)((C + 255) / 256)), blk, 0, s, (const double*)p.sum, (const double*)p.sq, p.chunks, C,
                     (double)n * lv.Hv * lv.Wv, scale, const_cast<float*>(bias), const_cast<float*>(logs));
}

int gbnf_image_trainer_actnorm_count(const gbnf_image_trainer* t, int32_t* count) {
  if (!t || !count) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_actnorm_count: bad argument");
  int total = 0;
  for (const auto& lv : t->levels) total += lv.K * t->n_net;    // a step's own + one behind each Conv2d (all but the last convolution)
  *count = total;
  return GBNF_OK;
}

int gbnf_image_trainer_actnorm_init_workspace_bytes(const gbnf_image_trainer* t, int64_t n, int64_t* bytes) {
  if (!t || !bytes || n < 0) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_actnorm_init_workspace_bytes: bad argument");
  *bytes = an_space(t, nullptr, n).bytes;
  return GBNF_OK;
}

int gbnf_image_trainer_actnorm_init(gbnf_image_trainer* t, const float* x, const float* noise, int64_t n, float scale, const uint8_t* skip,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "gbnf_image_trainer_actnorm_init";
  if (!t || !x) return fail(GBNF_ERR_INVALID, "%s: trainer / x is null", fn);
  if (n < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld < 1", fn, (long long)n);
  if (!std::isfinite(scale) || !(scale > 0.0f)) return fail(GBNF_ERR_INVALID, "%s: scale must be finite and > 0", fn);
  if (n > 65535) return fail(GBNF_ERR_UNSUPPORTED, "%s: at most 65535 images per call", fn);
  const AnSpace sp = an_space(t, workspace, n);
  if (!workspace || workspace_bytes < sp.bytes)
    return fail(GBNF_ERR_INVALID, "%s: workspace too small (gbnf_image_trainer_actnorm_init_workspace_bytes)", fn);
  hipStream_t s = (hipStream_t)stream;
  if (const int rc = image_step_compose(t, stream)) return rc;
  const int n_entries = (int)t->table.size();
  hipLaunchKernelGGL(img_train_pack_kernel, dim3(64, (unsigned)n_entries), dim3(256), 0, s, (const TConv*)t->table_dev, t->blob_dev);
  int count = 0, todo = 0, layer = 0;
  for (const auto& lv : t->levels) count += lv.K * t->n_net;
  for (int q = 0; q < count; ++q) todo += (skip == nullptr || !skip[q]) ? 1 : 0;       // (none: the pack above is all there is to do)
  auto wanted = [&](int idx) { return skip == nullptr || !skip[idx]; };
  auto pack_one = [&](const TConv* table, int entry) {
    hipLaunchKernelGGL(img_train_pack_kernel, dim3(64, 1), dim3(256), 0, s, table + entry, t->blob_dev);
  };
  float* cur = sp.S[0];
  float* oth = sp.S[1];
  if (todo > 0) img_launch_pre(x, noise, cur, sp.ldj, t->C, t->H, t->W, t->Hi, t->Wi, t->bounds, (float)t->ld_const, n, s);
  for (int l = 0; l < t->L && todo > 0; ++l) {
    const auto& lv = t->levels[l];
    const int64_t img = (int64_t)lv.C * lv.H * lv.W;
    const int c1 = lv.C / 2;
    for (int k = 0; k < lv.K; ++k) {
      const int first = t->step_first[l][k];
      const TConv& m = t->table[first];
      if (wanted(layer)) {                                     // the step's own ActNorm2d: the state as it stands
        an_launch_stats(lv, cur, img, lv.C, n, scale, sp, m.an_bias, m.an_logs, s);
        pack_one(t->table_dev, first);
      }
      ++layer;
      ConvLaunch p = conv_base(lv, sp.ldj);
      p.in = cur; p.in_img = img; p.wp = t->blob_dev + m.fwd_off; p.bias = t->blob_dev + m.b_off; p.out = oth; p.out_img = img;
      p.cin = lv.C; p.cout = lv.C; p.ks = 1;
      img_launch_conv(EPI_STORE, p, (int)n, s);
      std::swap(cur, oth);
      const float* hin = cur;
      int64_t hin_img = img;
      for (int q = 0; q + 1 < t->n_net; ++q, ++layer) {
        const int entry = first + 1 + q;
        const TConv& c = t->table[entry];
        ConvLaunch h = conv_base(lv, nullptr);
        h.in = hin; h.in_img = hin_img; h.wp = t->blob_dev + c.fwd_off; h.bias = t->blob_dev + c.b_off;
        h.out = sp.A[q & 1]; h.out_img = (int64_t)c.cout * lv.H * lv.W; h.cin = c.cin; h.cout = c.cout; h.ks = c.ks;
        if (wanted(layer)) {
          // the raw convolution on identity tiles, its statistics into the live tensors, the real tiles; relu(ActNorm2d(conv)) below
          pack_one(t->ident_dev, entry);
          img_launch_conv(EPI_STORE, h, (int)n, s);
          an_launch_stats(lv, h.out, h.out_img, c.cout, n, scale, sp, c.an_bias, c.an_logs, s);
          pack_one(t->table_dev, entry);
        }
        img_launch_conv(EPI_RELU, h, (int)n, s);
        hin = h.out; hin_img = h.out_img;
      }
      const TConv& c = t->table[first + t->n_net];
      ConvLaunch q = conv_base(lv, sp.ldj);
      q.in = hin; q.in_img = hin_img; q.wp = t->blob_dev + c.fwd_off; q.bias = t->blob_dev + c.b_off;
      q.st = cur + (int64_t)c1 * lv.H * lv.W; q.st_img = img; q.cin = c.cin; q.cout = c.cout; q.ks = c.ks;
      img_launch_conv(t->additive ? EPI_COUPLE_ADD : EPI_COUPLE_AFFINE, q, (int)n, s);
    }
    if (l < t->L - 1) {
      const TConv& c = t->table[t->split_entry[l]];
      ConvLaunch p = conv_base(lv, sp.ldj);
      p.in = cur; p.in_img = img; p.wp = t->blob_dev + c.fwd_off; p.bias = t->blob_dev + c.b_off;
      p.st = cur + (int64_t)c1 * lv.H * lv.W; p.st_img = img; p.cin = c.cin; p.cout = c.cout; p.ks = c.ks;
      img_launch_conv(EPI_SPLIT, p, (int)n, s);
      const auto& nx = t->levels[l + 1];
      img_launch_squeeze(cur, img, oth, c1, lv.H, lv.W, nx.H, nx.W, n, s);
      std::swap(cur, oth);
    }
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

// weight gradient of entry `c` and the data gradient of its input.  dst_store: the adjoint's result is stored there (stride dst_img);
// dst_add: it is ADDED there (the z1 half of the state gradient); both null: no data gradient wanted.  scr null: no weight gradient
// wanted (the data-gradient-only form of gbnf_image_trainer_backward_x).
static void conv_backward(const gbnf_image_trainer* t, const gbnf_image_trainer::Level& lv, const TConv& c, const float* in, int64_t in_img,
                          const float* G, int64_t G_img, float* scr, float* part, float* dst_store, float* dst_add, int64_t dst_img, int64_t n,
                          hipStream_t s) {
  if (scr != nullptr) launch_wgrad(c, in, in_img, G, G_img, scr, part, lv.H, lv.W, lv.Hv, n, s);
  if (!dst_store && !dst_add) return;
  ConvLaunch p = conv_base(lv, nullptr);
  p.in = G; p.in_img = G_img; p.wp = t->blob_dev + c.bwd_off; p.bias = t->blob_dev + t->zero_off;
  p.cin = c.cout; p.cout = c.cin; p.ks = c.ks;
  if (dst_store) { p.out = dst_store; p.out_img = dst_img; img_launch_conv(EPI_STORE, p, (int)n, s); }
  else { p.st = dst_add; p.st_img = dst_img; img_launch_conv(EPI_COUPLE_ADD, p, (int)n, s); }
}

// gbnf_image_trainer_backward (g_x null, grads required) and gbnf_image_trainer_backward_x (g_x required: the state gradient also
// goes through the first step's mix and the adjoint of img_pre_body; grads null: no weight-gradient launch, no scratch memset, no
// unfold).  The caller has checked every argument.
static int trainer_backward(const char* fn, gbnf_image_trainer* t, const float* trace_c, int64_t n, const float* g_z, const float* g_ldj,
                            float* grads, const float* x, const float* noise, float* g_x, int accumulate, const TrainSpace& sp, hipStream_t s) {
  float* trace = const_cast<float*>(trace_c);                // (read only)
  float* const scr = grads != nullptr ? sp.scr : nullptr;
  hipError_t e = scr != nullptr ? hipMemsetAsync(scr, 0, (size_t)t->scratch_floats * 4, s) : hipSuccess;
  const float* gl = g_ldj;
  if (gl == nullptr) {
    if (e == hipSuccess) e = hipMemsetAsync(sp.gl0, 0, (size_t)n * 4, s);
    gl = sp.gl0;
  }
  float* cur = sp.GS0;
  float* oth = sp.GS1;
  {
    const auto& lv = t->levels[t->L - 1];
    if (g_z != nullptr) img_launch_embed(g_z, cur, lv.C, lv.H, lv.W, lv.Hv, lv.Wv, n, s);
    else if (e == hipSuccess) e = hipMemsetAsync(cur, 0, (size_t)lv.C * lv.H * lv.W * n * 4, s);
  }
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  for (int l = t->L - 1; l >= 0; --l) {
    const auto& lv = t->levels[l];
    const int HW = lv.H * lv.W, c1 = lv.C / 2, c2 = lv.C - c1;
    const int64_t img = (int64_t)lv.C * HW;
    if (l < t->L - 1) {
      // cur: the gradient of the next level's input (4 c1 channels) -> the z1 half of this level's output; Split2d gives the other
      const auto& nx = t->levels[l + 1];
      img_launch_unsqueeze(cur, oth, img, c1, lv.H, lv.W, nx.H, nx.W, n, s);
      std::swap(cur, oth);
      float* O = trace_slot(t, trace, n, l, 2 * lv.K);
      const TConv& c = t->table[t->split_entry[l]];
      ConvLaunch p = conv_base(lv, nullptr);
      p.in = O; p.in_img = img; p.wp = t->blob_dev + c.fwd_off; p.bias = t->blob_dev + c.b_off;
      p.out = sp.HO; p.out_img = (int64_t)c.cout * HW; p.cin = c.cin; p.cout = c.cout; p.ks = c.ks;
      img_launch_conv(EPI_STORE, p, (int)n, s);
      const int64_t total = n * (int64_t)c1 * HW;              // (C even: the dropped half has c1 channels)
      hipLaunchKernelGGL(img_train_split_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, sp.HO, p.out_img,
                         (const float*)(O + (int64_t)c1 * HW), img, cur + (int64_t)c1 * HW, img, gl, c1, lv.H, lv.W, lv.Hv, lv.Wv, total);
      conv_backward(t, lv, c, O, img, sp.HO, p.out_img, scr, sp.wpart, nullptr, cur, img, n, s);
    }
    for (int k = lv.K - 1; k >= 0; --k) {
      const int first = t->step_first[l][k];
      float* prev = trace_slot(t, trace, n, l, 2 * k);
      float* P = trace_slot(t, trace, n, l, 1 + 2 * k);
      // the net again: hidden activations kept this time, and its raw output
      const float* hin; int64_t hin_img;
      net_hidden(t, lv, first, P, img, sp.A, true, n, s, &hin, &hin_img);
      const TConv& cl = t->table[first + t->n_net];
      const int64_t ho_img = (int64_t)cl.cout * HW;
      if (!t->additive) {                                      // (the additive coupling's gradient does not need the net's output)
        ConvLaunch p = conv_base(lv, nullptr);
        p.in = hin; p.in_img = hin_img; p.wp = t->blob_dev + cl.fwd_off; p.bias = t->blob_dev + cl.b_off;
        p.out = sp.HO; p.out_img = ho_img; p.cin = cl.cin; p.cout = cl.cout; p.ks = cl.ks;
        img_launch_conv(EPI_STORE, p, (int)n, s);
      }
      const int64_t total = n * (int64_t)c2 * HW;
      const dim3 eg((unsigned)((total + 255) / 256));
      if (t->additive)
        hipLaunchKernelGGL((img_train_couple_bwd_kernel<false>), eg, dim3(256), 0, s, sp.HO, ho_img, (const float*)(P + (int64_t)c1 * HW), img,
                           cur + (int64_t)c1 * HW, img, gl, c2, lv.H, lv.W, lv.Hv, lv.Wv, total);
      else
        hipLaunchKernelGGL((img_train_couple_bwd_kernel<true>), eg, dim3(256), 0, s, sp.HO, ho_img, (const float*)(P + (int64_t)c1 * HW), img,
                           cur + (int64_t)c1 * HW, img, gl, c2, lv.H, lv.W, lv.Hv, lv.Wv, total);
      // the net's convolutions, last to first
      const float* G = sp.HO;
      int64_t G_img = ho_img;
      for (int q = t->n_net - 1; q >= 0; --q) {
        const TConv& c = t->table[first + 1 + q];
        if (q == 0) {
          conv_backward(t, lv, c, P, img, G, G_img, scr, sp.wpart, nullptr, cur, img, n, s);
        } else {
          float* Gn = (G == sp.GA) ? sp.GB : sp.GA;
          const int64_t a_img = (int64_t)c.cin * HW;
          conv_backward(t, lv, c, sp.A[q - 1], a_img, G, G_img, scr, sp.wpart, Gn, nullptr, a_img, n, s);
          const int64_t total4 = n * a_img / 4;
          hipLaunchKernelGGL(img_train_relu_mask_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, Gn, (const float*)sp.A[q - 1], total4);
          G = Gn; G_img = a_img;
        }
      }
      // the mix: cur is the gradient of P_k now
      const bool need_data = !(l == 0 && k == 0) || g_x != nullptr;      // (the first step's input gradient: only on the way to g_x)
      conv_backward(t, lv, t->table[first], prev, img, cur, img, scr, sp.wpart, need_data ? oth : nullptr, nullptr, img, n, s);
      if (need_data) std::swap(cur, oth);
    }
  }
  if (grads != nullptr)
    hipLaunchKernelGGL(img_train_unfold_kernel, dim3(128, (unsigned)t->table.size()), dim3(256), 0, s, (const TConv*)t->table_dev, (const float*)scr,
                       g_ldj, n, grads);
  // cur: the gradient of level 0's input, (n, 4C, H/2, W/2) storage -> the image proper
  if (g_x != nullptr)
    img_launch_pre_adjoint(x, noise, cur, gl, g_x, t->C, t->H, t->W, t->Hi, t->Wi, t->bounds, accumulate, n, s);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

int gbnf_image_trainer_backward(gbnf_image_trainer* t, const float* trace_c, int64_t n, const float* g_z, const float* g_ldj, float* grads,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  if (!t || !trace_c || !grads) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_backward: null argument");
  if (n <= 0) return n == 0 ? GBNF_OK : fail(GBNF_ERR_INVALID, "gbnf_image_trainer_backward: n < 0");
  if (n > 65535) return fail(GBNF_ERR_UNSUPPORTED, "gbnf_image_trainer_backward: at most 65535 images per call");
  const TrainSpace sp = train_space(t, (float*)workspace, n);
  if (!workspace || workspace_bytes < sp.total * 4) return fail(GBNF_ERR_INVALID, "gbnf_image_trainer_backward: workspace too small");
  return trainer_backward("gbnf_image_trainer_backward", t, trace_c, n, g_z, g_ldj, grads, nullptr, nullptr, nullptr, 0, sp, (hipStream_t)stream);
}

int gbnf_image_trainer_backward_x(gbnf_image_trainer* t, const float* trace_c, const float* x, const float* noise, int64_t n, const float* g_z,
                                  const float* g_ldj, float* grads, float* g_x, int32_t accumulate, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  const char* fn = "gbnf_image_trainer_backward_x";
  if (!t || !trace_c || !x || !g_x) return fail(GBNF_ERR_INVALID, "%s: null argument (trainer, trace, x and g_x are required)", fn);
  if (n <= 0) return n == 0 ? GBNF_OK : fail(GBNF_ERR_INVALID, "%s: n < 0", fn);
  if (n > 65535) return fail(GBNF_ERR_UNSUPPORTED, "%s: at most 65535 images per call", fn);
  int64_t need = 0;
  if (const int rc = gbnf_image_trainer_workspace_bytes(t, n, &need)) return rc;
  if (!workspace || workspace_bytes < need)
    return fail(GBNF_ERR_INVALID, "%s: workspace too small: %lld bytes < %lld (gbnf_image_trainer_workspace_bytes)", fn,
                (long long)workspace_bytes, (long long)need);
  const TrainSpace sp = train_space(t, (float*)workspace, n);
  return trainer_backward(fn, t, trace_c, n, g_z, g_ldj, grads, x, noise, g_x, accumulate ? 1 : 0, sp, (hipStream_t)stream);
}

}  // extern "C"
