// gbnf_train_bwd.hip.h -- the backward sweep of the training path, register-chained (round 3).
//
// What loss.backward() of density_experiment.py:366-374 does to one component, given what the forward sweep
// (flow_kernel_hx3<..., TRAIN = 1>) saved: every step's normalised state (trace), the coupling nets' inputs, hidden
// activations and outputs (operand workspace).  Nothing is recomputed: per step, last to first,
//
//   coupling backward   g_z2 -> g_y2, g_shift, g_raw / g_scale   (element-wise, from the saved net outputs and the trace)
//   dgrad chain         g_o -> W3^T -> (.) act'(h2) -> W2^T -> (.) act'(h1) -> W1^T -> g_y1      (split-f16 MFMA; written for depth 1:
//                       depth 0 has no W2^T link, depth 2 one more, a one-block ResidualNet is depth 2 with its skip -- template DEPTH)
//   normalisation bwd   g_y -> g_x, ActNorm / BatchNorm parameter gradients (16-sample sums + atomics)
//
// and the gradient-side operands of every weight gradient (g_o, g_a2, g_a1) go to the operand workspace for wgrad_kernel.
// The chain has the shape of the forward chain -- a layer with K0 = ceil(OT / 2) input chunks, one with HC chunks, an output
// layer of two tiles -- and is written like it (gbnf_flow_kernel_hx3.hip.h): a wave owns its 16 samples through all three
// layers (D layout = B layout: the accumulator tile of one layer, times act' and split, IS the next layer's B operand),
// the transposed weights are staged once per workgroup by LDS DMA, one stage ahead, in consumption order.
// Reference semantics: FlowStep.encode models/glow.py:317-342, RealNVP.forward models/transformations.py:560-579,
// _ActNorm models/layers.py:488-533, BatchNorm (running statistics) models/layers.py:337-358, TanhNet / ReLUNet :208-243.
#pragma once

#include "gbnf_flow_kernel_hx3.hip.h"

#ifndef GBNF_BWD_PREFETCH
#define GBNF_BWD_PREFETCH 0        // 1: L2-warming look-ahead of the saved operands (see bwd_warm_lines)
#endif
#ifndef GBNF_BWD_ABLATE
#define GBNF_BWD_ABLATE 0          // diagnostic builds (tools/build_bwd_ablations.sh, timing only): 1 no parameter sums, 2 no operand stores, 4 no activation loads
#endif

namespace gbnf {

// Packed layout of one coupling net's TRANSPOSED weights (NP fragments per tile: 2 = f16x3, 3 = bf16x6), in consumption order.  The net has
// layer 0 (input -> hidden), DEPTH hidden -> hidden layers 1 .. DEPTH and the output layer DEPTH + 1 (coupling_network_depth 0, 1, 2):
//   L0' stages : W(DEPTH+1)^T tile rows t (hidden tile t = 16 output units of this layer), K0 tiles (k-chunks of 32 net outputs)
//                each, ROWS0 tile rows per stage
//   MID u      : (DEPTH = 2) W2^T row u, chunks c = 0..HC-1
//   PASS u     : (DEPTH >= 1) W1^T row u, chunks c = 0..HC-1; then, if u is even and u >= 2, the W0^T chunk (u-2)/2: IT = 2 tiles
//   DRAIN      : (DEPTH >= 1) W0^T chunk HC-1
//   IN k       : (DEPTH = 0) W0^T chunks k CGI .. : IT tiles each
struct BwdLayout {
  static constexpr int MAXS = 96;
  int HC, K0, ROWS0, N_L0, NS, NET_WORDS, STAGE_FRAGS, DEPTH, CGI, N_IN, NP;
  int off[MAXS], nf[MAXS];
  constexpr BwdLayout(int HT, int OT, int depth = 1, int np = 2)
      : HC((HT + 1) / 2), K0((OT + 1) / 2), ROWS0(1), N_L0(0), NS(0), NET_WORDS(0), STAGE_FRAGS(0), DEPTH(depth), CGI(1), N_IN(0), NP(np),
        off{}, nf{} {
    ROWS0 = (HC + 2) / K0 > 0 ? (HC + 2) / K0 : 1;
    N_L0 = (HT + ROWS0 - 1) / ROWS0;
    int s = 0, w = 0;
    for (int i = 0; i < N_L0; ++i) {
      const int cnt = (HT - i * ROWS0 < ROWS0) ? HT - i * ROWS0 : ROWS0;
      off[s] = w; nf[s] = np * cnt * K0; w += nf[s] * 256; ++s;
    }
    if (depth >= 1) {
      for (int j = depth; j >= 2; --j)
        for (int u = 0; u < HT; ++u) {
          off[s] = w; nf[s] = np * HC; w += nf[s] * 256; ++s;
        }
      for (int u = 0; u < HT; ++u) {
        off[s] = w; nf[s] = np * HC + ((u % 2 == 0 && u >= 2) ? np * 2 : 0); w += nf[s] * 256; ++s;
      }
      off[s] = w; nf[s] = np * 2; w += nf[s] * 256; ++s;
    } else {
      CGI = (HC + 2) / 2;                                 // chunks per stage: about the fragments of a pass
      N_IN = (HC + CGI - 1) / CGI;
      for (int k = 0; k < N_IN; ++k) {
        const int cnt = (HC - k * CGI < CGI) ? HC - k * CGI : CGI;
        off[s] = w; nf[s] = np * 2 * cnt; w += nf[s] * 256; ++s;
      }
    }
    NS = s;
    NET_WORDS = w;
    for (int k = 0; k < s; ++k) STAGE_FRAGS = nf[k] > STAGE_FRAGS ? nf[k] : STAGE_FRAGS;
  }
};
template <int HT, int OT, int DEPTH, int NP = 2>
struct BwdLayoutOf {
  static constexpr BwdLayout value = BwdLayout(HT, OT, DEPTH, NP);
};

// the device side of tr_grad_scale (gbnf_train.hip): alpha = the power of two that puts the largest upstream entry at [4, 8)
__device__ __forceinline__ void bwd_grad_scale(unsigned max_bits, float& alpha, float& inv_alpha) {
  const int e = (int)((max_bits >> 23) & 255u);
  if (max_bits == 0u || e == 255) { alpha = 1.0f; inv_alpha = 1.0f; return; }
  int k = 2 - (e - 127);
  k = k > 100 ? 100 : (k < -100 ? -100 : k);
  alpha = __builtin_bit_cast(float, (unsigned)(k + 127) << 23);
  inv_alpha = __builtin_bit_cast(float, (unsigned)(127 - k) << 23);
}

// sum over the 16 lanes of a lane group (the wave's 16 samples): a lane group is one DPP row, so four rotate-and-add steps on
// the VALU leave the sum in every lane (__shfl_xor compiles to ds_bpermute: 128 LDS round trips per step, a third of the kernel)
__device__ __forceinline__ float bwd_sum16(float v) {
  auto ror = [](float a, auto n_c) {
    constexpr int CTRL = 0x120 + decltype(n_c)::value;      // row_ror:n
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), CTRL, 0xf, 0xf, false));
  };
  v += ror(v, std::integral_constant<int, 8>{});
  v += ror(v, std::integral_constant<int, 4>{});
  v += ror(v, std::integral_constant<int, 2>{});
  v += ror(v, std::integral_constant<int, 1>{});
  return v;
}

// L2-warming look-ahead (GBNF_BWD_PREFETCH): one LDS-DMA dword per lane from 64 DIFFERENT cache lines (lane l reads the first word of
// line l of a block) into a dead 256-byte LDS cell -- no register is written, so nothing can be clobbered when the data lands, and the
// kernel's real loads of those lines (the saved activations a pass needs two tiles ahead, the next step's boundary operands) then
// find them in the L2 / Infinity Cache instead of waiting out an HBM round trip with nothing on the SIMD to switch to.  Counts as ONE
// vector-memory operation (vmcnt) like every LDS-DMA; the dword form is what tools/isa_hazard_lint.py tells from a staging DMA (x4).
__device__ __forceinline__ void bwd_warm_lines(const float* base, unsigned lane_off, uint32_t* dead_cell) {
  const unsigned m0v = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)dead_cell;
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(lane_off), "s"(base), "s"(m0v) : "memory", "m0");
}

// Waves per SIMD the 4-wave form is compiled for: 2 (256 registers, two workgroups share a CU and cover each other's memory
// latency: 498 -> 3xx us at N = 65536) where the kernel fits -- its register count is 8 per hidden tile (the saved second-layer
// activations and the split g_a2 operands) + ~125 (measured: HT = 14 -> 235) -- else 1 (512 registers).
constexpr int bwd_hx3_occupancy(int KIND, int HT, int OT, int DEPTH = 1, int PREC = 0) {
#ifdef GBNF_BWD_OCC
  return GBNF_BWD_OCC;
#else
  // (two hidden -> hidden layers: a second set of split gradient operands, 4 registers per hidden tile)
  // (a one-block ResidualNet at 7 hidden tiles spills 65 registers with two waves per SIMD and is still 12 % faster than with one:
  //  measured 0.98 against 1.10 ms of backward + wgrad at N = 65536 -- the skip tiles are NOT counted here)
  // (bf16x6: three pieces per split operand -- 2 more registers per hidden tile and operand set -- and three running sums per tile.
  //  An ESTIMATE from those counts, not a measured register use like the f16x3 line below)
  if (PREC == 1) return (DEPTH >= 2 ? 16 : 10) * HT + (DEPTH == 4 ? 60 : 0) + 150 + (KIND == GBNF_KIND_REALNVP ? 8 * OT + 8 : 0) <= 250 ? 2 : 1;
  return (DEPTH >= 2 ? 12 : 8) * HT + (DEPTH == 4 ? 60 : 0) + 125 + (KIND == GBNF_KIND_REALNVP ? 8 * OT + 8 : 0) <= 250 ? 2 : 1;
#endif
}
#define GBNF_BWD_KERNEL bwd_kernel_hx3
#define GBNF_BWD_PREC 0
#include "gbnf_train_bwd_kernel.inc"
#undef GBNF_BWD_KERNEL
#undef GBNF_BWD_PREC
// the range-safe form (bf16x6): what a trainer of GBNF_MATH_BF16X6 runs
#define GBNF_BWD_KERNEL bwd_kernel_hx3_safe
#define GBNF_BWD_PREC 1
#include "gbnf_train_bwd_kernel.inc"
#undef GBNF_BWD_KERNEL
#undef GBNF_BWD_PREC

inline size_t bwd_hx3_lds_bytes(int n_steps, int waves, int stage_frags, int d) {
  return ((size_t)n_steps * SMALL_WORDS + 2 * (size_t)stage_frags * 256 + (size_t)waves * (d + 1) * 17 + (size_t)waves * 32 * 17 +
          (size_t)waves * n_steps * 128 + (GBNF_BWD_PREFETCH ? 64 : 0)) * 4;
}

// 4-wave workgroups, one wave per SIMD (the kernel keeps a whole layer of saved activations in registers: 290-330 of a lone
// wave's 512); the 8-wave form exists for geometries whose 4-wave LDS does not fit at all
inline int bwd_hx3_waves(int n_steps, int stage_frags, int d) {
  return bwd_hx3_lds_bytes(n_steps, 4, stage_frags, d) <= 160 * 1024 ? 4 : 8;
}

// the kernel of an arithmetic: PREC 0 = f16x3, 1 = bf16x6 (the two have one function type; only the one asked for is instantiated)
template <int KIND, int HT, int OT, int ACTA, int ACTB, int WV, int DEPTH, int PREC>
constexpr auto bwd_kernel_of() {
  if constexpr (PREC == 0) return &bwd_kernel_hx3<KIND, HT, OT, ACTA, ACTB, WV, DEPTH>;
  else return &bwd_kernel_hx3_safe<KIND, HT, OT, ACTA, ACTB, WV, DEPTH>;
}

template <int KIND, int HT, int OT, int ACTA, int ACTB, int WV, int DEPTH, int PREC = 0>
static hipError_t bwd_launch_wv(FlowLaunch p, hipStream_t s) {
  constexpr BwdLayout L(HT, OT, DEPTH, hx3_pieces(PREC));
  constexpr auto kernel = bwd_kernel_of<KIND, HT, OT, ACTA, ACTB, WV, DEPTH, PREC>();
  const size_t lds = bwd_hx3_lds_bytes(p.n_steps, WV, L.STAGE_FRAGS, p.d);
  if (lds > 160 * 1024 || p.n_steps > LDS_TABLE_STEPS) return hipErrorInvalidValue;
  const long long tiles = p.np / 16;               // every padded row (np is a multiple of 32): wgrad_kernel sums over all of them
  const long long grid = (tiles + WV - 1) / WV;
  static DynamicLdsOptIn opt_in;
  if (hipError_t e = opt_in({(const void*)kernel}); e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(64 * WV), lds, s, p);
  return hipGetLastError();
}

// registry key: VariantKey{kind, ht, -3 (f16x3) | -6 (bf16x6: a `safe` line of variants.list), /*ks1*/ 2 (backward), ot, /*nt*/ 1, depth,
// act_a, act_b}; PREC: 0 | 1
#define GBNF_INSTANTIATE_HX3_BWD(PREC, KIND, HT, OT, ACTA, ACTB, DEPTH)                                     \
  namespace gbnf {                                                                                          \
  static hipError_t launch_hx3b_##KIND##_##HT##_##OT##_##ACTA##_##ACTB##_##DEPTH(const FlowLaunch& p0, unsigned, hipStream_t s) { \
    constexpr BwdLayout L(HT, OT, DEPTH, hx3_pieces(PREC));                                                 \
    if (bwd_hx3_waves(p0.n_steps, L.STAGE_FRAGS, p0.d) == 4) return bwd_launch_wv<KIND, HT, OT, ACTA, ACTB, 4, DEPTH, PREC>(p0, s); \
    return bwd_launch_wv<KIND, HT, OT, ACTA, ACTB, 8, DEPTH, PREC>(p0, s);                                  \
  }                                                                                                         \
  static const int reg_hx3b_##KIND##_##HT##_##OT##_##ACTA##_##ACTB##_##DEPTH =                              \
      (register_variant(VariantKey{KIND, HT, PREC == 0 ? -3 : -6, 2, OT, 1, DEPTH, ACTA, ACTB},            \
                        launch_hx3b_##KIND##_##HT##_##OT##_##ACTA##_##ACTB##_##DEPTH,                       \
                        PREC == 0 ? "bwd_kernel_hx3<" #KIND "," #HT "," #OT "," #ACTA "," #ACTB "," #DEPTH ">"       \
                                  : "bwd_kernel_hx3_safe<" #KIND "," #HT "," #OT "," #ACTA "," #ACTB "," #DEPTH ">"), \
       0);                                                                                                  \
  }

}  // namespace gbnf
