// gbnf_wgrad_kernel.inc -- the body of wgrad_kernel (GBNF_WG_DET 0: the text of the kernel as it always was) and of wgrad_det_kernel
// (GBNF_WG_DET 1: chunk `by` of a block stores its tile to part[by][..], see gbnf_train.hip).  Included twice by gbnf_train.hip.
#if GBNF_WG_DET
#define WG_DST (part + (int64_t)by * part_stride)
#else
#define WG_DST grads
#endif
  extern __shared__ __attribute__((aligned(16))) u32x4 wg_stage_raw[];      // WG_LDS_BYTES (dynamic: > 64 KB)
  // Launch index L = y G + x is dealt out in order (round-robin over the XCDs, a workgroup to every CU as it falls free); work
  // item L is chunk L mod Y of block L / Y, and the host numbers the blocks heaviest first (a 256 x 256 block streams 64 KB per
  // k-step, a 256 x 64 one 40 KB: a CU pulls ~24 GB/s whatever it does, so the time of a block is its bytes): the light blocks
  // fill in behind the heavy ones instead of the heavy ones finishing alone.
  int bx, by;
  {
    const int Y = gridDim.y, L = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
    bx = L / Y;
    by = L - bx * Y;
  }
  // blocks behind the dW blocks (first sample chunk only): the fixed-order sum of the backward kernel's per-workgroup
  // ActNorm / BatchNorm gradient partials, grads[goff[kw] + j] += sum_b partials[b][kw][j]  (kw = step * 2 + which)
  if (bx >= n_blocks) {
    if (by != 0 || red.partials == nullptr || bx - n_blocks >= 2 * red.K) return;
    float (*rsum)[64] = reinterpret_cast<float (*)[64]>(wg_stage_raw);       // (no static LDS)
    const int kw = bx - n_blocks, j = threadIdx.x & 63, part = threadIdx.x >> 6;      // 8 parts
    if ((red.skip_steps >> (kw >> 1)) & 1u) return;           // added already (a BatchNorm step of a batch-statistics sweep)
    const float* src = red.partials + kw * 64 + j;
    const int64_t stride = (int64_t)red.K * 128;
    // (16 loads in flight per thread: with 4 the 512 partials of an N = 65536 sweep were 16 dependent round trips, 11.8 us)
    float a[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = 0.0f;
    int b = part;
    for (; b + 8 * 15 < red.n_wg; b += 8 * 16) {
#pragma unroll
      for (int q = 0; q < 16; ++q) a[q] += src[(int64_t)(b + 8 * q) * stride];
    }
    for (; b < red.n_wg; b += 8) a[0] += src[(int64_t)b * stride];
    rsum[part][j] = (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) +
                    (((a[8] + a[9]) + (a[10] + a[11])) + ((a[12] + a[13]) + (a[14] + a[15])));
    __syncthreads();
    if (part == 0 && j < red.d)
      grads[red.goff[kw] + j] += ((rsum[0][j] + rsum[1][j]) + (rsum[2][j] + rsum[3][j])) + ((rsum[4][j] + rsum[5][j]) + (rsum[6][j] + rsum[7][j]));
    return;
  }
  float alpha = 1.0f, inv_alpha = 1.0f;          // the gradient-side operands were emitted on the scaled gradient
  if (gmax != nullptr) tr_grad_scale(__builtin_amdgcn_readfirstlane(*gmax), alpha, inv_alpha);
  int pi = 0;
  while (pi + 1 < n_probs && bx >= probs[pi + 1].blk_begin) ++pi;
  const WgProblem P = probs[pi];
  const int blk = bx - P.blk_begin;
  const int m0 = (blk / P.nb) * P.bm, n0 = (blk % P.nb) * P.bn;
  const int64_t s_begin = (int64_t)by * chunk;       // `chunk` samples per block (a multiple of 32)
  const int64_t s_end = (s_begin + chunk < np) ? s_begin + chunk : np;
  // pieces per thread (a 64-row operand: one, repeated by the upper waves) and the wave's tile of the block, see wg_shape()
#define WG_CASE(BM, BN, ND, NA, TM, TN) \
  if (P.bm == BM && P.bn == BN) return wgrad_block<ND, NA, TM, TN, (TM * TN < 32), (GBNF_WG_DET != 0)>(P, ws, WG_DST, np, s_begin, s_end, m0, n0, inv_alpha, wg_stage_raw)
  // (no 256 x 128 / 128 x 256: a trainer's hidden layers are square and its other edges are at most 64 -- wg_shape never cuts one)
  WG_CASE(256, 256, 2, 2, 8, 4);
  WG_CASE(256, 64, 2, 1, 2, 4);
  WG_CASE(64, 256, 1, 2, 4, 2);
  WG_CASE(128, 128, 1, 1, 4, 2);
  WG_CASE(128, 64, 1, 1, 2, 2);
  WG_CASE(64, 128, 1, 1, 2, 2);
  WG_CASE(64, 64, 1, 1, 2, 1);
#undef WG_CASE
#undef WG_DST
