// gbnf_wgrad_safe_kernel.inc -- the body of wgrad_safe_kernel (GBNF_WG_DET 0: the text of the kernel as it always was) and of wgrad_safe_det_kernel
// (GBNF_WG_DET 1: chunk `by` of a block stores its tile to part[by][..], see gbnf_train.hip).  Included twice by gbnf_train.hip.
#if GBNF_WG_DET
#define WG_DST (part + (int64_t)by * part_stride)
#else
#define WG_DST grads
#endif
  __shared__ float rsum[4][64];
  if (gate != nullptr && *gate == 0u) return;        // (the bf16x6 re-run of a repairing trainer's call that did not meet the range)
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx >= n_blocks) {
    if (by != 0 || red.partials == nullptr || bx - n_blocks >= 2 * red.K) return;
    const int kw = bx - n_blocks, j = threadIdx.x & 63, part = threadIdx.x >> 6;      // 4 parts
    if ((red.skip_steps >> (kw >> 1)) & 1u) return;
    const float* src = red.partials + kw * 64 + j;
    const int64_t stride = (int64_t)red.K * 128;
    float a[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] = 0.0f;
    int b = part;
    for (; b + 4 * 7 < red.n_wg; b += 4 * 8) {
#pragma unroll
      for (int q = 0; q < 8; ++q) a[q] += src[(int64_t)(b + 4 * q) * stride];
    }
    for (; b < red.n_wg; b += 4) a[0] += src[(int64_t)b * stride];
    rsum[part][j] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    __syncthreads();
    if (part == 0 && j < red.d) grads[red.goff[kw] + j] += (rsum[0][j] + rsum[1][j]) + (rsum[2][j] + rsum[3][j]);
    return;
  }
  float alpha = 1.0f, inv_alpha = 1.0f;          // the gradient-side operands were emitted on the scaled gradient
  if (gmax != nullptr) tr_grad_scale(__builtin_amdgcn_readfirstlane(*gmax), alpha, inv_alpha);
  int pi = 0;
  while (pi + 1 < n_probs && bx >= probs[pi + 1].blk_begin) ++pi;
  const WgProblem P = probs[pi];
  const int blk = bx - P.blk_begin;
  const int m0 = (blk / P.nb) * WGS_BLOCK, n0 = (blk % P.nb) * WGS_BLOCK;
  const int64_t s_begin = (int64_t)by * chunk;
  const int64_t s_end = (s_begin + chunk < np) ? s_begin + chunk : np;
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wmi = wave >> 1, wni = wave & 1;
  typedef const f32x4 __attribute__((address_space(1)))* gv4;
  // this lane's rows (clamped into the operand's own sub-region: a row past it only feeds outputs that are never stored) and its
  // 8 samples of a 32-sample step: tile g / 2, samples 8 (g & 1) .. + 7
  unsigned doff[2], aoff[2];
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    const int rd = m0 + 32 * wmi + 16 * x + i, ra = n0 + 32 * wni + 16 * x + i;
    doff[x] = (unsigned)((g >> 1) * P.d_rows * 16 + (rd < P.d_rows ? rd : P.d_rows - 1) * 16 + 8 * (g & 1));
    aoff[x] = (unsigned)((g >> 1) * P.a_rows * 16 + (ra < P.a_rows ? ra : P.a_rows - 1) * 16 + 8 * (g & 1));
  }
  const float* dbase = ws + P.d_row * np;
  const float* abase = ws + P.a_row * np;
  auto fetch = [&](f32x4 (&dv)[2][2], f32x4 (&av)[2][2], int64_t s) {
    const gv4 dp = (gv4)(dbase + s * P.d_rows), ap = (gv4)(abase + s * P.a_rows);
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      dv[x][0] = dp[doff[x] >> 2]; dv[x][1] = dp[(doff[x] >> 2) + 1];
      av[x][0] = ap[aoff[x] >> 2]; av[x][1] = ap[(aoff[x] >> 2) + 1];
    }
  };
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[2][2][3];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[x][y][c] = zero;
  float bs[2] = {0.0f, 0.0f};
  const bool own_bias = n0 == 0 && wni == 0;
  // the products of one f32 product, smallest terms first, and the running sum each goes to (Products<3>)
  constexpr int PW[6] = {2, 0, 1, 1, 0, 0}, PX[6] = {0, 2, 1, 0, 1, 0}, PA[6] = {2, 2, 2, 1, 1, 0};
  f32x4 dv[2][2], av[2][2], dn[2][2], an[2][2];
  fetch(dv, av, s_begin);
  for (int64_t s = s_begin; s < s_end; s += 32) {
    fetch(dn, an, s + 32 < s_end ? s + 32 : s);        // one step ahead (past the end: this step again, unused)
    u32x4 dp[2][3], ap[2][3];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      wgs_split8(dv[x][0], dv[x][1], dp[x]);
      wgs_split8(av[x][0], av[x][1], ap[x]);
      if (own_bias) {
        const f32x4 u = dv[x][0] + dv[x][1];
        bs[x] += (u[0] + u[1]) + (u[2] + u[3]);
      }
    }
#pragma unroll
    for (int pr = 0; pr < 6; ++pr)
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y][PA[pr]] = wgs_mfma(dp[x][PW[pr]], ap[y][PX[pr]], acc[x][y][PA[pr]]);
#pragma unroll
    for (int x = 0; x < 2; ++x) { dv[x][0] = dn[x][0]; dv[x][1] = dn[x][1]; av[x][0] = an[x][0]; av[x][1] = an[x][1]; }
  }
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      tr_mfma_drain(acc[x][y][0], acc[x][y][1]);
      tr_mfma_drain(acc[x][y][2], acc[x][y][2]);
    }
  if (own_bias) {      // db[m] = sum over samples of D[m][.]: the four lane groups hold 8 samples each of row i
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      float v = bs[x];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      const int m = m0 + 32 * wmi + 16 * x + i;
#if GBNF_WG_DET
      if (g == 0 && m < P.M) WG_DST[P.b_off + m] = v * inv_alpha;
#else
      if (g == 0 && m < P.M) atomicAdd(grads + P.b_off + m, v * inv_alpha);
#endif
    }
  }
  float* C = WG_DST + P.c_off;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const f32x4 v = acc[x][y][0] + (acc[x][y][1] + acc[x][y][2]);
      const int n = n0 + 32 * wni + 16 * y + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 32 * wmi + 16 * x + 4 * g + r;
#if GBNF_WG_DET
        if (m < P.M && n < P.N) C[(size_t)m * P.N + n] = v[r] * inv_alpha;
#else
        if (m < P.M && n < P.N) atomicAdd(C + (size_t)m * P.N + n, v[r] * inv_alpha);
#endif
      }
    }
#undef WG_DST
