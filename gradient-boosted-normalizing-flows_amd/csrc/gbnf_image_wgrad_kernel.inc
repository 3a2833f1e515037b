// gbnf_image_wgrad_kernel.inc -- the body of img_train_wgrad_kernel<PT,KS> (GBNF_IWG_DET 0: the text of the kernel as it always was,
// the flush adds with float atomics) and of img_train_wgrad_det_kernel<PT,KS> (GBNF_IWG_DET 1: slice blockIdx.y STORES its dW' tile
// entries and db' rows to partials[blockIdx.y][entry], p.dw / p.db pointing at slice 0 and `part_stride` floats between slices; a
// slice whose items all lie outside the map stores the zeros it holds).  Included twice by gbnf_image_train.hip.
#if GBNF_IWG_DET
#define IWG_FLUSH(ptr, v) (*((ptr) + (int64_t)blockIdx.y * part_stride) = (v))
#else
#define IWG_FLUSH(ptr, v) atomicAdd((ptr), (v))
#endif
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int W = 16 * PT / TR_R, NPIX = 16 * PT, HALO = KS >> 1;
  constexpr int WP = W + 2 * HALO, RP = TR_R + 2 * HALO, CS = RP * WP;
  constexpr int CSP = CS | 1, GSP = NPIX + 1;                 // odd channel strides: the 16 channels of a fragment hit 16 banks
  constexpr int TAPS = KS * KS, NP = KS == 3 ? 2 : 4;
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ob = blockIdx.x / p.n_ib, ib = blockIdx.x - ob * p.n_ib;
  const int och = p.obt * 16, ich = p.ibt * 16, npairs = p.obt * p.ibt;
  const int co0 = ob * och, ci0 = ib * ich;
  float* gL = lds;
  float* aL = lds + och * GSP;
  const int H = p.H;

  f32x4 acc[NP][TAPS];
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int t = 0; t < TAPS; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.0f;

  for (int item = blockIdx.y; item < p.n_items; item += gridDim.y) {
    const int n = item / p.n_strips, strip = item - n * p.n_strips, r0 = strip * TR_R;
    if (r0 >= p.Hv) continue;                                // (uniform) the gradient is zero on rows outside the map
    __syncthreads();                                         // the previous item's fragments are read
    {
      const float* gs = p.g + (int64_t)n * p.g_img + (int64_t)r0 * W;
      for (int idx = threadIdx.x; idx < och * NPIX; idx += 256) {
        const int ch = idx / NPIX, px = idx - ch * NPIX, co = co0 + ch;
        gL[ch * GSP + px] = co < p.cout ? gs[(int64_t)co * H * W + px] : 0.0f;
      }
      const float* as = p.a + (int64_t)n * p.a_img;
      for (int idx = threadIdx.x; idx < ich * CS; idx += 256) {
        const int ch = idx / CS, rem = idx - ch * CS, rr = rem / WP, cc = rem - rr * WP;
        const int row = r0 + rr - HALO, col = cc - HALO, ci = ci0 + ch;
        float v = 0.0f;
        if (ci < p.cin && row >= 0 && row < H && col >= 0 && col < W) v = as[((int64_t)ci * H + row) * W + col];
        aL[ch * CSP + rem] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int q = wave + 4 * j;
      if (q < npairs) {
        const int ol = q % p.obt, il = q / p.obt;
        const float* gf = gL + (ol * 16 + i) * GSP + g;
        const float* af = aL + (il * 16 + i) * CSP + HALO * WP + HALO;
        for (int kk = 0; kk < NPIX / 4; ++kk) {
          const int px = 4 * kk + g, pr = px / W, pc = px - pr * W;
          const float gv = gf[4 * kk];
          const float* ap = af + pr * WP + pc;
#pragma unroll
          for (int t = 0; t < TAPS; ++t) {
            const int dy = t / KS - HALO, dx = t % KS - HALO;
            acc[j][t] = tr_mfma(gv, ap[dy * WP + dx], acc[j][t]);
          }
        }
      }
    }
    if (ib == 0 && (int)threadIdx.x < och) {
      float s = 0.0f;
      for (int px = 0; px < NPIX; ++px) s += gL[threadIdx.x * GSP + px];
      dbacc += s;
    }
  }
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int t = 0; t < TAPS; ++t) tr_drain(acc[j][t]);
  // flush: lane (i, g) holds dW'[16 ot + 4 g + r][16 it + i] of every tap
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int q = wave + 4 * j;
    if (q < npairs) {
      const int ol = q % p.obt, il = q / p.obt;
      const int ci = ci0 + il * 16 + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + ol * 16 + 4 * g + r;
        if (co < p.cout && ci < p.cin) {
          float* dst = p.dw + ((int64_t)co * p.cin + ci) * TAPS;
#pragma unroll
          for (int t = 0; t < TAPS; ++t) IWG_FLUSH(dst + t, acc[j][t][r]);
        }
      }
    }
  }
  if (ib == 0 && (int)threadIdx.x < och && co0 + (int)threadIdx.x < p.cout) IWG_FLUSH(p.db + co0 + threadIdx.x, dbacc);
#undef IWG_FLUSH
