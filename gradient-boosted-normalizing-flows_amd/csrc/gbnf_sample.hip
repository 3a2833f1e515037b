// gbnf_sample.hip -- drawing from the boosted MIXTURE on the device (gfx950): every row gets a component of its own, the rows are
// partitioned by component, and each component's rows go through gbnf_flow_inverse as ONE contiguous batch.  What the reference leaves as
// a TODO (models/boosted_flow.py:209-218: one component per call, drawn on the host, :61-96) and a user writes in eager PyTorch today
// (a per-row draw, a boolean-mask loop over the components, a scatter back).
//
//   the draw                 gbnf_resample_rows on w = rho[0:n_used] (gbnf_boost.hip: the f64 cdf in index order, a binary search per row)
//   sample_hist_kernel       narrows the draw to int32 and counts every CHUNK of rows per component (integer LDS atomics: a count does not
//                            depend on the order of arrival)
//   sample_scan_kernel       one workgroup: counts[c], the exclusive scan component-major then chunk, the segments' padding
//   sample_rank_kernel       a row's rank among its chunk's rows of the same component by wave ballot + prefix popcount -> order
//   sample_gather_kernel     z[order[q]] -> its segment of the sorted buffer (consecutive lanes, consecutive floats of a row)
//   sample_scatter_kernel    the sorted x / log|det| back to the caller's rows
//
// Memory-bound, no matrix pipe, no float arithmetic at all outside the draw: comp, order and counts are bit-identical from run to run, and
// a component's segment holds its rows in ascending caller index (a stable counting sort).  The flow kernels are not touched: a segment
// starts on a multiple of 64 rows of the sorted buffer (a 256-byte boundary, what they have always been handed) and is launched exactly
// as a caller's batch of that many rows would be.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gbnf.h"
#include "gbnf_internal.h"

namespace gbnf {

constexpr int SAMPLE_THREADS = 256;                          // 4 waves
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr int SAMPLE_ROUNDS = 4;                             // 64-row rounds per wave
constexpr int SAMPLE_WAVE_ROWS = 64 * SAMPLE_ROUNDS;         // a wave owns 256 consecutive rows of its chunk
constexpr int SAMPLE_CHUNK = SAMPLE_THREADS * SAMPLE_ROUNDS; // rows per workgroup of the histogram and rank kernels: 1024
constexpr int SAMPLE_MAX_COMPONENTS = 1024;                  // per-wave running counts live in LDS: 4 x 1024 x 4 bytes
constexpr int SAMPLE_SCAN_THREADS = 1024;
constexpr int SAMPLE_SCAN_WAVES = SAMPLE_SCAN_THREADS / 64;
constexpr int SAMPLE_SEGMENT_ALIGN = 64;                     // rows: 64 x d floats = a multiple of 256 bytes for every d
constexpr int SAMPLE_COPY_MAX_BLOCKS = 256 * 8;              // grid-stride copies: 8 workgroups per CU

static int64_t sample_align256(int64_t b) { return (b + 255) / 256 * 256; }
static int64_t sample_chunks(int64_t n) { return (n + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK; }

// The caller's workspace in 256-byte aligned pieces.  `rows` = n + 64 n_flows: every segment rounded up to 64 rows.  The cdf piece holds
// the draw's n_flows doubles first and, once the search has read them, the segments' padding (sample_scan_kernel) until the scatter.
struct SampleLayout {
  int64_t rows, z, x, ldj, hist, cdf, total;
};
static SampleLayout sample_layout(int n_flows, int64_t n, int d) {
  SampleLayout L;
  L.rows = n + (int64_t)SAMPLE_SEGMENT_ALIGN * n_flows;
  int64_t off = 0;
  L.z = off; off += sample_align256(L.rows * d * 4);
  L.x = off; off += sample_align256(L.rows * d * 4);
  L.ldj = off; off += sample_align256(L.rows * 4);
  L.hist = off; off += sample_align256(sample_chunks(n) * n_flows * 8);
  L.cdf = off; off += sample_align256((int64_t)n_flows * 8);
  L.total = off;
  return L;
}

// comp[i] = (int32) drawn[i], clamped into [0, C) whatever the draw left;  hist[c * n_chunks + b] = rows of component c in chunk b
__global__ void __launch_bounds__(SAMPLE_THREADS) sample_hist_kernel(const int64_t* __restrict__ drawn, int64_t n, int C,
                                                                     int* __restrict__ comp, int64_t* __restrict__ hist,
                                                                     int64_t n_chunks) {
  __shared__ int cnt[SAMPLE_MAX_COMPONENTS];
  for (int c = threadIdx.x; c < C; c += SAMPLE_THREADS) cnt[c] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SAMPLE_CHUNK;
#pragma unroll
  for (int r = 0; r < SAMPLE_ROUNDS; ++r) {
    const int64_t i = base + r * SAMPLE_THREADS + threadIdx.x;
    if (i < n) {
      int64_t c = drawn[i];
      c = c < 0 ? 0 : (c >= C ? C - 1 : c);
      comp[i] = (int)c;
      atomicAdd(&cnt[c], 1);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += SAMPLE_THREADS) hist[(int64_t)c * n_chunks + blockIdx.x] = cnt[c];
}

// One workgroup, component after component: counts[c] = the component's rows; hist[c][b] becomes the position in `order` of the component's
// first row of chunk b (the exclusive scan over (component, chunk) in that order); pad[c] = start_c - (rows of the components before c),
// start_0 = 0, start_c = roundup64(start_{c-1} + counts[c-1]): what turns a position in `order` into a row of the sorted buffer.
// Thread t owns a contiguous run of chunks, as resample_scan_kernel's threads own rows.
__global__ void __launch_bounds__(SAMPLE_SCAN_THREADS) sample_scan_kernel(int64_t* __restrict__ hist, int64_t n_chunks, int C,
                                                                          int64_t* __restrict__ counts, int64_t* __restrict__ pad) {
  __shared__ int64_t wave_tot[SAMPLE_SCAN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t run_len = (n_chunks + SAMPLE_SCAN_THREADS - 1) / SAMPLE_SCAN_THREADS;
  int64_t begin = (int64_t)tid * run_len;
  if (begin > n_chunks) begin = n_chunks;
  int64_t end = begin + run_len;
  if (end > n_chunks) end = n_chunks;
  int64_t before = 0, start = 0;                      // rows of the components before c / first row of c's segment
  for (int c = 0; c < C; ++c) {
    int64_t* h = hist + (int64_t)c * n_chunks;
    int64_t s = 0;
    for (int64_t b = begin; b < end; ++b) s += h[b];
    int64_t incl = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int64_t run = before + incl - s, total = 0;
    for (int k = 0; k < SAMPLE_SCAN_WAVES; ++k) {
      if (k < wave) run += wave_tot[k];
      total += wave_tot[k];
    }
    for (int64_t b = begin; b < end; ++b) {
      const int64_t v = h[b];
      h[b] = run;
      run += v;
    }
    if (tid == 0) {
      counts[c] = total;
      pad[c] = start - before;
    }
    start = (start + total + SAMPLE_SEGMENT_ALIGN - 1) / SAMPLE_SEGMENT_ALIGN * SAMPLE_SEGMENT_ALIGN;
    before += total;
    __syncthreads();                                  // wave_tot is rewritten for the next component
  }
}

// order[q] = i for row i of component c in chunk b:  q = hist[c][b] + (rows of c in the chunk before row i).  Wave w owns the chunk's rows
// [256 w, 256 w + 256) in four rounds of 64: inside a round the lanes of one component are found by ballot and ranked by the popcount
// of the lanes below; `run[w][c]` carries the wave's count from round to round (wave-private until the barrier), and the waves before
// w add their totals afterwards.
__global__ void __launch_bounds__(SAMPLE_THREADS) sample_rank_kernel(const int* __restrict__ comp, int64_t n, int C,
                                                                     const int64_t* __restrict__ hist, int64_t n_chunks,
                                                                     int64_t* __restrict__ order) {
  __shared__ int run_lds[SAMPLE_WAVES * SAMPLE_MAX_COMPONENTS];
  volatile int* run = run_lds;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < SAMPLE_WAVES * C; k += SAMPLE_THREADS) run[k] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SAMPLE_CHUNK + (int64_t)wave * SAMPLE_WAVE_ROWS;
  const unsigned long long below = (1ull << lane) - 1ull;
  int c_of[SAMPLE_ROUNDS], rank_of[SAMPLE_ROUNDS];
#pragma unroll
  for (int r = 0; r < SAMPLE_ROUNDS; ++r) {
    const int64_t i = base + r * 64 + lane;
    const bool valid = i < n;
    const int c = valid ? comp[i] : -1;
    int rank = 0;
    unsigned long long todo = __ballot(valid);
    while (todo) {                                    // once per component present in this round (wave-uniform)
      const int leader = __ffsll((long long)todo) - 1;
      const int c0 = __shfl(c, leader);
      const unsigned long long same = __ballot(c == c0);
      const int seen = run[wave * C + c0];
      if (c == c0) rank = seen + __popcll(same & below);
      if (lane == leader) run[wave * C + c0] = seen + __popcll(same);
      todo &= ~same;
    }
    c_of[r] = c;
    rank_of[r] = rank;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SAMPLE_ROUNDS; ++r) {
    const int c = c_of[r];
    if (c < 0) continue;
    int rank = rank_of[r];
    for (int w = 0; w < wave; ++w) rank += run[w * C + c];
    order[hist[(int64_t)c * n_chunks + blockIdx.x] + rank] = base + r * 64 + lane;
  }
}

// The component whose segment holds position q of `order`: the largest c with first_c <= q, where first_c = hist[c][0] is the position of
// the component's first row (what sample_scan_kernel left there; first_0 = 0, and an empty component shares its successor's).
__device__ __forceinline__ int segment_of(const int64_t* __restrict__ hist, int64_t n_chunks, int C, int64_t q) {
  int lo = 0, hi = C;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (hist[(int64_t)mid * n_chunks] <= q) lo = mid; else hi = mid;
  }
  return lo;
}

// z_sorted[(q + pad[c]) * d + j] = z[order[q] * d + j], c = the segment of q
__global__ void __launch_bounds__(SAMPLE_THREADS) sample_gather_kernel(const float* __restrict__ z, const int64_t* __restrict__ order,
                                                                       const int64_t* __restrict__ hist, int64_t n_chunks, int C,
                                                                       const int64_t* __restrict__ pad, int64_t n, int d,
                                                                       float* __restrict__ z_sorted) {
  const int64_t total = n * d, stride = (int64_t)gridDim.x * SAMPLE_THREADS;
  for (int64_t e = (int64_t)blockIdx.x * SAMPLE_THREADS + threadIdx.x; e < total; e += stride) {
    const int64_t q = e / d;
    const int j = (int)(e - q * d);
    z_sorted[(q + pad[segment_of(hist, n_chunks, C, q)]) * d + j] = z[order[q] * d + j];
  }
}

// x[order[q]] = x_sorted[q + pad[c]], ldj[order[q]] = ldj_sorted[q + pad[c]] (ldj null: skipped)
__global__ void __launch_bounds__(SAMPLE_THREADS) sample_scatter_kernel(const float* __restrict__ x_sorted, const float* __restrict__ ldj_sorted,
                                                                        const int64_t* __restrict__ order, const int64_t* __restrict__ hist,
                                                                        int64_t n_chunks, int C, const int64_t* __restrict__ pad, int64_t n,
                                                                        int d, float* __restrict__ x, float* __restrict__ ldj) {
  const int64_t total = n * d, stride = (int64_t)gridDim.x * SAMPLE_THREADS;
  for (int64_t e = (int64_t)blockIdx.x * SAMPLE_THREADS + threadIdx.x; e < total; e += stride) {
    const int64_t q = e / d;
    const int j = (int)(e - q * d);
    const int64_t i = order[q];
    const int64_t p = q + pad[segment_of(hist, n_chunks, C, q)];
    x[i * d + j] = x_sorted[p * d + j];
    if (j == 0 && ldj != nullptr) ldj[i] = ldj_sorted[p];
  }
}

static unsigned copy_blocks(int64_t elems) {
  const int64_t nb = (elems + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
  return (unsigned)(nb < SAMPLE_COPY_MAX_BLOCKS ? nb : SAMPLE_COPY_MAX_BLOCKS);
}

}  // namespace gbnf

using namespace gbnf;

extern "C" {

int gbnf_mixture_sample_workspace_bytes(int32_t n_flows, int64_t n, int32_t d, int64_t* bytes) {
  const char* fn = "gbnf_mixture_sample_workspace_bytes";
  if (!bytes) return fail(GBNF_ERR_INVALID, "%s: bytes is null", fn);
  if (n_flows < 1 || n < 1 || d < 1) return fail(GBNF_ERR_INVALID, "%s: n_flows = %d, n = %lld, d = %d (all must be >= 1)", fn, n_flows, (long long)n, d);
  *bytes = sample_layout(n_flows, n, d).total;
  return GBNF_OK;
}

int gbnf_mixture_sample_begin(const float* rho_dev, int32_t n_used, const float* u, const float* z_or_null, int64_t n, int32_t d,
                              int32_t* comp, int64_t* order, int64_t* counts_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "gbnf_mixture_sample_begin";
  if (!rho_dev || !u || !comp || !order || !counts_dev || !workspace)
    return fail(GBNF_ERR_INVALID, "%s: rho_dev / u / comp / order / counts_dev / workspace is null", fn);
  if (n < 1 || n_used < 1 || d < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld, n_used = %d, d = %d (all must be >= 1)", fn, (long long)n, n_used, d);
  if (n_used > SAMPLE_MAX_COMPONENTS) return fail(GBNF_ERR_UNSUPPORTED, "%s: n_used = %d > %d components", fn, n_used, SAMPLE_MAX_COMPONENTS);
  const SampleLayout L = sample_layout(n_used, n, d);
  if (workspace_bytes < L.total)
    return fail(GBNF_ERR_INVALID, "%s: workspace of %lld bytes < %lld (gbnf_mixture_sample_workspace_bytes)", fn, (long long)workspace_bytes, (long long)L.total);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int64_t* hist = (int64_t*)(ws + L.hist);
  int64_t* pad = (int64_t*)(ws + L.cdf);
  // the draw lands in `order` (n int64, what gbnf_resample_rows writes); the histogram kernel narrows it into comp before the rank
  // kernel writes the real order
  if (const int rc = gbnf_resample_rows(rho_dev, n_used, u, n, order, ws + L.cdf, sample_align256((int64_t)n_used * 8), stream)) return rc;
  const int64_t n_chunks = sample_chunks(n);
  if (n_chunks >= (1LL << 31)) return fail(GBNF_ERR_UNSUPPORTED, "%s: n = %lld rows", fn, (long long)n);
  hipLaunchKernelGGL(sample_hist_kernel, dim3((unsigned)n_chunks), dim3(SAMPLE_THREADS), 0, s, (const int64_t*)order, n, (int)n_used, comp, hist, n_chunks);
  hipLaunchKernelGGL(sample_scan_kernel, dim3(1), dim3(SAMPLE_SCAN_THREADS), 0, s, hist, n_chunks, (int)n_used, counts_dev, pad);
  hipLaunchKernelGGL(sample_rank_kernel, dim3((unsigned)n_chunks), dim3(SAMPLE_THREADS), 0, s, (const int*)comp, n, (int)n_used, (const int64_t*)hist, n_chunks, order);
  if (z_or_null != nullptr)
    hipLaunchKernelGGL(sample_gather_kernel, dim3(copy_blocks(n * d)), dim3(SAMPLE_THREADS), 0, s, z_or_null, (const int64_t*)order, (const int64_t*)hist,
                       n_chunks, (int)n_used, (const int64_t*)pad, n, (int)d, (float*)(ws + L.z));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

int gbnf_mixture_sample_finish(gbnf_flow* const* flows, int32_t n_flows, const int64_t* counts_host, const int64_t* order, int64_t n,
                               float* x, float* ldj_or_null, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "gbnf_mixture_sample_finish";
  if (!flows || !counts_host || !order || !x || !workspace)
    return fail(GBNF_ERR_INVALID, "%s: flows / counts_host / order / x / workspace is null", fn);
  if (n < 1 || n_flows < 1) return fail(GBNF_ERR_INVALID, "%s: n = %lld, n_flows = %d (both must be >= 1)", fn, (long long)n, n_flows);
  if (n_flows > SAMPLE_MAX_COMPONENTS) return fail(GBNF_ERR_UNSUPPORTED, "%s: n_flows = %d > %d components", fn, n_flows, SAMPLE_MAX_COMPONENTS);
  int d = 0;
  int64_t sum = 0;
  for (int c = 0; c < n_flows; ++c) {
    int dc = 0;
    if (!flows[c] || flow_features(flows[c], &dc)) return fail(GBNF_ERR_INVALID, "%s: flow %d is null", fn, c);
    if (c == 0) d = dc;
    if (dc != d) return fail(GBNF_ERR_INVALID, "%s: flow %d has d = %d, flow 0 d = %d", fn, c, dc, d);
    if (counts_host[c] < 0 || counts_host[c] > n) return fail(GBNF_ERR_INVALID, "%s: counts_host[%d] = %lld outside [0, n]", fn, c, (long long)counts_host[c]);
    sum += counts_host[c];
  }
  if (sum != n) return fail(GBNF_ERR_INVALID, "%s: counts_host sums to %lld, n = %lld", fn, (long long)sum, (long long)n);
  const SampleLayout L = sample_layout(n_flows, n, d);
  if (workspace_bytes < L.total)
    return fail(GBNF_ERR_INVALID, "%s: workspace of %lld bytes < %lld (gbnf_mixture_sample_workspace_bytes)", fn, (long long)workspace_bytes, (long long)L.total);
  char* ws = (char*)workspace;
  const float* z_sorted = (const float*)(ws + L.z);
  float* x_sorted = (float*)(ws + L.x);
  float* ldj_sorted = (float*)(ws + L.ldj);
  int64_t start = 0;
  for (int c = 0; c < n_flows; ++c) {                 // the rule of sample_scan_kernel, from the counts the caller read back
    const int64_t m = counts_host[c];
    if (m > 0)
      if (const int rc = gbnf_flow_inverse(flows[c], z_sorted + start * d, m, x_sorted + start * d, ldj_or_null ? ldj_sorted + start : nullptr, stream))
        return rc;
    start = (start + m + SAMPLE_SEGMENT_ALIGN - 1) / SAMPLE_SEGMENT_ALIGN * SAMPLE_SEGMENT_ALIGN;
  }
  hipLaunchKernelGGL(sample_scatter_kernel, dim3(copy_blocks(n * d)), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, (const float*)x_sorted,
                     (const float*)ldj_sorted, order, (const int64_t*)(ws + L.hist), sample_chunks(n), (int)n_flows, (const int64_t*)(ws + L.cdf), n, d,
                     x, ldj_or_null);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GBNF_ERR_HIP, "%s launch: %s", fn, hipGetErrorString(e));
  return GBNF_OK;
}

}  // extern "C"
