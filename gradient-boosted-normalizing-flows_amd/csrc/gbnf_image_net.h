// gbnf_image_net.h -- the fused image coupling-net kernel's launch interface (gbnf_image_net.hip), shared with gbnf_image.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace gbnf {

// epilogues of the image convolution kernels (img_conv_kernel, img_last_hx3_kernel, img_net_hx3_kernel)
enum { EPI_RELU = 0, EPI_STORE = 1, EPI_COUPLE_AFFINE = 2, EPI_COUPLE_ADD = 3, EPI_SPLIT = 4,
       // the z -> x direction (gbnf_image_flow_inverse): coupling^-1 and Split2d's re-draw of the half it dropped
       EPI_COUPLE_AFFINE_INV = 5, EPI_COUPLE_ADD_INV = 6, EPI_SPLIT_INV = 7,
       // the image trainer's deterministic mode: EPI_COUPLE_AFFINE / EPI_SPLIT whose waves STORE their log-det partials to per-image
       // slots (ConvLaunch::ldj, img_ldj_slots) instead of adding them into ldj[n]; img_launch_ldj_reduce adds the slots in order
       EPI_COUPLE_AFFINE_ORD = 8, EPI_SPLIT_ORD = 9,
       // gbnf_image_flow_encode: EPI_SPLIT / EPI_SPLIT_ORD that also STORE the standardised half the level drops,
       // eps = (z2 - mean) * exp(-log-var) -- the exact inverse of EPI_SPLIT_INV at temperature 1 -- to ConvLaunch::eps
       EPI_SPLIT_EPS = 10, EPI_SPLIT_EPS_ORD = 11 };

struct NetLaunch {
  const float* pre_in;      // (n, *, H, W) f32: the coupling net's input z1
  int64_t pre_in_img;
  const unsigned* pre_wp;   // f16x3 fragments of the first 3x3 with taps folded into k: [tile][pre_kc][hi|mid][64][4 u32]
  const float* pre_bias;    // [16 * tiles]
  const int* pre_koff;      // [32 * pre_kc] im2col offsets of the folded contraction for a 6-row staging (img_mid_hx3's table)
  int pre_kc, pre_cin;
  const unsigned* wp;       // 1x1: [o][c][hi|mid][64][4 u32]
  const float* bias;
  int n_mid;                // round 6: 1x1 layers between the two 3x3s (coupling_network_depth): 1, or 0 / 2 for hidden widths to 256
  const unsigned* wp2;      //   the second 1x1 (n_mid == 2), as wp
  const float* bias2;
  const unsigned* wp3;      // last 3x3: [o][tap][c][hi|mid][64][4 u32]
  const float* bias3;
  float* st;                // coupled half z2 (n, *, H, W) f32, first channel of image 0
  int64_t st_img;
  float* ldj;
  int hid, chp, cout, H;
  int inverse;              // 1: the coupling's way back (models/glow.py:349-355): z2 - h, or z2 / scale - shift; no log-det
  int Hv, Wv;               // the map proper inside its H x W storage (gbnf_image.hip, ConvLaunch): rows < Hv, columns < Wv
  unsigned bf_off;          // byte offset of the first 3x3's B-fragment buffer in LDS (set by img_net_hx3_launch)
  unsigned long long* sat;  // per-device counter of workgroups that met an operand beyond the fp16 range, or null
  unsigned* mark;           // (n,) per-image marks (non-zero: re-evaluate this image on the exact-f32 path), or null
  const unsigned* only;     // repair launches: (n,) run only images whose entry is non-zero; null = all
  int ldj_stride;           // the evaluation handle's deterministic mode (0 = the atomic form): ldj is this launch's first slot of image
                            //   0 in an (n, ldj_stride) array of log-det slots -- wave w of workgroup s of image n STORES its partial
                            //   to slot s * 8 + w (zero if it ran no epilogue) instead of adding it into ldj[n]
  unsigned long long* dbg;  // diagnostic builds (-DGBNF_IMG_STAMPS) only: [workgroup][wave][8] phase cycle sums
};

// LDS bytes of img_net_hx3_kernel for W-wide maps (16 | 8), hidden width padded to chp, cin input channels of the first 3x3
// in pre_kc 32-wide chunks of its folded contraction, cout outputs of the last 3x3; 0 = this geometry has no fused kernel
size_t img_net_hx3_lds(int W, int chp, int cin, int pre_kc, int cout);
// One launch for n images (W = H = 16 | 8): grid n * (W == 16 ? 2 : 1) workgroups of 512 threads (hidden widths above 256: n * 4
// workgroups on 16-wide maps).
hipError_t img_net_hx3_launch(const NetLaunch& q, int W, bool additive, int64_t n, hipStream_t s);
// log-det slots per image of such a launch (NetLaunch::ldj_stride): workgroups per image x 8 waves
int img_net_hx3_ldj_slots(int W, int chp);

// One launch of img_conv_kernel (gbnf_image.hip): an implicit-GEMM convolution of n images, strip by strip.
struct ConvLaunch {
  const float* in;        // (n, *, H, W): first input channel of image 0
  int64_t in_img;         // floats between images
  const float* wp;        // packed weights [OT][taps][KC][64][4]
  const float* bias;      // [OT*16]
  float* out;             // EPI_RELU / EPI_STORE: (n, *, H, W) first output channel of image 0
  int64_t out_img;
  float* st;              // EPI_COUPLE_* / EPI_SPLIT: the coupled half z2 (n, *, H, W), first channel of image 0
  int64_t st_img;
  float* ldj;             // (n,) accumulated with atomics (EPI_COUPLE_AFFINE / EPI_SPLIT); EPI_*_ORD: (n, slots) partials, slot
                          // (strip * o_split + osp) * IMG_WAVES + wave of image n is STORED by that wave (zero if it ran no epilogue)
  int ldj_stride;         // EPI_*_ORD: floats between the slot rows of two images; 0 = the launch's own slot count (the trainer's
                          // per-launch arrays).  The evaluation handle's deterministic mode keeps ONE (n, stride) array for the whole
                          // chain: ldj = this launch's first slot of image 0
  int cin, cout, H, W, ks, n_strips;
  int Hv, Wv;             // the map proper: rows < Hv, columns < Wv of the H x W storage (a 14 x 14 map lives in 16 x 16 storage;
                          // everything outside is ZERO in every tensor in HBM -- the 'same' padding of the map -- and stays so)
  float temperature;      // EPI_SPLIT_INV: z2 = mean + exp(log-var) * temperature * eps (models/layers.py:697)
  int c_chunk;            // input channels staged per pass (a multiple of 16; 0 = all: 3 x 3 convolutions from > 256 channels do not
                          // fit the LDS at once and stage their input in two halves; split-contraction form only)
  int o_split;            // workgroups sharing one strip, each with 1/o_split of the output tiles (fills the chip at small batch)
  // fused producer (1x1 convolutions only): the input of this convolution is relu(conv3x3(pre_in) + pre_bias), computed
  // for the strip straight into LDS instead of being read from `in` (the ConvNet's first layer never touches HBM)
  const float* pre_in;    // (n, *, H, W) first input channel of image 0, or null
  int64_t pre_in_img;
  const float* pre_wp;    // packed 3x3 weights [cin/16 tiles][9][pre_kc][64][4]
  const float* pre_bias;
  int pre_cin;
  float* eps;             // EPI_SPLIT_EPS*: this level's eps (n, cout/2, Hv, Wv) -- the map's own size, no storage padding --
  int64_t eps_img;        //   first channel of image 0, and the floats between images; only pixels of the map proper are stored
};

// ---- the evaluation path's kernels as the training path (gbnf_image_train.hip) launches them; defined in gbnf_image.hip.
// img_allow_lds: the convolution kernels' opt-in to 160 KB of dynamic LDS on the CURRENT device.  img_launch_conv: epi = EPI_RELU,
// EPI_STORE, EPI_COUPLE_AFFINE, EPI_COUPLE_ADD, EPI_SPLIT, EPI_COUPLE_AFFINE_ORD or EPI_SPLIT_ORD (false: another value); c_chunk
// and o_split are chosen here.  img_ldj_slots: the log-det slots per image of an EPI_*_ORD launch of that shape (cout output
// channels, n_strips strips, n images) -- n_strips * o_split * waves, with the o_split img_launch_conv chooses.
// img_launch_ldj_reduce: ldj[i] += part[i][0] + part[i][1] + ... in slot order, one thread per image.
hipError_t img_allow_lds();
bool img_launch_conv(int epi, const ConvLaunch& p, int n, hipStream_t s);
int img_ldj_slots(int cout, int n_strips, int64_t n);
void img_launch_ldj_reduce(const float* part, int slots, float* ldj, int64_t n, hipStream_t s);
void img_launch_pre(const float* x, const float* noise, float* out, float* ldj, int C, int H, int W, int Hi, int Wi, float bounds,
                    float ld_const, int64_t n, hipStream_t s);
void img_launch_squeeze(const float* in, int64_t in_img, float* out, int C, int H, int W, int Ho, int Wo, int64_t n, hipStream_t s);
void img_launch_unsqueeze(const float* in, float* out, int64_t out_img, int C, int H, int W, int Hs, int Ws, int64_t n, hipStream_t s);
void img_launch_embed(const float* z, float* out, int C, int H, int W, int Hv, int Wv, int64_t n, hipStream_t s);
void img_launch_final(const float* state, int64_t state_img, const float* prior, const float* ldj, float* ll, float* z, int C, int H, int W,
                      int Hv, int Wv, int64_t n, hipStream_t s);

}  // namespace gbnf
