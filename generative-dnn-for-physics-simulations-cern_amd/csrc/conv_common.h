// Shared host/device definitions of the implicit-GEMM convolution kernels (conv_igemm_kernel.h, built in
// conv_igemm_bf16.hip / conv_igemm_f32.hip: the generic / register-staged and first LDS-DMA kernels;
// conv_ring_kernel.h, conv_persist.hip, conv_mfma.hip: the 8-wave LDS-DMA ring kernels) and of their host
// dispatchers (conv_host.hip, conv_ring_host.hip).  ConvArgs is passed by value to every conv kernel, so
// all of these files see one definition.
#pragma once
#include "common.h"

enum { MODE_FWD = 0, MODE_DGRAD = 1, MODE_WGRAD = 2 };

// Unsigned division by a run-time constant (x < 2^31): q = (umulhi(x, m) + x) >> l.
struct FastDiv {
  uint32_t m;
  int l;
};
static inline FastDiv mkdiv(uint32_t d) {
  FastDiv f;
  f.l = 0;
  while ((1ull << f.l) < d) ++f.l;
  f.m = (uint32_t)(((1ull << 32) * ((1ull << f.l) - d)) / d + 1);
  return f;
}
__device__ __forceinline__ int fdiv(int x, FastDiv f) {
  return (int)((__umulhi((uint32_t)x, f.m) + (uint32_t)x) >> f.l);
}

// Sub-pixel decomposition of a stride-1 conv over a x2 nearest-upsampled input (conv_ring_host.hip).
// Output pixels split into 4 parity classes c = 2a + b, (p - pad) mod 2 = a, (q - pad) mod 2 = b.
// Class c covers output rows p = p0[c] + 2u (u < ph[c]) and is a plain dh[c] x dw[c] conv on the
// SOURCE grid: y[p0 + 2u][q0 + 2v] = sum_{d,e} x[u + oh + d][v + ow + e] * W'_c[d][e] with
// W'_c[d][e] = sum of W[r][s] over r in {2d - a, 2d - a + 1}, s in {2e - b, 2e - b + 1} (in range).
struct SubPixel {
  int on;
  int ph[4], pw[4];      // class grid
  int p0[4], q0[4];      // first output row / column of the class
  int oh[4], ow[4];      // source row of (u, d) = u + oh + d
  int dh[4], dw[4];      // combined taps
  int tap0[5];           // prefix sums of dh*dw (packed weight blocks)
  int tile0[5];          // FWD: prefix sums of the classes' row tiles (per 8-image group)
};
void es_make_subpixel(const es_conv_desc_t& d, int row_tile, SubPixel& sp);

struct ConvArgs {
  FastDiv fC, fS, fK, fQ, fP, fWu, fHu, fUh, fUw, fRSK, fW, fH;
  int fold;            // DGRAD with integer upsample folded (rows on the source grid)
  es_conv_desc_t d;
  const void* a_src;
  const void* b_src;
  int64_t as[4];      // FWD: x strides;  DGRAD/WGRAD: dy strides
  int64_t bs[4];      // WGRAD: x strides
  void* out;
  int64_t os[4];      // FWD: y strides; DGRAD: dxu strides
  const float* bias;
  float beta;
  int out_bf16;
  int M, Ng, Kd;
  int k_per_split;
  int dense_f32_out;   // host: output is fp32, dense [M][Ng] and beta == 0 (split-K allowed)
  int splitk;          // FWD / DGRAD split over blockIdx.z: fp32 atomics into a zeroed dense output
  SubPixel sp;         // ring kernels: sub-pixel class geometry (sp.on)
  int ng;              // ring FWD/DGRAD: images per group of the row order (8, 16, 32 or 64)
  int vec_out;         // ring FWD/DGRAD: output rows channel-contiguous, 16-byte aligned, beta == 0
  float* stats_part;   // ring FWD: per-row-tile BatchNorm partials [tile][3][Ng] (count, mean, M2)
  int sp_tpc;          // ring SP FWD: 0 = class-major tile order; else class-interleaved with this
                       // many tiles per class (the 4 classes of the same source pixels adjacent)
  int sp_merge;        // ring SP FWD with 4 identical class geometries: ONE GEMM whose columns are
                       // (class, out-channel) (4*Ng columns; the classes share the source gather)
  // persistent DGRAD fused with the reduction pass of the BatchNorm backward that consumes its
  // output (es_conv2d_dgrad_bnred): x = the norm's input h (same layout as the dgrad output), its
  // dropout keep bits and statistics; per workgroup sums of dnorm and dnorm*xhat -> bnr_part
  const void* bnr_x;
  const uint8_t* bnr_keep;
  const float *bnr_mean, *bnr_invstd, *bnr_gamma, *bnr_beta;
  float bnr_scale, bnr_slope;   // dropout 1/(1-p) (1 without dropout), LeakyReLU slope
  int bnr_dfirst, bnr_drop;
  float* bnr_part;              // [workgroup][3][Ng] (slots 1, 2: the two sums)
  int det;                      // WGRAD (es_conv2d_wgrad_det): split z stores its raw tile into
                                // out (ConvCall::det_ws) + z * M * Ng instead of atomics; split-K FWD /
                                // DGRAD (es_conv2d_*_det): into det_ws + z * M * Ng
  float* det_ws;
  int prio;                     // split-fp32 ring kernels: waves 4-7 at s_setprio 1 (VALU arbitration)
  int nbase;                    // dynamic rows: the launch's first image within d.rows' count (chunks)
  int mslot;                    // generic kernels (device-side): the launch's M, the split partials' stride
  // FWD with a per-output-channel affine + activation epilogue (es_conv2d_fwd_affine: an eval-mode
  // BatchNorm folded by es_bn_fold, then LeakyReLU / ReLU): read only by the AFF instantiations
  const float *epi_scale, *epi_shift;
  int epi_act;
  float epi_slope;
};

// Images of the launch that carry data: d.N, or with dynamic rows (es_conv_desc_t.rows, a device
// count of the batch's live images) the part of [nbase, nbase + d.N) below that count.  Kernels
// skip the tiles / K-steps past it and read its images as zeros (buffer num_records).
__device__ __forceinline__ int conv_live(const ConvArgs& a) {
  if (a.d.rows == nullptr) return a.d.N;
  const int px = a.d.rows_px > 0 ? a.d.rows_px : 1;
  const int v = __builtin_amdgcn_readfirstlane(a.d.rows[0]) - a.nbase * px;
  const int img = (v + px - 1) / px;       // (pixel rows: the images holding a live one)
  return v <= 0 ? 0 : (img < a.d.N ? img : a.d.N);
}
// rows_px > 0: the live pixel rows (samples) of the launch, image-major; else INT_MAX (whole images)
__device__ __forceinline__ int conv_live_px(const ConvArgs& a) {
  if (a.d.rows == nullptr || a.d.rows_px <= 0) return 0x7fffffff;
  const int v = __builtin_amdgcn_readfirstlane(a.d.rows[0]) - a.nbase * a.d.rows_px;
  return v < 0 ? 0 : v;
}

// The generic GEMM kernels (conv_igemm_kernel.h) shrink their problem to the live images: M (FWD /
// DGRAD rows, image-major) or the K of a WGRAD (N*P*Q pixels).  mslot keeps the launch's M.
__device__ __forceinline__ void conv_live_gemm(ConvArgs& a, int mode) {
  a.mslot = a.M;
  if (a.d.rows == nullptr) return;
  const int nl = conv_live(a), npx = conv_live_px(a);
  if (mode == MODE_WGRAD) a.Kd = min(nl * (a.Kd / a.d.N), npx);
  else a.M = min(nl * (a.M / a.d.N), npx);
}


// One call of a public conv entry (es_conv2d_*): what the caller asked for beyond the plain
// convolution, and what the launch path answers.  Host only: it lives on the stack of the C-ABI entry
// and is passed by reference down to the kernel launch.  A default-constructed value is a plain call.
struct ConvCall {
  // requests
  float* stats_part = nullptr;        // es_conv2d_fwd_stats: BatchNorm partials of the output, [chunk][3][Ng]
  int64_t stats_floats = 0;
  const es_affine_t* aff = nullptr;   // es_conv2d_fwd_affine: y = act(scale[k] * (acc + bias[k]) + shift[k])
  const void* bnr_x = nullptr;        // es_conv2d_dgrad_bnred: the consuming BatchNorm's input, statistics
  const es_norm_t* bnr_nm = nullptr;  // and chain, and the buffer of its backward's partial sums
  const es_chain_t* bnr_ch = nullptr;
  float* bnr_part = nullptr;
  int64_t bnr_floats = 0;
  float* det_ws = nullptr;            // es_conv2d_*_det: workspace of per-split partials (ordered sums)
  int64_t det_floats = 0;
  // results
  int stats_chunks = 0;   // partials a ring FWD launch wrote into stats_part (0: none)
  int bnr_chunks = 0;     // partials a DGRAD launch wrote into bnr_part (0: the request was declined)
  int det_splits = 0;     // partial slots written into det_ws (0: the kernel wrote the output itself)
  int aff_fused = 0;      // the kernel that ran applied the affine epilogue
  int path = 0;           // PATH_* bits of the kernels that ran (es_conv_exec_flops accounting)
};
enum { PATH_RING = 1, PATH_SPLIT = 2, PATH_SUBPIXEL = 4, PATH_THIN = 8 };   // (SPLIT: split-fp32 planes)

// rows of a DGRAD over n images: the source grid when the integer upsample is folded into the GEMM
inline int64_t dgrad_rows(const es_conv_desc_t& d, int n) {
  return (int64_t)n * (d.up_h > 0 ? d.H * d.W : d.Hu * d.Wu);
}

// the fp32 MFMA arithmetic level of the ring kernels (es_conv_set_f32_split: 0 exact, 2 split-fp32)
int es_f32_split_level();

// split-fp32 weight planes: byte offset of the planes behind an fp32 packing of n elements
extern "C" int64_t es_weight_planes_offset(int64_t n);

// 8-wave LDS-DMA ring kernels (conv_ring_host.hip plans and launches them).  Return 1 when the call was launched, 0 when the
// shape is not eligible (the caller falls back to the kernels of conv_igemm_kernel.h), <0 on error.
int es_conv_ring_launch(ConvArgs& a, int mode, ConvCall& call, hipStream_t st);
// fp32 operands (parity mode): FWD / DGRAD ring kernels over image chunks (same return convention)
int es_conv_ring_launch_f32(ConvArgs& a, int mode, ConvCall& call, hipStream_t st);
// deterministic fp32 WGRAD on the ring (conv_ring_host.hip, conv_mfma.hip): partial floats needed (-1: not eligible), and
// the launch (partials in call.det_ws + ordered reduce into the torch-layout dW; 1 done, 0 not eligible,
// < 0 error)
int64_t es_wgrad_f32_ring_floats(const es_conv_desc_t& d, const int64_t ys[4], const int64_t xs[4]);
int es_wgrad_f32_ring(const es_conv_desc_t& d, const void* dy, const int64_t ys[4], const void* x,
                      const int64_t xs[4], float* dw, float beta, ConvCall& call, hipStream_t st);
// the wave-specialised split-fp32 WGRAD partial kernel (conv_wgrad_ws.hip), 128 x bn tiles over grid
// (row tiles, column tiles, K splits); 1 launched, 0 not eligible
int es_wgrad_ws_launch(int bn, bool sp, dim3 grid, const ConvArgs& a, float* wsc, int ngt, hipStream_t st);
// ordered sum of per-split partials ws[split][K][R*S*C] into dW (torch layout [K][C][R][S])
void es_wgrad_reduce_plain(const float* ws, int splits, int K, int C, int R, int S, float* dw, float beta,
                           hipStream_t st);
