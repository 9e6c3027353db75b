/*
 * expertsim_hip.h — C ABI of the MI355X (gfx950) kernels behind the expertsim GAN training step.
 *
 * The reference (patrick-bedkowski/Generative-DNN-for-Physics-Simulations-CERN) has no FFI: its
 * hot path is PyTorch ATen ops dispatched from Python.  This header is the boundary the build
 * puts underneath the reference's own Python API (expertsim.models.* forward signatures and
 * MoEWrapper.train_step); each entry point replaces the ATen ops named at it,
 * with the reference call site cited as file:line (paths relative to the reference root).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the comment says otherwise; kernels never allocate,
 *    free or synchronise; everything is enqueued on `stream` (a hipStream_t);
 *  - tensors are described logically as (n, c, h, w) with element strides s[4] — the device layout
 *    (NHWC for conv activations, [rows][features] for linear activations) is the caller's choice;
 *  - return 0 (ES_OK) or an error code; es_last_error() gives the message (thread-local);
 *  - dtypes: ES_F32 (fp32 parity mode) and ES_BF16 (bf16 operands, fp32 accumulation).
 */
#ifndef EXPERTSIM_HIP_H
#define EXPERTSIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { ES_F32 = 0, ES_BF16 = 1 } es_dtype_t;
enum { ES_OK = 0, ES_ERR_ARG = 1, ES_ERR_HIP = 2, ES_ERR_UNSUPPORTED = 3 };
enum { ES_ACT_NONE = 0, ES_ACT_RELU = 1, ES_ACT_LRELU = 2 };
enum { ES_NORM_NONE = 0, ES_NORM_BN = 1, ES_NORM_GN = 2, ES_NORM_LN = 3 };

typedef void* es_stream_t; /* hipStream_t */

/* Logical 4-D view: element (n,c,h,w) lives at base + n*s[0] + c*s[1] + h*s[2] + w*s[3].
 * rows (optional, device int32): the LIVE batch count of a capacity-sized tensor.  A multi-expert
 * step keeps each expert's activations in buffers of n = capacity images and the expert's image
 * count on the device (es_expert_plan), so the step issues the same launches whatever the routing
 * (no host synchronisation, one captured graph): every kernel given a view / descriptor with rows
 * set works on images [0, min(rows[0], n)) only — images at or past it are neither read nor
 * written and take no part in any reduction (BatchNorm statistics, weight gradients, losses).
 * NULL: all n images (reference moe.py:121-207 runs each expert on exactly its B_e samples). */
typedef struct {
  int n, c, h, w;
  int64_t s[4];
  const int32_t* rows;
} es_view_t;

/* Counter-based dropout (expertsim/utils/philox.py).  keep(i) = (philox(seed, stream, i + index_offset)
 * >> 8) < threshold, i = NCHW-logical element index; kept values are multiplied by `scale` = 1/(1-p).
 * With step_ptr set, the stream used is stream + step_ptr[0] * step_mul, read on the device: a
 * captured HIP graph then draws fresh masks at every replay (the train step's step counter).
 * index_offset: logical index of this tensor's first element within the global batch (data-parallel
 * rank r holding samples [n0, n0 + n) of an expert's batch passes n0 * C*H*W), so every rank draws
 * exactly the single-device masks of its samples.  Must keep i + index_offset 4-aligned wherever i is
 * (a multiple of 8 for C % 8 == 0 layers). */
typedef struct {
  uint64_t seed;
  uint32_t stream;
  uint32_t threshold;
  float scale;
  int enabled;
  const int32_t* step_ptr; /* device int32 or NULL */
  int32_t step_mul;
  uint64_t index_offset;
  const int32_t* index_ptr; /* optional device int32: index_offset += index_ptr[0] * index_mul (a
                               data-parallel rank's first sample of the expert, known on the device) */
  int64_t index_mul;
} es_dropout_t;

const char* es_last_error(void);
int es_version(void);
int es_device_sync(void); /* hipDeviceSynchronize, for tests only */

/* ------------------------------------------------------------------------------------------
 * Convolution / linear as MFMA implicit GEMM.
 * Replaces aten::convolution / convolution_backward and aten::addmm / mm for nn.Conv2d and
 * nn.Linear (neutron/generator.py:11,17,24,29,33,37; neutron/discriminator.py:12,17,27,33,39;
 * neutron/aux_reg.py:13,20,27,34,45,68; proton/generator.py:14,19,27,33,38,41;
 * proton/discriminator.py:122,127,134,140,146; proton/aux_reg.py:20-30,61,104-117;
 * routers/router.py:12-19).  A Linear layer is the 1x1 convolution of a 1x1 image.
 * The nearest upsample feeding a generator conv (neutron/generator.py:23,29;
 * proton/generator.py:26,32) is folded into the input gather through hmap/wmap.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int N, C, H, W;   /* conv input (before upsample): batch, in-channels, height, width      */
  int Hu, Wu;       /* conv input after nearest upsample (== H, W when hmap/wmap are NULL)   */
  int K, P, Q;      /* out-channels, output height, output width                             */
  int R, S;         /* kernel height, width                                                  */
  int stride, pad;
  const int32_t* hmap; /* device [Hu]: source row of upsampled row (torch nearest), or NULL  */
  const int32_t* wmap; /* device [Wu]                                                        */
  int up_h, up_w;      /* integer nearest-upsample factors (Hu = H*up_h), or 0 to use the maps.
                          With factors set, es_conv2d_dgrad folds the upsample backward: it
                          writes dx on the SOURCE grid (H x W) with dxs strides.               */
  int subpixel;        /* 1: the packed weights are the sub-pixel combination of a x2 upsample
                          conv (es_pack_conv_weight mode 2 for fwd, 3 for dgrad) and the conv runs
                          as 4 parity-class convs on the source grid (es_conv_subpixel_ok).      */
  const int32_t* rows; /* optional device int32: live images of the N-capacity batch (es_view_t) */
  int rows_px;         /* > 0: rows counts SAMPLES that are the P*Q == rows_px pixels of each image
                          (a linear over 16-sample pixel blocks, layers.ConvOp._pixel_view): image i
                          pixel p is live when i*rows_px + p < rows[0]                             */
} es_conv_desc_t;

/* y[n,k,p,q] = bias[k] + sum_{c,r,s} xu[n,c,p*stride-pad+r,q*stride-pad+s] * W[k,c,r,s]
 * wk: packed weights [K][R][S][C] of dtype dt (es_pack_conv_weight, mode 0). bias may be NULL. */
/* Select the bf16 FWD/DGRAD main loop: 1 = LDS-DMA staged kernel where eligible (default),
 * 0 = register-staged kernel.  Both accumulate in the same order (bit-identical results); the
 * switch exists for A/B measurement and tests.  Returns the previous setting. */
int es_conv_set_glds(int on);
/* Select the 8-wave LDS-DMA ring kernels (conv_ring_kernel.h) for the bf16 convs whose K-step is one tap
 * x 64 channels: 1 = on (default), 0 = use the 4-wave kernels.  Returns the previous setting. */
int es_conv_set_ring(int on);
/* 256 x 256 ring tiles with 32-deep K-steps for sub-pixel FWD and DGRAD with >= 256 output channels:
 * 1 = on (default), 0 = 256 x 128 tiles (same accumulation order: bit-identical results).
 * Returns the previous setting. */
int es_conv_set_ring256(int on);
/* Persistent short-K DGRAD kernel (conv_persist.hip conv_persist_kernel: generator conv_layers.9's
 * dgrad, <= 8 K-steps of 64 channels, 64 or 128 output columns): 1 = on (default), 0 = the ring
 * kernel (same accumulation order: bit-identical outputs).  Only bit 0 of `on` is read.  Returns the
 * previous setting. */
int es_conv_set_persist(int on);
/* Persistent 256 x 256 kernel for the merged sub-pixel FWD (conv_persist.hip conv_p256_kernel:
 * generator conv_layers.0 / .5): 1 = on (default), 0 = the per-tile ring kernel (same accumulation
 * order: bit-identical outputs).  Returns the previous setting. */
int es_conv_set_p256(int on);
/* Sub-pixel decomposition of stride-1 convs over a x2 nearest upsample (conv_ring_host.hip): 1 = on
 * (default; wgrad uses it internally, fwd/dgrad when the caller packs mode 2/3 weights and sets
 * desc->subpixel), 0 = off.  Returns the previous setting. */
int es_conv_set_subpixel(int on);
/* 1 if es_conv2d_fwd / es_conv2d_dgrad can run this conv on the sub-pixel path (bf16, x2 integer
 * upsample, stride 1, channels % 64 == 0, tensors below 1 GiB, dense NHWC activations). */
int es_conv_subpixel_ok(const es_conv_desc_t* d, es_dtype_t dt);
/* Number of combined taps of the sub-pixel packing (16 for 3x3, 25 for 4x4): the packed weight
 * of mode 2 / 3 holds K * C * es_subpixel_taps(R, S) elements. */
int es_subpixel_taps(int R, int S);

int es_conv2d_fwd(const es_conv_desc_t* d, es_dtype_t dt, const void* x, const int64_t xs[4],
                  const void* wk, const float* bias, void* y, es_dtype_t ydt, const int64_t ys[4],
                  es_stream_t stream);
/* es_conv2d_fwd fused with the BatchNorm statistics of the stored y (torch batch_norm train mode,
 * neutron/generator.py:26,31,35): when the 8-wave ring kernel runs this conv, its epilogue also
 * writes per row tile and channel (count, mean, M2) partials to part [chunks][3][K] (part_floats
 * available) and *chunks > 0; es_norm_stats_finalize then merges them.  *chunks == 0 means y was
 * computed but no partials were written (use es_norm_stats). */
int es_conv2d_fwd_stats(const es_conv_desc_t* d, es_dtype_t dt, const void* x, const int64_t xs[4],
                        const void* wk, const float* bias, void* y, es_dtype_t ydt, const int64_t ys[4],
                        float* part, int64_t part_floats, int* chunks, es_stream_t stream);
/* Per-output-channel affine + activation applied to a conv's fp32 accumulator (indexed by output
 * channel k): an eval-mode BatchNorm (a per-channel affine of the running statistics, es_bn_fold)
 * and the LeakyReLU behind it, i.e. the reference's Conv / Linear -> BatchNorm -> Dropout (identity
 * in eval) -> LeakyReLU chains (neutron/generator.py:13-36) in model.eval(). */
typedef struct {
  const float* scale; /* [K] */
  const float* shift; /* [K] */
  int act;            /* ES_ACT_* */
  float slope;        /* LeakyReLU negative slope */
} es_affine_t;
/* es_conv2d_fwd with the epilogue y = act(scale[k] * (acc + bias[k]) + shift[k]) applied before the
 * rounding to ydt (evaluated as one fma with shift' = scale * bias + shift).  Replaces
 * aten::convolution / addmm + the eval-mode aten::native_batch_norm + leaky_relu of
 * neutron/generator.py:13-36 on the simulation path (train/utils.py:179-266).
 * *fused = 1: the kernel that ran applied the epilogue (the ring FWD kernels of conv_ring_kernel.h / conv_persist.hip, bf16
 * and split-fp32 operands).  *fused = 0: y holds the plain conv + bias output, bit-identical to
 * es_conv2d_fwd, and the caller runs es_norm_act_fwd with the running statistics.
 * d->rows / rows_px as es_conv2d_fwd: images past the live count are neither read nor written. */
int es_conv2d_fwd_affine(const es_conv_desc_t* d, es_dtype_t dt, const void* x, const int64_t xs[4],
                         const void* wk, const float* bias, const es_affine_t* epi, void* y, es_dtype_t ydt,
                         const int64_t ys[4], int* fused, es_stream_t stream);
/* dxu[n,c,hu,wu] = sum_{k,r,s} dy[n,k,p,q] * W[k,c,r,s] over (hu+pad-r) = p*stride, ...
 * (gradient w.r.t. the UPSAMPLED input; es_upsample_bwd folds it to the source grid).  With
 * integer factors d->up_h/up_w the fold happens inside the GEMM (K grows by up_h*up_w) and the
 * output is dx on the source grid.
 * wd: packed weights [C][R][S][K] (es_pack_conv_weight, mode 1).  beta=1 accumulates into dxu. */
int es_conv2d_dgrad(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4],
                    const void* wd, void* dxu, es_dtype_t dxdt, const int64_t dxs[4], float beta,
                    es_stream_t stream);
/* dw[k][r][s][c] += sum_{n,p,q} dy[n,k,p,q] * xu[n,c,...]   (fp32, split-K with atomics: the
 * caller zeroes dw first; es_unpack_conv_grad converts to torch's [K][C][R][S]). */
int es_conv2d_wgrad(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4],
                    const void* x, const int64_t xs[4], float* dw, es_stream_t stream);
/* Deterministic weight gradient (parity mode; replaces the same aten::convolution_backward weight
 * output as es_conv2d_wgrad): dw (torch layout [K][C][R][S], fp32) = beta * dw + dW, summed in a
 * fixed order.  The K splits store raw partials into ws (no float atomics), then one ordered reduce
 * (split, then sub-pixel class) writes dw; the result is bit-identical across runs and boxes.  fp32
 * ring shapes (channels % 64, dense NHWC) run the LDS-DMA ring kernel on v_mfma_f32_16x16x4_f32.
 * ws: es_conv2d_wgrad_det_ws_bytes(d, dt, ys, xs) bytes (-1: bad descriptor). */
int64_t es_conv2d_wgrad_det_ws_bytes(const es_conv_desc_t* d, es_dtype_t dt, const int64_t ys[4],
                                     const int64_t xs[4]);
int es_conv2d_wgrad_det(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4],
                        const void* x, const int64_t xs[4], float* dw, float beta, void* ws, int64_t ws_bytes,
                        es_stream_t stream);
/* Deterministic split-K (parity mode) of es_conv2d_fwd / es_conv2d_dgrad (beta 0): when the GEMM
 * has few output tiles and a long K (the generators' fc2 dgrad, K = 21632 / 92160), the K splits
 * store partials into ws and one ordered sum writes y / dx (fp32, dense), instead of float
 * atomics.  ws: es_conv2d_splitk_ws_bytes(d, mode) bytes (mode 0 FWD, 1 DGRAD). */
int64_t es_conv2d_splitk_ws_bytes(const es_conv_desc_t* d, int mode);
int es_conv2d_fwd_det(const es_conv_desc_t* d, es_dtype_t dt, const void* x, const int64_t xs[4], const void* wk,
                      const float* bias, void* y, es_dtype_t ydt, const int64_t ys[4], void* ws, int64_t ws_bytes,
                      es_stream_t stream);
int es_conv2d_dgrad_det(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4], const void* wd,
                        void* dxu, es_dtype_t dxdt, const int64_t dxs[4], void* ws, int64_t ws_bytes,
                        es_stream_t stream);
/* split-fp32 WGRAD with 128-row tiles: 1 (default) the wave-specialised kernel (waves 0-3 MFMA only,
waves 4-7 load + split), 0 the cooperative kernel (every wave loads, splits and multiplies); the
two give bitwise equal weight gradients.  Returns the previous setting.  Replaces nothing in the
reference (a kernel choice for ATen convolution_backward's weight gradient). */
int es_conv_set_wgrad_ws(int on);
/* Deterministic mode on / off (returns the previous setting): fp32 FWD / DGRAD take no split-K
 * float atomics, the generic norm backward's conv-bias sums become an ordered column reduction.
 * MoEWrapper turns it on in the fp32 parity mode (train.deterministic, default on). */
int es_set_deterministic(int on);
/* Test knob: ring convolutions (fp32 and bf16) launch over chunks of at most `images` images (0: only
 * as the 1 GiB operand limit requires); returns the previous value. */
int es_conv_set_f32_chunk(int images);
/* fp32 MFMA arithmetic of the ring convolutions (returns the previous setting): 0 = exact fp32
 * (v_mfma_f32_16x16x4_f32), any other value = split-fp32 (returned as 2): each fp32 operand is the exact sum of three bf16
 * planes and the six plane products with p + q <= 2 run on v_mfma_f32_16x16x32_bf16 into the fp32
 * accumulator (dropped terms < 2^-23 |a b| per product; deterministic, fixed order).  Replaces the
 * same fp32 conv2d / conv_transpose products as es_conv2d_fwd / _dgrad / _wgrad_det (neutron
 * generator.py:23-35, proton generator.py:26-38).  MoEWrapper sets it from train.fp32_mfma. */
int es_conv_set_f32_split(int on);
/* Split-fp32 FWD / DGRAD kernels read the packed weights' bf16 planes precomputed by
 * es_pack_weight_planes (the caller packs them whenever the split mode is set), and split only the
 * activations themselves.
 * Byte offset of the planes behind an fp32 packing of n elements, and the planes themselves: each
 * 32-element block g of the packing -> 192 bytes at base + es_weight_planes_offset(n) + 192 g, three
 * planes of 32 bf16 (x0 = rne(x), x1 = rne(x - x0), x2 = x - x0 - x1), k-permuted as the ring
 * kernels' fragments.  Same weights as es_pack_conv_weight (neutron generator.py:24,29,33). */
int64_t es_weight_planes_offset(int64_t n);
int es_pack_weight_planes(const float* packed, int64_t n, void* base, es_stream_t stream);
/* Host-side count of MFMA conv kernels issued so far (ring / persistent / p256 / fp32 WGRAD).
 * Instrumentation only: lets a profiler state how many kernel launches one conv op was. */
int64_t es_conv_launch_count(void);
/* Host-side tally of the MFMA work the conv entry points (es_conv2d_fwd / _dgrad / _wgrad /
 * _wgrad_det and their _stats / _bnred / _det variants) issued, as executed FLOPs (2 per MAC):
 * out[0] on the bf16 pipe (bf16 operands, and split-fp32: 6 plane products per fp32 product),
 * out[1] on the fp32 MFMA (v_mfma_f32_16x16x4_f32), out[2] on the VALU (thin Cin/Cout = 1 convs).
 * A sub-pixel conv counts its 4 parity-class convs (es_subpixel_taps / (4 R S) of the reference's
 * MACs).  reset != 0 zeroes the tally after reading it.  Instrumentation only (bench.py's executed
 * step MFMA fraction); the same products as neutron generator.py:23-35 / proton generator.py:26-38. */
int es_conv_exec_flops(double out[3], int reset);

/* Weight packing for the implicit GEMM (fp32 master [K][C][R][S] -> dt).
 * mode 0: out[k][r][s][c] = w*scale ; mode 1: out[c][r][s][k] = w*scale.
 * mode 2 / 3 (sub-pixel, x2 upsample): for each parity class t = 2a + b the combined weights
 * W'_t[d][e] = sum of w[.][.][r][s] over r in {2d-a, 2d-a+1}, s in {2e-b, 2e-b+1} (within range),
 * d < ((a+R-1)>>1)+1, e < ((b+S-1)>>1)+1; mode 2: class blocks [K][d][e][C] one after another,
 * mode 3: out[c][tap][k] with tap = the classes' (d, e) taps in order.  col_perm must be NULL.
 * scale = (inv_scale ? 1/inv_scale[0] : 1)  — the spectral-norm division W/sigma
 * (torch.nn.utils.spectral_norm compute_weight) is folded here.
 * col_perm (optional, device [C*R*S] for R=S=1 linears): input column index permutation. */
int es_pack_conv_weight(const float* w, int K, int C, int R, int S, int mode,
                        const float* inv_scale, const int32_t* col_perm, void* out, es_dtype_t dt,
                        es_stream_t stream);
/* One weight packing of es_pack_conv_weight (scale 1, no column permutation), with the split-fp32
 * planes behind it when planes != 0 (es_pack_weight_planes); out is the packing's buffer. */
typedef struct {
  const float* w;
  int K, C, R, S, mode;
  int dt;     /* es_dtype_t of the packing */
  int planes; /* fp32 only: also write the bf16 planes at out + es_weight_planes_offset(n) */
  void* out;
} es_pack_job_t;
/* The packings of every layer of a module rebuilt after a weight update (MoE optimizer steps) in one
 * launch per 32 jobs instead of one or two per layout (jobs: host array).  Same values as
 * es_pack_conv_weight + es_pack_weight_planes per job; the large mode-1 transposes keep their
 * LDS-tiled kernel. */
int es_pack_conv_weights(const es_pack_job_t* jobs, int n, es_stream_t stream);
/* grad[k][c][r][s] = beta*grad + dw[k][r][s][c] * (inv_scale ? 1/inv_scale[0] : 1) */
int es_unpack_conv_grad(const float* dw, int K, int C, int R, int S, const int32_t* col_perm,
                        float* grad, float beta, es_stream_t stream);
/* as es_unpack_conv_grad (no permutation), then dw[] = 0: a persistent packed accumulator needs no
 * zero fill before the next es_conv2d_wgrad */
int es_unpack_conv_grad_clear(float* dw, int K, int C, int R, int S, float* grad, float beta,
                              es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Normalisation + dropout + activation (aten::native_batch_norm / native_group_norm /
 * native_layer_norm, aten::bernoulli_ + mul (nn.Dropout), leaky_relu / relu and their
 * backward).  One fused elementwise pass forward, reductions + one pass backward.
 * Stats groups: BN -> channel c (count N*H*W), GN -> (n, c / (C/groups)), LN -> n (count C*H*W).
 * gamma/beta index: BN/GN -> c; LN -> (c*H + h)*W + w.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int kind;            /* ES_NORM_*                                                       */
  int groups;          /* GN only                                                         */
  const float* mean;   /* per stats group                                                 */
  const float* invstd; /* per stats group                                                 */
  const float* gamma;  /* may be NULL (identity)                                          */
  const float* beta;   /* may be NULL                                                     */
} es_norm_t;

typedef struct {
  es_dropout_t drop;
  int dropout_first; /* 1: act(drop(norm(x)))  [generator.py:13-15]; 0: drop(act(norm(x))) [aux_reg.py:15-17] */
  int act;           /* ES_ACT_*                                                          */
  float slope;       /* LeakyReLU negative slope (0.1 everywhere in the reference)        */
  uint8_t* keep;     /* optional device dropout keep bits, layout [n*h*w][c/8] (bit c%8 of byte
                        (row, c/8)), c % 8 == 0 required: es_norm_act_fwd writes the mask it draws,
                        es_norm_act_bwd then reads it instead of re-running Philox (same mask)   */
  int keep_ready;    /* 1: keep already holds this chain's mask (es_dropout_keep_bits, e.g. drawn on a
                        side stream ahead of the forward): es_norm_act_fwd reads it instead of
                        drawing it                                                                */
} es_chain_t;

/* Batch statistics of x (train-mode BN / GN / LN), written to mean/invstd per stats group.
 * For BN, running_mean/var (may be NULL) are updated with `momentum` and the unbiased
 * variance, as torch does.  ws: workspace of es_norm_stats_ws_bytes() bytes. */
int64_t es_norm_stats_ws_bytes(const es_view_t* x, int kind, int groups);
int es_norm_stats(const es_view_t* x, es_dtype_t xdt, const void* xp, int kind, int groups,
                  float eps, float* mean, float* invstd, float* running_mean, float* running_var,
                  float momentum, void* ws, es_stream_t stream);
/* y = chain(norm(x) [+ addend]) ; addend may be NULL (residual add of proton/aux_reg.py:130) */
/* Merge BatchNorm partials [chunks][3][C] (count, mean, M2; es_conv2d_fwd_stats) into mean /
 * invstd and the running statistics (momentum, unbiased variance), as es_norm_stats does. */
int es_norm_stats_finalize(const float* part, int chunks, int C, float eps, float* mean, float* invstd,
                           float* running_mean, float* running_var, float momentum, es_stream_t stream);
int es_norm_act_fwd(const es_view_t* x, es_dtype_t xdt, const es_norm_t* nm, const es_chain_t* ch,
                    const es_view_t* addend, es_dtype_t adt, const void* addend_ptr, const void* xp,
                    const es_view_t* y, es_dtype_t ydt, void* yp, es_stream_t stream);
/* Backward of es_norm_act_fwd.  dy: gradient of y.  act_ref (optional): evaluate the activation
 * derivative on this stored tensor (the block output) instead of the recomputed pre-activation.
 * Writes dx (beta=1 accumulates), accumulates dgamma/dbeta (fp32, may be NULL) and, when dsum is
 * given (C <= 1024), the per-channel sum of dx (the gradient of a conv bias feeding the norm). */
int64_t es_norm_bwd_ws_bytes(const es_view_t* x, int kind, int groups);
int es_norm_act_bwd(const es_view_t* x, es_dtype_t xdt, const void* xp, const es_norm_t* nm,
                    const es_chain_t* ch, const es_view_t* dy, es_dtype_t dydt, const void* dyp,
                    const es_view_t* act_ref, es_dtype_t rdt, const void* refp,
                    const es_view_t* dx, es_dtype_t dxdt, void* dxp, float beta, float* dgamma,
                    float* dbeta, float* dsum, void* ws, es_stream_t stream);
/* es_conv2d_dgrad (beta 0) fused with the REDUCTION pass of the BatchNorm backward that consumes dx
 * (aten::native_batch_norm_backward's sums, neutron/generator.py:30-33: conv_layers.9's dgrad feeds
 * BatchNorm2d conv_layers.6 -> Dropout -> LeakyReLU): x = that norm's input (dx's layout), nm its
 * statistics, ch its dropout / activation chain with the forward's keep bits.  When the
 * persistent DGRAD kernel runs this conv, its epilogue writes per workgroup the sums of dnorm and
 * dnorm * xhat over the stored dx to part [chunks][3][C] (slots 1, 2; part_floats available) and
 * *chunks > 0 (then es_norm_act_bwd_sums finishes the backward); *chunks == 0: dx was computed
 * but no sums were written (use es_norm_act_bwd). */
int es_conv2d_dgrad_bnred(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4],
                          const void* wd, void* dx, es_dtype_t dxdt, const int64_t dxs[4], const void* x,
                          const es_norm_t* nm, const es_chain_t* ch, float* part, int64_t part_floats,
                          int* chunks, es_stream_t stream);

/* Rest of the BatchNorm backward after es_conv2d_dgrad_bnred produced its reduction sums
 * (sums_part [chunks][3][C], slots 1, 2): the finalize (a1, a2, dgamma += , dbeta +=) and the
 * apply pass of es_norm_act_bwd (dx, and dsum += sum(dx) per channel when dsum != NULL).  BN only,
 * dense NHWC x / dy / dx of one dtype; ws: es_norm_bwd_ws_bytes(x, BN, 1) bytes. */
int es_norm_act_bwd_sums(const es_view_t* x, es_dtype_t xdt, const void* xp, const es_norm_t* nm,
                         const es_chain_t* ch, const es_view_t* dy, es_dtype_t dydt, const void* dyp,
                         const es_view_t* dx, es_dtype_t dxdt, void* dxp, const float* sums_part, int chunks,
                         float* dgamma, float* dbeta, float* dsum, void* ws, es_stream_t stream);


/* Data-parallel (synchronised) BatchNorm: the batch statistics of the neutron generator's and aux
 * regressor's BatchNorms (neutron/generator.py:13,19,26,31,35; neutron/aux_reg.py:15-47) over the
 * GLOBAL batch, as one device computes them for the reference.
 *   es_norm_stats_merge: [chunks][3][C] (count, mean, M2) partials -> one [3][C] partial;
 *   es_norm_stats_local: the rank's [3][C] partial straight from x (ws: es_norm_stats_ws_bytes);
 * the caller all-gathers the ranks' [3][C] partials and finalizes them with es_norm_stats_finalize
 * (world partials -> mean / invstd / running stats).
 *   es_norm_bwd_sync phase 0: raw per-channel sums [2][C] (sum dnorm, sum dnorm*xhat) of the rank
 *   into `sums`, and the rank's dgamma / dbeta accumulation; the caller all-reduces `sums`;
 *   phase 1: dx from the global sums and the global row count `cnt` (+ dsum as es_norm_act_bwd);
 *   with cnt_mul (device float, dynamic rows) the count is cnt_mul[0] * cnt (cnt: per sample).
 * ws: es_norm_bwd_ws_bytes(x, ES_NORM_BN, 1). */
int es_norm_stats_merge(const float* part, int chunks, int C, float* out, es_stream_t stream);
int es_norm_stats_local(const es_view_t* x, es_dtype_t xdt, const void* xp, void* ws, float* out,
                        es_stream_t stream);
int es_norm_bwd_sync(int phase, const es_view_t* x, es_dtype_t xdt, const void* xp, const es_norm_t* nm,
                     const es_chain_t* ch, const es_view_t* dy, es_dtype_t dydt, const void* dyp,
                     const es_view_t* dx, es_dtype_t dxdt, void* dxp, float* sums, float cnt,
                     const float* cnt_mul, float* dgamma, float* dbeta, float* dsum, void* ws,
                     es_stream_t stream);

/* Plain elementwise chain without normalisation (router LeakyReLU, final ReLU, casts):
 * y = chain(x). And its backward dx = beta*dx + dchain(dy) evaluated at x (or act_ref). */
/* Draw the dropout keep bits of chain ch over x's geometry (n, c, h, w; dynamic rows: the live
 * samples of x->rows) into ch->keep -- the mask es_norm_act_fwd would draw for the same chain.  A
 * forward given the chain with keep_ready = 1 then reads them (reference: the nn.Dropout masks of
 * neutron/generator.py:13-36, drawn ahead of their layer; bit-identical to the in-pass draw). */
int es_dropout_keep_bits(const es_view_t* x, const es_chain_t* ch, es_stream_t stream);
int es_act_fwd(const es_view_t* x, es_dtype_t xdt, const void* xp, const es_chain_t* ch,
               const es_view_t* y, es_dtype_t ydt, void* yp, es_stream_t stream);

/* Per-channel sum over (n,h,w): out[c] = beta*out[c] + sum x (conv/linear bias gradients). */
int64_t es_channel_sum_ws_bytes(const es_view_t* x);
int es_channel_sum(const es_view_t* x, es_dtype_t xdt, const void* xp, float* out, float beta,
                   void* ws, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pooling / resampling / layout (aten::max_pool2d_with_indices(+_backward),
 * upsample_nearest2d_backward, adaptive_avg_pool2d, cat, copy_)
 * ---------------------------------------------------------------------------------------- */
/* max pool, kernel (kh,kw), stride (sh,sw), no padding, floor mode; idx: uint8 window argmax
 * (first max in row-major window order, as torch). */
int es_maxpool_fwd(const es_view_t* x, es_dtype_t dt, const void* xp, int kh, int kw, int sh, int sw,
                   const es_view_t* y, void* yp, uint8_t* idx, es_stream_t stream);
int es_maxpool_bwd(const es_view_t* dy, es_dtype_t dt, const void* dyp, const uint8_t* idx, int kh,
                   int kw, int sh, int sw, const es_view_t* dx, void* dxp, float beta,
                   es_stream_t stream);
/* Fused discriminator front (neutron/discriminator.py:11-15, proton/discriminator.py:121-125):
 * SNconv3x3 1->32 (+bias, weight w * 1/sigma[0]) -> GroupNorm(8, 32) -> LeakyReLU(slope) ->
 * MaxPool 2x2, one workgroup per image, the 32-channel conv map recomputed from the image in LDS
 * instead of stored.  img: fp32 [N][1][H][W] (element strides is[4]); H-2 and W-2 even,
 * H*W <= 2048.  Forward writes pooled [N][(H-2)/2][(W-2)/2][32] fp32 (dense NHWC), idx (same
 * shape, uint8 window argmax as es_maxpool_fwd) and the GN mean / invstd [N][8]. */
int es_dfront_fwd(const float* img, const int64_t is[4], int N, int H, int W, const float* w,
                  const float* sigma, const float* bias, const float* gamma, const float* beta, float eps,
                  float slope, float* mean, float* invstd, float* pooled, uint8_t* idx, es_stream_t stream);
/* Backward from dpooled (dense NHWC like pooled).  dx (optional, fp32 [N][1][H][W], strides dxs):
 * image gradient, written.  part: workspace of es_dfront_part_floats(N) floats.  dw (gradient of
 * W/sigma, [32][1][3][3]) is written; dbias / dgamma / dbeta are accumulated; each may be NULL. */
int64_t es_dfront_part_floats(int N);
int es_dfront_bwd(const float* img, const int64_t is[4], int N, int H, int W, const float* w,
                  const float* sigma, const float* bias, const float* gamma, const float* beta, float eps,
                  float slope, const float* mean, const float* invstd, const uint8_t* idx,
                  const float* dpooled, float* dx, const int64_t dxs[4], float* part, float* dw,
                  float* dbias, float* dgamma, float* dbeta, es_stream_t stream);
/* Fused discriminator front, both conv blocks (neutron/discriminator.py:11-24,
 * proton/discriminator.py:121-134): SNconv3x3 1->32 -> GroupNorm(8, 32) -> LeakyReLU -> MaxPool 2x2
 * -> SNconv3x3 32->16 -> GroupNorm(8, 16) -> LeakyReLU -> MaxPool (ph, pw) -> flatten (NCHW order),
 * one workgroup per image: the pooled 32-channel map and the 16-channel conv map stay in LDS (the
 * second conv on v_mfma_f32_16x16x4_f32), only the flattened features leave the chip.  Replaces
 * es_dfront_* + es_conv2d_fwd/dgrad/wgrad of conv_layers.4 + the GroupNorm / pool passes after it.
 * Weights are used as w * (1/sigma[0]) (sigma may be NULL: 1). */
typedef struct {
    const float* w1; const float* sigma1; const float* b1; const float* g1; const float* be1;  /* [32][1][3][3], GN(8,32) */
    const float* w2; const float* sigma2; const float* b2; const float* g2; const float* be2;  /* [16][32][3][3], GN(8,16) */
    float eps1, eps2, slope;
    int ph, pw;                       /* second pool window = stride (neutron 2x2, proton 2x1) */
    const int32_t* rows;              /* optional device int32: live images of the N-image capacity */
} es_dfront2_params_t;
/* 1 when the fused path supports this geometry (H*W <= 2048, H-2 and W-2 even, pooled map <= 448
 * pixels, second conv map <= 368 pixels) */
int es_dfront2_ok(int H, int W, int ph, int pw);
/* Forward.  img fp32 [N][1][H][W] (strides is).  Writes feat[n*feat_stride + f], f < 16*Hq*Wq
 * (the reference's view(B, -1) order) and stats [N][32] = GN1 mean[8], invstd[8], GN2 mean[8],
 * invstd[8].  save (optional; required by the backward): [N][es_dfront2_save_floats] floats of
 * per-image activations the backward reads instead of recomputing them. */
int64_t es_dfront2_save_floats(int H, int W, int ph, int pw);
int es_dfront2_fwd(const float* img, const int64_t is[4], int N, int H, int W, const es_dfront2_params_t* p,
                   float* stats, float* feat, int64_t feat_stride, float* save, es_stream_t stream);
/* Backward from dfeat (the gradient of the features, same indexing as feat), with the forward's
 * stats and save.  dx (optional): fp32 image gradient [N][1][H][W] (strides dxs), written.  part
 * (optional, es_dfront2_part_floats(N) floats): per-image weight-gradient partials; when given,
 * dw1 / dw2 (gradients of W/sigma, torch layouts) are written and db*, dg*, dbe* (biases, GN
 * affines) accumulated; each may be NULL. */
int64_t es_dfront2_part_floats(int N);
int es_dfront2_bwd(const float* img, const int64_t is[4], int N, int H, int W, const es_dfront2_params_t* p,
                   const float* stats, const float* save, const float* dfeat, int64_t dfeat_stride, float* dx,
                   const int64_t dxs[4],
                   float* part, float* dw1, float* db1, float* dg1, float* dbe1, float* dw2, float* db2,
                   float* dg2, float* dbe2, es_stream_t stream);
/* Fused fc tail of the spectral-norm discriminator (neutron/discriminator.py:26-48,
 * proton/discriminator.py:136-158): SNLinear F->128 -> LayerNorm(128) -> LeakyReLU -> SNLinear
 * 128->64 -> LayerNorm(64) -> LeakyReLU (latent) -> SNLinear 64->1, 16 samples per workgroup, fp32
 * (v_mfma_f32_16x16x4_f32), weights used as w * (1/sigma[0]) (sigma may be NULL: 1).  Replaces the
 * es_conv2d_* / es_norm_* / es_pack_conv_weight launches of those layers. */
typedef struct {
    const float* w1; const float* sigma1; const float* b1; const float* g1; const float* be1;  /* [128][F], LN(128) */
    const float* w2; const float* sigma2; const float* b2; const float* g2; const float* be2;  /* [64][128], LN(64) */
    const float* w3; const float* sigma3; const float* b3;                                    /* [1][64] */
    float eps1, eps2, slope;
    const int32_t* rows;   /* optional device int32: live samples of the B-sample capacity */
} es_dmlp_params_t;
/* Forward over X [B][F] (row stride xs): writes h3 [B][128] (fc1 output), s3 [B][2] (LN1 mean,
 * invstd), h4 [B][64], s4 [B][2], lat [B][64] (the latent) and out [B] (the logit). */
int es_dmlp_fwd(const float* X, int64_t xs, int B, int F, const es_dmlp_params_t* p, float* h3, float* s3,
                float* h4, float* s4, float* lat, float* out, es_stream_t stream);
/* Backward from dout [B] and / or dlat [B][64] (either may be NULL) with the forward's saved
 * values.  dX (optional, row stride dxs): the fc1 input gradient, written.  part (optional,
 * es_dmlp_part_floats(B, F) floats): per-workgroup partials; when given, dw1 / dw2 / dw3 (gradients
 * of W/sigma, torch layouts) are written and the bias / LayerNorm-affine gradients accumulated;
 * any output may be NULL. */
int64_t es_dmlp_part_floats(int B, int F);
int es_dmlp_bwd(const float* X, int64_t xs, int B, int F, const es_dmlp_params_t* p, const float* h3,
                const float* s3, const float* h4, const float* s4, const float* lat, const float* dout,
                const float* dlat, float* dX, int64_t dxs, float* part, float* dw1, float* db1, float* dg1,
                float* dbe1, float* dw2, float* db2, float* dg2, float* dbe2, float* dw3, float* db3,
                es_stream_t stream);
/* Nearest resize gather y[n, :, hu, wu] = x[n, :, hmap[hu], wmap[wu]] (torch upsample_nearest2d's index
 * maps; dense NHWC, C % 4 == 0 fp32 / % 8 bf16): the proton generator's 35x19 -> 56x30 resize feeding
 * conv_layers.5 (proton/generator.py:33-34), materialised so that the conv runs on the ring kernels. */
int es_upsample_fwd(const es_view_t* x, es_dtype_t dt, const void* xp, const int32_t* hmap, const int32_t* wmap,
                    const es_view_t* y, void* yp, es_stream_t stream);
/* dx[n,c,h,w] = beta*dx + sum over upsampled positions mapping to (h,w).  hstart/hcount (device
 * [H]) and wstart/wcount (device [W]) describe the contiguous preimage of each source row/col.
 * Dense NHWC views with C % 4 == 0 take a vectorised kernel. */
int es_upsample_bwd(const es_view_t* dxu, es_dtype_t dt, const void* dxup, const int32_t* hstart,
                    const int32_t* hcount, const int32_t* wstart, const int32_t* wcount,
                    const es_view_t* dx, es_dtype_t dxdt, void* dxp, float beta, es_stream_t stream);
/* y = alpha*x (+ beta*y) elementwise between any two views of equal logical shape (also casts) */
int es_copy(const es_view_t* x, es_dtype_t xdt, const void* xp, const es_view_t* y, es_dtype_t ydt,
            void* yp, float alpha, float beta, es_stream_t stream);
/* global average pool over (h,w): y[n,c] (view (N,C,1,1)) and its backward */
int es_avgpool_fwd(const es_view_t* x, es_dtype_t dt, const void* xp, const es_view_t* y, void* yp,
                   es_stream_t stream);
int es_avgpool_bwd(const es_view_t* dy, const void* dyp, const es_view_t* dx, es_dtype_t dxdt,
                   void* dxp, float beta, es_stream_t stream);
/* rows gathered by index: dst[i,:] = src[idx[i],:] (fp32 rows of `cols`); idx NULL = identity */
int es_gather_rows(const float* src, int64_t src_ld, const int32_t* idx, int rows, int cols,
                   float* dst, int64_t dst_ld, es_stream_t stream);
/* Same with idx = perm + start[0], start read on the device (es_router_dispatch's offsets): the
 * per-expert gather of a multi-expert step (moe.py:121-143).  live (optional, device int32): only the
 * first live[0] of the `rows` (capacity) rows are gathered, the rest are written as zeros. */
int es_gather_rows_at(const float* src, int64_t src_ld, const int32_t* perm, const int32_t* start, int rows,
                      int cols, float* dst, int64_t dst_ld, const int32_t* live, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Spectral norm (torch.nn.utils.spectral_norm, n_power_iterations=1, eps=1e-12) for every
 * discriminator layer (neutron/discriminator.py:12,17,27,33,39; proton/discriminator.py:122,
 * 127,134,140,146).  One power iteration updates u,v in place and writes sigma = u.(W v).
 * sigma points to 1 + 2*(h + wd) floats: sigma[0], scratch, then a snapshot of the u [h] and
 * v [wd] this call used (what es_sn_bwd needs once the next call has updated u, v in place).
 * ---------------------------------------------------------------------------------------- */
/* active (optional, device int32): with active[0] == 0 the call computes sigma from the stored u, v
 * and updates nothing (an expert that does not train this step, moe.py:126-135). */
int es_sn_power_iter(const float* w, int h, int wd, float* u, float* v, float* sigma, int update,
                     const int32_t* active, es_stream_t stream);
/* es_sn_power_iter for n <= ES_SN_BATCH_MAX small layers (h*wd < 16384 each) in ONE launch; the
 * arrays are host arrays of device pointers / sizes, buf[i] as es_sn_power_iter's sigma buffer. */
#define ES_SN_BATCH_MAX 8
int es_sn_power_iter_batch(int n, const float* const* w, const int* h, const int* wd, float* const* u,
                           float* const* v, float* const* buf, int update, const int32_t* active,
                           es_stream_t stream);
/* es_sn_bwd for n <= ES_SN_BATCH_MAX small layers in ONE launch (host arrays of device pointers). */
int es_sn_bwd_batch(int n, const float* const* w, const float* const* g, const int* h, const int* wd,
                    const float* const* u, const float* const* v, const float* const* sigma, float* const* dw,
                    float beta, es_stream_t stream);
/* dW_orig = beta*dW_orig + G/sigma - (<G, W>/sigma^2) u v^T   (G = grad of W/sigma).
 * sigma is the buffer es_sn_power_iter wrote (1 + h + wd floats); its tail is used as scratch. */
int es_sn_bwd(const float* w, const float* g, int h, int wd, const float* u, const float* v,
              const float* sigma, float* dw_orig, float beta, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Losses (moe.py:506-642, proton/aux_reg.py:42-45, train/utils.py:623-642) and their gradients.
 * ---------------------------------------------------------------------------------------- */
/* Discriminator hinge (moe.py:518-523): out[0] = w*(mean relu(1-ro) + mean relu(1+fo));
 * dro/dfo = gradients of out[0].  w is read from device memory (w_ptr[0]) to avoid host syncs.
 * rows (optional, device int32): the live count of the n-capacity batch (0: out[0] = 0). */
int es_hinge_d(const float* ro, const float* fo, int n, const int32_t* rows, const float* w_ptr, float* out,
               float* dro, float* dfo, es_stream_t stream);
/* per-sample photon sum s[b] = sum_{h,w} (exp(x)-1) of the generated image (moe.py:611-616) */
int es_image_expsum(const es_view_t* x, es_dtype_t dt, const void* xp, float* s, es_stream_t stream);
/* Generator-step losses (moe.py:544-563): gen hinge, SDI diversity, intensity L1, log-cosh aux,
 * weighted by w.  Writes out[0..7] = {total, gen_hinge, div, intensity, aux, std_int, mean_int, w}
 * and gradients: dfo[n], dl1/dl2 [n,L], dcoord [n,2], coef[n] (= d total / d s[b]). */
typedef struct {
  int n, latent, noise;
  float di_strength, in_strength, aux_strength;
  const float* std_mean; /* optional device scalar: mean(std) over the expert's GLOBAL batch (data
                            parallel, SDI prefactor); NULL: the mean over these n samples */
  const int32_t* rows;   /* optional device int32: live samples of the n-capacity batch (0: metrics 0) */
} es_gen_loss_t;
int es_gen_losses(const es_gen_loss_t* p, const float* fo, const float* l1, const float* l2,
                  const float* n1, const float* n2, const float* std_, const float* s,
                  const float* intensity, const float* coord, const float* pos, const float* w_ptr,
                  float* out, float* dfo, float* dl1, float* dl2, float* dcoord, float* coef,
                  es_stream_t stream);
/* dimg[b,..] = beta*dimg + coef[b]*exp(x)   (intensity-term gradient of the generated image) */
int es_image_expsum_bwd(const es_view_t* x, es_dtype_t dt, const void* xp, const float* coef,
                        const es_view_t* dx, void* dxp, float beta, es_stream_t stream);

/* Router tail (routers/router.py:23 gumbel_softmax, moe.py:97-103 argmax/bincount):
 * gates = softmax((logits - log(e))/tau); idx = argmax; counts[E] (int32) */
int es_router_gumbel(const float* logits, const float* expo, int B, int E, float tau, float* gates,
                     int32_t* idx, int32_t* counts, es_stream_t stream);
/* Router loss gradient w.r.t. logits for the ALB term (train/utils.py:623-642, moe.py:407,429)
 * and the loss value: out[0] = coef*mean_e exp(1/(S_e+1e-6)), S_e = sum_b gates[b,e]. */
int es_router_alb(const float* gates, int B, int E, float tau, float coef, float* out,
                  float* dlogits, es_stream_t stream);
/* All router-loss terms that carry gradient (moe.py:258-268,407-434; train/utils.py:372-395
 * calculate_expert_distribution_loss, 398-419 calculate_expert_utilization_entropy, 623-642 ALB):
 * out[0] = alb_coef*mean_e exp(1/(S_e+1e-6)), the unweighted value the metric dict reports; its
 * gradient is weighted by dec_w (moe.py:424-434: the coefficient is (float)(alb_coef*dec_w), so
 * dec_w = 0 gives a finite out[0] and no ALB gradient); out[1] = util*sum_e avg_e*log(avg_e+1e-9)
 * (= -entropy*util, avg = S/B_total); out[2] = 0.1*ed/B_total*sum_{a,b: idx_a=idx_b} |feat_a - feat_b|
 * (cdist of the [B,1] per-sample photon sums, gated by the straight-through one-hot gates);
 * dlogits = d(sum of the three)/d logits through the Gumbel softmax, for the B rows of `gates`.
 * Data parallel: colsum = the all-reduced S_e (NULL: this call's rows), B_total = the global batch
 * (<= 0: B), feat_all / idx_all [B_all] = the all-gathered ED features (NULL: this call's rows); out
 * then holds this rank's share of the ED sum.  feat / idx may be NULL when ed_strength == 0. */
int es_router_loss(const float* gates, const int32_t* idx, const float* feat, int B, int E, float tau,
                   double alb_coef, double dec_w, float util_strength, float ed_strength, const float* colsum,
                   int B_total, const float* feat_all, const int32_t* idx_all, int B_all, float* out,
                   float* dlogits, es_stream_t stream);
/* Device-side expert dispatch (moe.py:121-123 `(idx == i).nonzero()` per expert, without the host
 * round trip): perm[B] = the batch rows grouped by expert, each group in batch order;
 * offs[E+1] = start of each group (offs[E] = B). */
int es_router_dispatch(const int32_t* idx, int B, int E, int32_t* perm, int32_t* offs, es_stream_t stream);
/* out[e] = sum_b gates[b, e] (the rank's share of the router's gate sums). */
int es_router_colsum(const float* gates, int B, int E, float* out, es_stream_t stream);
/* The train step's metric dict (moe.py:480-502) in one launch: out[11 + 8E] = gen, disc, div,
 * intensity, aux (means over the experts of mbuf [E][9] = per expert total, gen, div, int, aux,
 * std_int, mean_int, w, disc), router, ED, differentiation, entropy, ALB, gan (moe.py:255-434 from
 * rl = es_router_loss's out = [ALB, entropy, ED]; router = ED + gan + differentiation + entropy +
 * dec_w*ALB), then per expert gen_i, disc_i, div_i, int_i, aux_i, std_int_i,
 * mean_int_i, n_i (counts int32 or countsf float).  flags: 1 router (E > 1), 2 router trained this
 * epoch, 4 ALB on, 8 entropy on, 16 ED on. */
int es_step_metrics(const float* mbuf, int E, const float* rl, const int32_t* counts, const float* countsf,
                    float gan_strength, float diff_strength, float dec_w, int flags, float* out,
                    es_stream_t stream);
/* Data-parallel merge of the per-expert metric rows: rows [world][E][10] (the 9 metric columns of
 * MoEWrapper's buffer + the rank's sample count, 0 = not run) -> out [E][9], global-batch values. */
int es_dp_metrics_merge(const float* rows, int world, int E, float* out, es_stream_t stream);
/* dst[rows[i]] = src[i] for i < n (rows NULL: identity) -- moe.py:196-198 scatter of the
 * per-sample photon sums into the batch-ordered ED features. */
int es_scatter_rows(const float* src, const int32_t* rows, int n, float* dst, es_stream_t stream);
/* Same with the rows read from a dispatch permutation at a DEVICE start position (perm + start[0]),
 * so a captured per-expert graph stays valid whatever the expert's offset in a later step. */
int es_scatter_rows_at(const float* src, const int32_t* perm, const int32_t* start, int n, const int32_t* live,
                       float* dst, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer (torch.optim.Adam, created at train/training_setup.py:20-40, stepped at
 * moe.py:439,526,565,566): one launch over a flat fp32 parameter buffer.
 * ---------------------------------------------------------------------------------------- */
int es_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
            float beta2, float eps, int step, float grad_scale, es_stream_t stream);
/* Same update with the (1-based) step read on the device from step_ptr[0]; bias corrections
 * computed in the kernel (for captured train steps).  active (optional, device int32): no update when
 * active[0] == 0 (an expert skipped this step, moe.py:126-135). */
int es_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                float beta2, float eps, const int32_t* step_ptr, float grad_scale, const int32_t* active,
                es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Random numbers (torch.randn at moe.py:144,535; exponential_ inside F.gumbel_softmax):
 * Philox4x32-10 + Box-Muller, counter = element index.
 * ---------------------------------------------------------------------------------------- */
int es_randn(float* out, int64_t n, uint64_t seed, uint32_t stream_id, es_stream_t stream);
int es_rand_exponential(float* out, int64_t n, uint64_t seed, uint32_t stream_id,
                        es_stream_t stream);
/* Same draws with the stream id offset on the device: stream_id + step_ptr[0] * step_mul, and the
 * element counter starting at `offset` (out[i] = draw number offset + i; randn: offset even), so a
 * data-parallel rank draws exactly its rows of the single-device draw. */
int es_randn_dev(float* out, int64_t n, uint64_t seed, uint32_t stream_id, const int32_t* step_ptr,
                 int32_t step_mul, int64_t offset, es_stream_t stream);
int es_rand_exponential_dev(float* out, int64_t n, uint64_t seed, uint32_t stream_id,
                            const int32_t* step_ptr, int32_t step_mul, int64_t offset, es_stream_t stream);
/* es_randn_dev whose element offset adds off_ptr[0] * off_mul on the device (a data-parallel rank's
 * first sample of an expert, es_expert_plan n0; offsets even). */
int es_randn_dev_at(float* out, int64_t n, uint64_t seed, uint32_t stream_id, const int32_t* step_ptr,
                    int32_t step_mul, int64_t offset, const int32_t* off_ptr, int64_t off_mul, es_stream_t stream);
/* counter[0] += v on the device (step counters of a captured train step); the _if forms only when
 * flag[0] != 0 (flag NULL: always) -- an expert's optimizer steps and BatchNorm num_batches_tracked
 * counters advance only when it trains (moe.py:126-135). */
int es_counter_add(int32_t* counter, int32_t v, es_stream_t stream);
int es_counter_add_if(int32_t* counter, int32_t v, const int32_t* flag, es_stream_t stream);
int es_counter_add_i64_if(int64_t* counter, int64_t v, const int32_t* flag, es_stream_t stream);
/* es_counter_add_i64_if over n counters in one launch (host arrays of device pointers / addends): the
 * BatchNorm num_batches_tracked counts of one expert program (dynamic rows) applied together. */
int es_counters_add_i64_if(int64_t* const* counters, const int64_t* v, int n, const int32_t* flag,
                           es_stream_t stream);
/* Multi-expert step plan on the device (moe.py:97-135 without the host round trip): from counts [E]
 * (this rank's expert counts, es_router_gumbel) and, data parallel, counts_all [world][E] (all ranks'
 * counts, all-gathered on the device; NULL on one process), for each expert e: rows[e] = this rank's
 * live rows (its count if the expert trains -- global count > 1 -- and the count is >= min_local, else
 * 0), active[e] (the expert trains), n0[e] (this rank's first sample of the expert's global batch),
 * w[e] = float(count) / float(B) (class_counts_adjusted, moe.py:99-100), gcnt[e] (global count, float),
 * lcnt[e] (rows[e] as float). */
int es_expert_plan(const int32_t* counts, const int32_t* counts_all, int world, int rank, int E, int B,
                   int min_local, int32_t* rows, int32_t* active, int32_t* n0, float* w, float* gcnt,
                   float* lcnt, es_stream_t stream);
/* sizeof of the ABI structs (0 es_view_t, 1 es_dropout_t, 2 es_conv_desc_t, 3 es_norm_t, 4 es_chain_t,
 * 5 es_gen_loss_t, 6 es_dfront2_params_t, 7 es_dmlp_params_t, 8 es_pack_job_t, 9 es_affine_t;
 * -1 unknown): the bindings check their mirrors against it on load. */
int64_t es_struct_size(int which);
/* x[i] /= max(d[0], 1) for i < n (a sum over an expert's global batch -> its mean, d = the device count) */
int es_div_by(float* x, int n, const float* d, es_stream_t stream);
/* EMA of a flat parameter buffer — replaces EMAHelper.update (expertsim/train/loop.py:392-400):
 * shadow[i] = decay*shadow[i] + one_minus_decay*p[i], each product rounded, then one add. */
int es_ema_update(float* shadow, const float* p, int64_t n, float decay, float one_minus_decay,
                  es_stream_t stream);
/* dropout mask materialisation (tests): out[i] = keep(i) */
int es_dropout_mask(uint8_t* out, int64_t n, const es_dropout_t* d, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation (moe.py:644-692).
 * ---------------------------------------------------------------------------------------- */
/* 5-channel photon sums of x [n,1,h,w] (any strides): out[b*5 + k] (fp64) = sum over mask k+1 of
 * get_channel_masks (train/utils.py:18-59) as sum_channels_parallel (train/utils.py:62-78)
 * computes it; log_domain != 0 applies expm1 first (moe.py:646, train/utils.py:198). */
int es_channel_sums(const es_view_t* x, es_dtype_t dt, const void* xp, int log_domain, double* out,
                    es_stream_t stream);
/* 1-D Wasserstein-1 distances on the device -- replaces the scipy.stats.wasserstein_distance calls of
 * calculate_joint_ws_across_experts (train/utils.py:117-176), scipy's _cdf_distance with p = 1 term for term
 * (fp64; a fixed summation order, bitwise reproducible).
 * out[s * channels + c] = 1-D Wasserstein-1 distance between column c of the u rows and of the v rows
 * of segment s.  Segment s covers u rows u_idx[u_seg[2s] .. u_seg[2s+1]) (u_idx NULL: the rows
 * themselves) and likewise for v; segments may overlap (the joint distribution plus one per expert).
 * u_seg / v_seg / u_idx / v_idx are DEVICE int32 arrays: no host sync.  u_cap / v_cap: host upper bounds
 * of any segment's length (grid and workspace sizing).  A segment empty on either side gives 0
 * (the reference's `continue`, train/utils.py:117-176).
 * u is [u_rows][u_ld] fp64 (u_ld >= channels), u_idx (when given) has u_rows entries; segment bounds are
 * clamped to [0, u_rows], a segment's length to u_cap and every row index to [0, u_rows); likewise v.
 * Values must be finite.  u_cap + v_cap <= ES_WS_LDS_MAX: one launch, each problem sorted in LDS, no
 * workspace; up to 2^20: global-memory passes over `work` (es_wasserstein_1d_workspace bytes).  Above
 * that, or with too small a workspace: ES_ERR_ARG and nothing is launched. */
#define ES_WS_LDS_MAX 8192
size_t es_wasserstein_1d_workspace(int n_seg, int channels, int u_cap, int v_cap);
int es_wasserstein_1d(const double* u, int64_t u_ld, int u_rows, const int32_t* u_idx, const int32_t* u_seg,
                      const double* v, int64_t v_ld, int v_rows, const int32_t* v_idx, const int32_t* v_seg,
                      int n_seg, int channels, int u_cap, int v_cap, double* out,
                      void* work, size_t work_bytes, es_stream_t stream);
/* ES_WS_LDS_MAX of the built library (the largest u_cap + v_cap sorted in LDS) */
int es_wasserstein_lds_max(void);
/* Shower-shape observables of x [n,1,h,w] (any strides, fp32 / bf16) -- calculate_image_features and
 * get_max_value_image_coordinates (train/utils.py:81-112).  v = the pixel, or the float32 expm1 of it when
 * log_domain != 0 (the same expm1f as es_channel_sums / es_sim_finish).  feat[b*5 + k] (fp64), in the
 * reference's row order:
 *   0 max_x     max over columns j of sum_i v[i,j]     (np.max(np.sum(img, axis=0)))
 *   1 max_y     max over rows i of sum_j v[i,j]
 *   2 center_x  mean column index of the pixels with v > 0 (center_of_mass(img > 0)[1]); w / 2 without one
 *   3 center_y  mean row index of the pixels with v > 0; h / 2 without one
 *   4 nonzero   number of pixels with v > 0
 * peak[b*2 .. +1] = (row, col) of the first maximum in row-major order (np.unravel_index(np.argmax(img))).
 * Values must not be NaN.  Arithmetic (bitwise reproducible, no atomics, independent of n, of the image's
 * position in the batch and of the strides): each column sum is the fp64 sum over i = 0..h-1 in that
 * order and each row sum the fp64 sum over j = 0..w-1 in that order, both from +0.0; the index sums and
 * the count are integers; each centre is one fp64 division.  feat or peak may be NULL (not both).
 * 1 <= h, w <= 64; outside that, with c != 1, a NULL x / xp or both outputs NULL: ES_ERR_ARG and nothing is
 * launched.  n == 0: ES_OK without a launch. */
int es_image_features(const es_view_t* x, es_dtype_t dt, const void* xp, int log_domain,
                      double* feat /* [n,5] or NULL */, int32_t* peak /* [n,2] or NULL */,
                      es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Dataset preparation (the reference's notebooks calculating_diversity_for_data,
 * calculate_and_analysis_of_max_coordinates and data_filtering) -- csrc/prepare.hip.
 * ---------------------------------------------------------------------------------------- */
/* SDI-GAN diversity of condition groups over x [n,1,h,w] (any strides; x_f64 = 0: fp32 pixels, 1: fp64
 * pixels; fp32 is widened exactly, so the results are those of the fp64 arithmetic below on the widened
 * values).  Group g = the rows perm[offs[g] .. offs[g+1]) -- perm [n] / offs [n_groups + 1] are DEVICE int32
 * arrays in the layout es_router_dispatch produces: no host sync.  The bounds are clamped to [0, n], every
 * row index to [0, n).  With n_g the group's member count, per pixel p (fp64, no contraction):
 *   S = sum_k x[k,p]      over the members in perm order, from +0.0
 *   m = S / (double)n_g
 *   Q = sum_k d*d, d = x[k,p] - m   same order, from +0.0; the product is rounded, then added
 *   var = Q / (double)n_g           (the population variance, ddof = 0)      sd = sqrt(var)
 * n_g <= ES_PREP_SPLIT_MIN: both sums are one sequential chain.  Above: the members are cut into
 * ES_PREP_CHUNKS chunks [c L, min(n_g, (c+1) L)), L = ceil(n_g / ES_PREP_CHUNKS); each chunk is summed
 * sequentially from +0.0 and the chunk sums are added in chunk order from +0.0 (S and Q alike) -- a
 * function of n_g only.
 * group_sum[g] = sum_p sd[p] in this order, a function of h*w only: the pixels are cut into tiles of 128
 * (row-major pixel index; the last tile is padded with +0.0); inside a tile a[i] = sd[2i] + sd[2i+1],
 * i = 0..63, and the 64 values are combined by six butterfly steps a[i] <- a[i] + a[i ^ o],
 * o = 32, 16, 8, 4, 2, 1; the tile sums are
 * then added in tile order from +0.0.  An empty group gives var = 0 and group_sum = +0.0; a one-member
 * group gives exactly +0.0.  pix_var (optional) receives var per (group, pixel).
 * Bitwise reproducible; no float atomics; a group's result does not depend on n, on the other groups, on
 * the strides or on how many workgroups ran.  Values must be finite.
 * work: es_group_diversity_workspace(n_groups, h, w) bytes.  1 <= h*w <= 4096 and c == 1; outside that,
 * with a NULL x / xp / perm / offs / group_sum, x_f64 not 0 or 1, or too small a workspace: ES_ERR_ARG and
 * nothing is launched.  n == 0 or n_groups == 0: ES_OK without a launch. */
#define ES_PREP_SPLIT_MIN 256
#define ES_PREP_CHUNKS 16
size_t es_group_diversity_workspace(int n_groups, int h, int w);
int es_group_diversity(const es_view_t* x, int x_f64, const void* xp, const int32_t* perm,
                       const int32_t* offs, int n_groups, double* group_sum /* [G] */,
                       double* pix_var /* [G, h*w] or NULL */, void* work, size_t work_bytes,
                       es_stream_t stream);
/* Photon sum and peak of each image of x [n,1,h,w] (any strides, x_f64 as above):
 * sum[b] (fp64) = the sum of the image in this order: lane l of 64 adds the pixels with row-major index
 * l, l + 64, l + 128, .. in that order from +0.0, and the 64 lane sums are combined by the butterfly
 * a[i] <- a[i] + a[i ^ o], o = 32, 16, 8, 4, 2, 1 (np.sum of the image within h*w 2^-53 relative for
 * non-negative pixels).  peak[b*2 .. +1] = (row, col) of the first maximum in row-major order, compared in
 * the input's own precision (np.unravel_index(np.argmax(img), (h, w)); the reference's max_x is the row).
 * Values must be finite.  sum or peak may be NULL (not both).  1 <= h*w <= 4096 and c == 1; outside that,
 * with a NULL x / xp, both outputs NULL or x_f64 not 0 or 1: ES_ERR_ARG and nothing is launched.
 * n == 0: ES_OK without a launch. */
int es_image_sum_peak(const es_view_t* x, int x_f64, const void* xp, double* sum /* [n] or NULL */,
                      int32_t* peak /* [n, 2] or NULL */, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Expert diagnostics (the numbers behind the reference's specialisation plots: train/loop.py:234-329,
 * train/utils.py:470-620, utils/utils_eval.py:44-51; nothing is drawn) -- csrc/diagnostics.hip.
 * ---------------------------------------------------------------------------------------- */
/* Both entries read a value matrix x [rows][ld] (x_f64 = 0: fp32, 1: fp64; fp32 is widened exactly, so the
 * results are those of the fp64 arithmetic below on the widened values), of which the first `cols` columns
 * count (1 <= cols <= ES_DIAG_MAX_COLS, cols <= ld).  Segments follow es_wasserstein_1d: segment s covers
 * the rows idx[seg[2s] .. seg[2s+1]) (idx NULL: the rows themselves), in that order; seg [n_seg][2] and idx
 * [rows] are DEVICE int32 arrays: no host sync, everything runs on `stream`.  The bounds are clamped to
 * [0, rows], a segment's length to seg_cap (the host's upper bound of it: grid and workspace sizing) and every
 * row index to [0, rows).  Segments may overlap ("all rows" plus one per expert).  Values must be finite.
 * 0 <= rows <= 2^20, 1 <= seg_cap, n_seg <= 65535.  Outside the limits stated here and per entry, with a
 * NULL required pointer, x_f64 not 0 or 1 or too small a workspace: ES_ERR_ARG and nothing is launched.
 * rows == 0 or n_seg == 0: ES_OK without a launch and NOTHING is written -- the outputs, the counts
 * included, are then the caller's to initialise.
 *
 * The range of column c is lo = min, hi = max of x[0 .. rows)[c] over ALL rows (not the segments'): exact
 * and order-independent (integer min / max atomics on an order-preserving encoding of the doubles; whether a
 * zero comes out as -0.0 or +0.0 is unspecified).  linspace(lo, hi, num)[k], k = 0 .. num - 1, is
 * np.linspace's arithmetic, fp64, no contraction: div = num - 1; delta = hi - lo; step = delta / div;
 * value = (double)k * step + lo (product rounded, then added) -- or ((double)k / div) * delta + lo when
 * step == 0 -- and the last value (k = div, num > 1) is hi itself; num == 1 gives lo.  lo == hi gives num
 * equal values.
 *
 * es_segment_histogram.  counts[s][c][b] (int32) = the members of segment s whose column c falls into bin b
 * of the edges e = edges_out[c][0 .. bins], compared in fp64:
 *   right = 0   np.histogram(x, bins=e):                   e[b] <= x < e[b+1]; the last bin also holds
 *               x == e[bins].  With all edges equal every value lands in the last bin.
 *   right = 1   pd.cut(x, bins=e, include_lowest=True):    e[b] < x <= e[b+1]; bin 0 also holds x == e[0].
 *               With all edges equal every value lands in bin 0.
 * The bin is found by a binary search over the edges themselves, so it is the definition exactly (no
 * multiply-by-reciprocal estimate).  outside[s][c] counts the members below e[0] or above e[bins]; they are in
 * no bin (possible with caller-given edges only).  edges: a DEVICE array [cols][bins + 1], non-decreasing
 * per column, copied to edges_out; or NULL: edges_out[c] = linspace(lo_c, hi_c, bins + 1) of the column's
 * range.  edges_out is always written.  counts and outside are zeroed on the stream, then filled by
 * integer (vector) atomics on LDS and, to merge the workgroups of a segment, on global memory: order does not
 * matter, a rerun is bit-equal.
 * Limits: 1 <= bins and cols * (2 * bins + 1) <= ES_DIAG_HIST_MAX_CELLS (one workgroup's LDS holds the edges
 * and one histogram per column, at three workgroups per CU).  work: es_segment_histogram_workspace(cols, bins)
 * bytes (0: outside the limits), needed only when edges is NULL. */
#define ES_DIAG_MAX_COLS 64
#define ES_DIAG_HIST_MAX_CELLS 5120
size_t es_segment_histogram_workspace(int cols, int bins);
int es_segment_histogram(const void* x, int x_f64, int64_t ld, int rows, int cols, const int32_t* idx,
                         const int32_t* seg, int n_seg, int seg_cap, int bins, int right,
                         const double* edges /* [cols, bins + 1] or NULL */,
                         double* edges_out /* [cols, bins + 1] */, int32_t* counts /* [n_seg, cols, bins] */,
                         int32_t* outside /* [n_seg, cols] */, void* work, size_t work_bytes,
                         es_stream_t stream);
/* es_segment_kde.  1-D Gaussian kernel density estimate, scipy.stats.gaussian_kde(d, bw_method='scott'),
 * of the n members d_i of (segment s, column c) on the grid g = grid_out[c][0 .. points): the caller's
 * `grid` (DEVICE [cols][points], copied to grid_out) or, with grid NULL, linspace(lo_c, hi_c, points) of the
 * column's range, where lo == hi becomes lo - 1e-6, hi + 1e-6 first (train/utils.py:571-607).  fp64
 * throughout, no contraction, no float atomics.
 *   S = sum d_i, m = S / (double)n, Q = sum (d_i - m)^2 (product rounded, then added): es_group_diversity's
 *   fixed order, a function of n only -- n <= ES_PREP_SPLIT_MIN one sequential chain in member order from
 *   +0.0; above, ES_PREP_CHUNKS chunks [k L, min(n, (k+1) L)), L = ceil(n / ES_PREP_CHUNKS), each summed
 *   sequentially from +0.0, the chunk sums added in chunk order from +0.0.
 *   valid[s][c] = 0 when n < max(min_samples, 2) (the reference: 5), sqrt(Q / n) < std_eps (np.std,
 *   ddof = 0; the reference: 1e-12) or Q == 0 (no bandwidth): bw = 0, sd = 0 and the density row is NaN.  Otherwise valid = 1,
 *   sd = sqrt(Q / (n - 1)) (np.cov, ddof = 1), bw[s][c] = sd * pow((double)n, -0.2) (Scott; the device
 *   library's pow, within 16 ulp by the OpenCL bound it conforms to, plus one rounding for the product) and
 *   density[s][c][j] = T_j / (((double)n * bw) * sqrt(2 pi)),  T_j = sum_i exp(-0.5 * (z * z)),
 *   z = (g_j - d_i) * r, r = 1.0 / bw computed once (sqrt(2 pi) = 2.5066282746310002).
 *   T_j in a fixed order that is a function of n only: the members are cut into chunks of
 *   ES_DIAG_KDE_CHUNK in member order; each chunk is summed sequentially from +0.0 and the chunk sums are
 *   added in chunk order from +0.0.
 * A segment's result depends on its members, their order and the grid alone: not on rows, the other
 * segments, ld, idx against contiguous rows or the number of workgroups; a rerun is bit-equal.
 * sd (optional, [n_seg][cols]) receives sd.  Limits: 1 <= points <= ES_DIAG_KDE_MAX_POINTS, min_samples >= 0.
 * work: es_segment_kde_workspace(n_seg, cols, points, seg_cap) bytes (0: outside the limits): the range and
 * the chunk sums [n_seg][cols][ceil(seg_cap / ES_DIAG_KDE_CHUNK)][points] fp64. */
#define ES_DIAG_KDE_CHUNK 256
#define ES_DIAG_KDE_MAX_POINTS 1024
#define ES_DIAG_RANGE_BYTES 1024   /* the head of both workspaces: min / max keys [2][ES_DIAG_MAX_COLS] */
size_t es_segment_kde_workspace(int n_seg, int cols, int points, int seg_cap);
int es_segment_kde(const void* x, int x_f64, int64_t ld, int rows, int cols, const int32_t* idx,
                   const int32_t* seg, int n_seg, int seg_cap, int points,
                   const double* grid /* [cols, points] or NULL */, int min_samples, double std_eps,
                   double* grid_out /* [cols, points] */, double* density /* [n_seg, cols, points] */,
                   double* bw /* [n_seg, cols] */, int32_t* valid /* [n_seg, cols] */,
                   double* sd /* [n_seg, cols] or NULL */, void* work, size_t work_bytes, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Conditioning embeddings (the numbers behind the reference's plot_cond_pca_tsne, train/utils.py:422-467:
 * PCA(n_components=2) and TSNE(n_components=2, perplexity=30) of the conditions; nothing is drawn)
 * -- csrc/embedding.hip.
 * ---------------------------------------------------------------------------------------- */
/* The conventions of the expert diagnostics above: x [rows][ld] with unit column stride, of which the first
 * `cols` columns count (1 <= cols <= ES_DIAG_MAX_COLS, cols <= ld); every pointer is a DEVICE pointer; no
 * host sync, everything runs on `stream`.  Values must be finite.  Outside the limits stated here and per
 * entry, with a NULL required pointer or too small a workspace: ES_ERR_ARG before any launch, and
 * NOTHING is written.  There are no float atomics anywhere: every sum has an order that is a function of the
 * sizes only, so a rerun is bit-equal.
 *
 * es_pca_project.  x fp32 (x_f64 = 0; widened exactly) or fp64 (x_f64 = 1), 2 <= rows <= 2^20, 1 <= k <= cols.
 * fp64 throughout, no contraction:
 *   S_c = sum_r x[r][c], mean[c] = S_c / (double)rows;
 *   Q_ab = sum_r (x[r][a] - mean[a]) * (x[r][b] - mean[b])  (product rounded, then added), computed for a <= b
 *   and mirrored; cov[a][b] = Q_ab / ((double)rows - 1.0)   (ddof = 1: sklearn.decomposition.PCA(svd_solver=
 *   'full')'s explained_variance_).  Both sums run in es_group_diversity's fixed order, a function of rows only:
 *   rows <= ES_PREP_SPLIT_MIN one sequential chain in row order from +0.0; above, ES_PREP_CHUNKS chunks
 *   [k L, min(rows, (k+1) L)), L = ceil(rows / ES_PREP_CHUNKS), each summed sequentially from +0.0, the chunk
 *   sums added in chunk order from +0.0.
 *   The eigenpairs (lambda, v) of the symmetric cols x cols matrix cov come from cyclic Jacobi rotations in one
 *   workgroup, in row-cyclic order (p, q), p < q; a pair is skipped when cov_pq == 0 or
 *   |cov_pq| <= 2^-56 sqrt(|cov_pp| |cov_qq|); the sweeps end with the first sweep that rotates nothing (at most
 *   30).  Components are sorted by decreasing eigenvalue (equal eigenvalues: the lower Jacobi column first).
 *   Sign: sklearn's svd_flip(u_based_decision=False) -- the entry of largest magnitude of each component is
 *   positive, the first index wins a tie.
 *   components[m][c] (m < k), explained_variance[m] = lambda_m, explained_variance_ratio[m] = lambda_m / trace,
 *   trace = sum_c cov[c][c] in column order from +0.0 (0 when the trace is 0); mean[c];
 *   scores[r][m] = sum_c (x[r][c] - mean[c]) * components[m][c], columns in order from +0.0, the product rounded,
 *   then added.  A constant column is legal: its row and column of cov are exactly zero, no rotation touches
 *   them and its loading is zero in every component with a positive eigenvalue.
 * work: es_pca_project_workspace(cols) bytes (0: outside the limits): cov and the eigenvector matrix. */
size_t es_pca_project_workspace(int cols);
int es_pca_project(const void* x, int x_f64, int64_t ld, int rows, int cols, int k, double* scores /* [rows, k] */,
                   double* components /* [k, cols] */, double* explained_variance /* [k] */,
                   double* explained_variance_ratio /* [k] */, double* mean /* [cols] */, void* work,
                   size_t work_bytes, es_stream_t stream);
/* es_tsne_affinities.  The per-row scalars of t-SNE's input similarities
 * (sklearn.manifold._utils._binary_search_perplexity).  x fp32, 2 <= rows <= 2^17, 0 < perplexity < rows
 * (sklearn's rule).
 *   d_ij is DEFINED in fp32: acc = +0.0f; for c = 0 .. cols-1 in order: t = x[i][c] - x[j][c]; q = t * t;
 *   acc = acc + q (the product rounded, then added; no contraction).  So d_ij == d_ji bitwise, duplicate rows
 *   give exactly 0, and numpy float32 arithmetic reproduces it bit for bit.
 *   dmin_i = min_{j != i} d_ij (fp32, exact).  In fp64, with dd_ij = (double)d_ij - (double)dmin_i (exact):
 *   S_i(beta) = sum_{j != i} exp(-beta * dd_ij),   W_i(beta) = sum_{j != i} dd_ij * exp(-beta * dd_ij),
 *   H_i = log S_i + beta * (W_i / S_i).  The shifted form is the same distribution as sklearn's but cannot
 *   underflow to an empty row (S_i >= 1).  Order of both sums: thread t of 256 adds j = t, t + 256, .. in that
 *   order from +0.0; the 64 lane sums of a wave are combined by the butterfly a[l] <- a[l] + a[l ^ o],
 *   o = 32, 16, 8, 4, 2, 1; the four wave sums are added in wave order from +0.0.  exp and log are the device
 *   library's fp64 functions.
 *   Search: beta = 1, lower bound -inf, upper bound +inf; at most 100 evaluations; an evaluation with
 *   |H - log(perplexity)| <= 1e-5 ends the search; otherwise H too large: lower = beta, beta = beta * 2 while
 *   the upper bound is +inf, else (beta + upper) / 2; H too small: upper = beta, beta = beta / 2 while the
 *   lower bound is -inf, else (beta + lower) / 2.
 *   beta[i] = the beta of the LAST evaluation, log_s[i] = log S_i at that beta, dmin[i], steps[i] = the number
 *   of evaluations (1 .. 100).  They define the conditional p_{j|i} = exp(-beta_i dd_ij - log_s_i) (j != i) and
 *   the joint p_ij = (p_{j|i} + p_{i|j}) / (2 rows).
 *   A row whose nearest distance is shared by m >= perplexity points cannot reach the target (H -> log m): it
 *   ends with steps = 100 and a large finite beta (2^99 when no upper bound was ever found); that is the
 *   defined result, not an error. */
int es_tsne_affinities(const float* x, int64_t ld, int rows, int cols, double perplexity, double* beta /* [rows] */,
                       double* log_s /* [rows] */, float* dmin /* [rows] */, int32_t* steps /* [rows] */,
                       es_stream_t stream);
/* es_tsne_gradient / es_tsne_run.  Exact (all-pairs) t-SNE on the joint p_ij above, matrix-free: p_ij is
 * recomputed per pair, never stored.  y [rows][2] fp32 (dense).  With w_ij = 1 / (1 + |y_i - y_j|^2):
 *   Z = sum_{i != j} w_ij,   q_ij = max(w_ij / Z, DBL_EPSILON),
 *   g_i = 4 sum_j (a p_ij - q_ij) w_ij (y_i - y_j),
 *   KL = sum_{i != j} p_ij log(max(p_ij, DBL_EPSILON) / q_ij)     (no exaggeration in the KL).
 * The device evaluates the split form A_i = sum_j p_ij w_ij (y_i - y_j), R_i = sum_j w_ij^2 (y_i - y_j),
 * Zr_i = sum_j w_ij, K_i = sum_j p_ij (log max(p_ij, DBL_EPSILON) - log w_ij), P_i = sum_j p_ij, then
 * Z = sum_i Zr_i, g_i = 4 (a A_i - R_i / Z), KL = sum_i K_i + log(Z) sum_i P_i: identical except where the
 * clamp of q binds (w_ij / Z < DBL_EPSILON, an embedding 10^7 wide), where it differs by at most
 * 4 sum_j max(0, DBL_EPSILON - w_ij / Z) w_ij |y_i - y_j| per row.
 * Pair math is fp32 (v_exp_f32 and v_rcp_f32, 1 ulp each): b_i = fl32(beta_i log2 e) and
 * l_i = fl32(log_s_i log2 e + log2(2 rows)) (the fp64 expressions rounded once);
 * p_ij = exp2(-b_i (d_ij - dmin_i) - l_i) + exp2(-b_j (d_ij - dmin_j) - l_j) with d_ij as above (direct
 * differences: d_ij == 0 for duplicates); exp2 flushes results below 2^-126 to zero;
 * w_ij = rcp(1 + dy0^2 + dy1^2).  The pair j == i contributes exactly zero.
 * Order of the five (seven) row sums: fp32 along a tile of ES_TSNE_TILE consecutive columns j in j order from
 * +0.0f (a fused multiply-add per term where the target has one); the tile sums are added in fp64 in tile order
 * from +0.0; the columns are cut into n_s = min(ES_TSNE_MAX_SPLITS, ceil(rows / 256)) splits
 * [s L, min(rows, (s+1) L)), L = 4 ES_TSNE_TILE * ceil(ceil(rows / n_s) / (4 ES_TSNE_TILE)) (a split may be
 * empty; its tiles start at its first column),
 * and a row's split sums are added in split order from +0.0.  Sums over rows (Z, K, P, |g|^2): thread t of
 * 1024 adds the rows (elements) t, t + 1024, .. in that order from +0.0, then the wave butterfly of
 * es_tsne_affinities, then the 16 wave sums in wave order from +0.0.
 *
 * es_tsne_gradient writes g [rows][2] fp64 at the given y and a = exaggeration, and z_kl[0] = Z, z_kl[1] = KL.
 * es_tsne_run runs the iterations t = iter0 .. iter0 + n_iter - 1 on y in place with the same device code and
 * sklearn's _gradient_descent update, element-wise, fp64, no contraction.  State: upd, gains [rows][2] fp64
 * (before iteration 0 the caller zeroes upd and sets gains to 1).  With a = exaggeration and mu = momentum0
 * while t < exaggeration_iters, else a = 1 and mu = momentum1:
 *   inc = upd * g < 0;  gains = inc ? gains + 0.2 : gains * 0.8;  gains = max(gains, min_gain);
 *   upd = mu * upd - learning_rate * (g * gains);   y = (float)((double)y + upd).
 * sklearn's defaults: exaggeration 12, exaggeration_iters 250, momentum0 0.5, momentum1 0.8, min_gain 0.01,
 * learning_rate 'auto' = max(rows / exaggeration / 4, 50), check_every 50.  iter0 is the global index of the
 * first iteration, so a run can be split into calls: one call of n equals two calls that split it, bit for bit.
 * log: when (t + 1) % check_every == 0, and after the last iteration of the call, row t / check_every of
 * log [log_rows][2] fp64 receives (KL, |g|_2) of iteration t (at the y before its update; |g|_2 with that
 * iteration's a); log_rows > (iter0 + n_iter - 1) / check_every.  n_iter == 0: ES_OK without a launch.
 * sklearn's two early-stop rules (n_iter_without_progress, min_grad_norm) are NOT rebuilt: the run has no host
 * round trip, and sklearn itself ran 999 of 1000 iterations on the golden's data.
 * work: es_tsne_workspace(rows) bytes (0: outside the limits): the split sums [n_s][rows][8] fp64, g, three
 * scalars, b and l. */
#define ES_TSNE_TILE 32
#define ES_TSNE_MAX_SPLITS 16
size_t es_tsne_workspace(int rows);
int es_tsne_gradient(const float* x, int64_t ld, int rows, int cols, const double* beta, const double* log_s,
                     const float* dmin, const float* y, double exaggeration, double* g /* [rows, 2] */,
                     double* z_kl /* [2] */, void* work, size_t work_bytes, es_stream_t stream);
int es_tsne_run(const float* x, int64_t ld, int rows, int cols, const double* beta, const double* log_s,
                const float* dmin, float* y, double* upd, double* gains, int n_iter, int iter0,
                double exaggeration, int exaggeration_iters, double momentum0, double momentum1,
                double learning_rate, double min_gain, int check_every, double* log /* [log_rows, 2] */,
                int log_rows, void* work, size_t work_bytes, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Clustering (the proton sets' expert_number column: scikit-learn's KMeans(algorithm="lloyd"), k-means++) and
 * the confusion matrix behind the reference's evaluate_router (train/utils.py:299-310) -- csrc/cluster.hip.
 * ---------------------------------------------------------------------------------------- */
/* x [rows][ld] with unit column stride (x_f64 = 0: fp32, widened exactly; 1: fp64), of which the first `cols`
 * columns count.  1 <= rows <= ES_KMEANS_MAX_ROWS, 1 <= cols <= ES_KMEANS_MAX_COLS, cols <= ld,
 * 1 <= K <= ES_KMEANS_MAX_K, K <= rows.  Centres are fp64 [K][cols], dense.  Every pointer is a DEVICE pointer;
 * no host sync, everything runs on `stream`.  Values must be finite.  Outside the limits, with a NULL required
 * pointer, x_f64 not 0 or 1 or too small a workspace: ES_ERR_ARG before any launch, and nothing is written.
 * All arithmetic on values is fp64 without contraction; there are no float atomics and every sum has an order
 * that is a function of the sizes only, so a rerun is bit-equal.
 *
 * d(r, k), the squared distance of row r to centre k, is the sum of differences
 *   lane l of 64: a_l = +0.0; for c = l, l + 64, .. < cols in order: t = x[r][c] - centre[k][c]; q = t * t;
 *   a_l = a_l + q;  then the butterfly a[l] <- a[l] + a[l ^ o], o = 32, 16, 8, 4, 2, 1.
 * It is NOT the |x|^2 - 2 x.c + |c|^2 expansion scikit-learn uses: the difference form is translation invariant,
 * so scikit-learn's mean-centring of x (there to tame the expansion's cancellation) is unnecessary here, a row
 * equal to a centre is at distance exactly 0 and equal centres are at exactly equal distances.
 * sum_rows(v), a sum over the rows: chunks of 4096 rows; in a chunk thread t of 1024 adds the rows t, t + 1024,
 * t + 2048, t + 3072 in that order from +0.0, the 64 lane sums of a wave are combined by the butterfly above and
 * the 16 wave sums are added in wave order from +0.0; the chunk sums are added the same way (thread t adds the
 * chunks t, t + 1024, ..).
 *
 * es_kmeans_assign.  label[r] = the k of smallest d(r, k), the lowest k on a tie; dist[r] = that d;
 * changed[0] = the rows with label[r] != label_old[r] (label_old NULL, the first iteration: rows; label_old must
 * not be label); inertia[0] = sum_rows(dist).
 *
 * es_kmeans_update.  New centres from the labels (entries outside [0, K) are clamped), scikit-learn's M-step:
 *   S[k][c] = the sum of x[r][c] over the rows labelled k: the rows are cut into
 *   n_c = min(256, ceil(rows / 256), max(1, floor(2^24 / (K cols)))) chunks [i L, min(rows, (i+1) L)),
 *   L = ceil(rows / n_c); inside a chunk the rows are added in row order from +0.0, the chunk sums in chunk order
 *   from +0.0.  n[k] = the number of rows labelled k.
 *   Empty clusters (_relocate_empty_clusters_dense): the j-th empty cluster in ascending index takes the row p_j
 *   that is j-th in the order of descending dist, the lower row first on a tie; for j ascending,
 *   S[label[p_j]] -= x[p_j], n[label[p_j]] -= 1, S[empty_j] = x[p_j], n[empty_j] = 1; labels are not changed.
 *   scikit-learn leaves the order among SEVERAL empty clusters to np.argpartition; the rule here is pinned
 *   against scikit-learn for one empty cluster only.
 *   centres_new[k][c] = S[k][c] * (1.0 / (double)n[k]) (n[k] == 0: S[k][c] as it stands).
 *   shift[0] = sum_k sum_c (centres_new - centres_old)^2: per (k, 128-column tile) the butterfly over each of its
 *   two waves, wave 0 + wave 1; the K * ceil(cols / 128) tile sums, k-major, by lane l of 64 adding l, l + 64, ..
 *   from +0.0 and the butterfly.  centres_new must not be centres_old.  dist is es_kmeans_assign's, read only when
 *   a cluster is empty.
 * work: es_kmeans_workspace(rows, cols, K) bytes for both (0: outside the limits): the reduction chunks, the
 * update's chunk sums [n_c][K][cols] fp64 and its tile sums.
 *
 * es_kmeans_plusplus.  Greedy k-means++ (sklearn.cluster._kmeans._kmeans_plusplus) on the caller's uniform draws
 * u [K][trials] in [0, 1), trials = es_kmeans_trials(K) = 2 + (int)ln K for scikit-learn's rule (1 .. 8 accepted).
 *   index[0] = min(floor(u[0][0] * rows), rows - 1); closest[r] = d(r, x[index[0]]).
 *   Step s = 1 .. K-1: cum = the prefix sums of closest in this order: 1024 segments of Ls = ceil(rows / 1024)
 *   consecutive rows; local_i = the sequential sum of the segment's rows up to and including i, from +0.0;
 *   off_t = the segment totals added in segment order from +0.0; cum[i] = off_t + local_i (non-decreasing by
 *   construction); total = cum[rows - 1].  Candidate j < trials: v = u[s][j] * total,
 *   cand_j = min(the first i with cum[i] >= v, rows - 1) (np.searchsorted, side='left', clipped).
 *   pot_j = sum_rows(min(closest[r], d(r, x[cand_j]))); the candidate of lowest pot_j wins, the first on a tie;
 *   index[s] = cand_j, closest = that minimum.
 *   centres[s] = x[index[s]] widened.  d() uses the row as the centre: d(r, r) is exactly 0.
 * work: es_kmeans_plusplus_workspace(rows, cols, K) bytes: closest and eight candidates' distances.
 *
 * es_confusion_matrix.  counts[t][p] (int64 [n_true][n_pred]) = the pairs i < n with target[i] == t and
 * pred[i] == p; invalid[0] = the pairs with an index outside either range, which are in no cell.  Both are zeroed
 * on the stream and filled by integer adds only (an int32 LDS histogram per workgroup, then 64-bit integer
 * atomics on global memory), so the result does not depend on any order.  n == 0 is legal (all zeros).
 * 1 <= n_true * n_pred <= ES_CONFUSION_MAX_CELLS. */
#define ES_KMEANS_MAX_ROWS (1 << 24)
#define ES_KMEANS_MAX_COLS 4096
#define ES_KMEANS_MAX_K 64
#define ES_CONFUSION_MAX_CELLS 4096
int es_kmeans_trials(int K);
size_t es_kmeans_workspace(int rows, int cols, int K);
size_t es_kmeans_plusplus_workspace(int rows, int cols, int K);
int es_kmeans_assign(const void* x, int x_f64, int64_t ld, int rows, int cols, const double* centres /* [K, cols] */,
                     int K, const int32_t* label_old /* [rows] or NULL */, int32_t* label /* [rows] */,
                     double* dist /* [rows] */, int64_t* changed /* [1] */, double* inertia /* [1] */, void* work,
                     size_t work_bytes, es_stream_t stream);
int es_kmeans_update(const void* x, int x_f64, int64_t ld, int rows, int cols, const int32_t* label,
                     const double* dist, const double* centres_old, int K, double* centres_new /* [K, cols] */,
                     double* shift /* [1] */, void* work, size_t work_bytes, es_stream_t stream);
int es_kmeans_plusplus(const void* x, int x_f64, int64_t ld, int rows, int cols, int K,
                       const double* u /* [K, trials] */, int trials, double* centres /* [K, cols] */,
                       int32_t* index /* [K] */, void* work, size_t work_bytes, es_stream_t stream);
int es_confusion_matrix(const int32_t* pred, const int32_t* target, int64_t n, int n_true, int n_pred,
                        int64_t* counts /* [n_true, n_pred] */, int64_t* invalid /* [1] */, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sample-level fidelity and diversity: the k-nearest-neighbour radii and the counts behind precision / recall
 * (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020, the `prdc` package) -- csrc/fidelity.hip.
 * ---------------------------------------------------------------------------------------- */
/* x [rows][ld] fp32 with unit column stride, of which the first `cols` columns count.  1 <= rows <= ES_KNN_MAX_ROWS,
 * 1 <= cols <= ES_KNN_MAX_COLS, cols <= ld, 1 <= k <= ES_KNN_MAX_K, 1 <= n_seg <= ES_KNN_MAX_SEG,
 * 1 <= cap <= ES_KNN_MAX_ROWS.  Every pointer is a DEVICE pointer; no host sync, everything runs on `stream`.
 * Values must be finite.  Outside the limits, with a NULL required pointer or too small a workspace: ES_ERR_ARG
 * before any launch, and nothing is written.
 *
 * Segments follow es_wasserstein_1d: segment s of a side covers the rows idx[seg[2s] .. seg[2s+1]) (idx NULL: the
 * rows themselves); idx (when given) has `rows` entries; the bounds are clamped to [0, rows], a segment's length to
 * `cap` (the host upper bound that sizes grids, outputs and workspaces) and every row index to [0, rows).  Segments
 * may overlap (the joint distribution plus one per expert).  Lengths are read on the device: grids are sized from
 * `cap` and tiles past the live length exit.
 *
 * d2(a, b), the squared distance of two rows, is the sum of squared differences in column order:
 *   s = +0.0; for c = 0, 1, .., cols - 1 in order: t = (double)a[c] - (double)b[c]; q = t * t; s = s + q.
 * Every operation is rounded (no contraction, no FMA) and one pair's sum is walked by one thread, so d2 does not
 * depend on how the rows are tiled.  It is NOT the |a|^2 - 2 a.b + |b|^2 expansion scikit-learn uses, which cancels
 * exactly where these metrics matter (near-duplicate images of a collapsed generator): d2(a, a) is exactly 0,
 * d2(a, b) == d2(b, a) bitwise and equal rows are at equal distances from everything.
 *
 * es_knn_radius.  radius2[s][p] (fp64 [n_seg][cap]), p < L_s = the segment's length: the (k+1)-th smallest value of
 * the multiset { d2(x_p, x_q) : q in segment s }, q = p included (prdc's "k-th neighbour, self included at distance
 * 0").  L_s <= k: there is no such value and the entries p < L_s are +inf.  Entries at p >= L_s are not written.
 * Only the value is selected, so the result depends on neither the tiling nor the merge order.
 * work: es_knn_radius_workspace(n_seg, cap, k) bytes (0: outside the limits): the partial lists
 * [n_seg][cap][split][k + 1] fp64 when the other side's tiles are cut into split > 1 runs.
 *
 * es_prdc_count.  real / fake have their own ld / rows / idx / seg / cap and share cols and n_seg; r_radius2
 * [n_seg][r_cap] and f_radius2 [n_seg][f_cap] are es_knn_radius's of each side at the same segments.  For segment s
 * with real members p < n_r and generated members q < n_f:
 *   f_count[s][q] (int32 [n_seg][f_cap]) = #{ p : d2(r_p, f_q) < r_radius2[s][p] }
 *   r_hit[s][p]   (int32 [n_seg][r_cap]) = 1 if some q has d2(r_p, f_q) < f_radius2[s][q], else 0
 *   r_min2[s][p]  (fp64  [n_seg][r_cap]) = min_q d2(r_p, f_q)  (+inf when n_f == 0)
 *   totals[s]     (int64 [n_seg][8])     = { n_r, n_f, valid, precision_hits, recall_hits, density_pairs,
 *                                            coverage_hits, 0 }
 *     valid = (n_r > k && n_f > k); precision_hits = #{ q : f_count > 0 }; recall_hits = sum_p r_hit;
 *     density_pairs = sum_q f_count; coverage_hits = #{ p : r_min2 < r_radius2 }; all four are 0 when the segment
 *     is not valid (the per-row outputs follow the formulas whatever the radii hold).
 * Comparisons are strict and on squared distances (prdc compares the square roots: the same in exact arithmetic).
 * Entries at p >= n_r / q >= n_f are not written; f_count, r_hit and r_min2 may each be NULL.  Reductions are
 * integer adds / ors and minima of non-negative doubles (an unsigned integer minimum on the bit pattern), by vector
 * atomics on the workspace: no order matters and a rerun is bit-equal.  precision = precision_hits / n_f,
 * recall = recall_hits / n_r, density = density_pairs / (k n_f), coverage = coverage_hits / n_r are left to the host.
 * work: es_prdc_workspace(n_seg, r_cap, f_cap) bytes (0: outside the limits): the three per-row arrays. */
#define ES_KNN_MAX_K 16
#define ES_KNN_MAX_ROWS (1 << 20)
#define ES_KNN_MAX_COLS 4096
#define ES_KNN_MAX_SEG 65
size_t es_knn_radius_workspace(int n_seg, int cap, int k);
size_t es_prdc_workspace(int n_seg, int r_cap, int f_cap);
int es_knn_radius(const float* x, int64_t ld, int rows, int cols, const int32_t* idx /* [rows] or NULL */,
                  const int32_t* seg /* [n_seg, 2] */, int n_seg, int cap, int k, double* radius2 /* [n_seg, cap] */,
                  void* work, size_t work_bytes, es_stream_t stream);
int es_prdc_count(const float* real, int64_t r_ld, int r_rows, const int32_t* r_idx, const int32_t* r_seg, int r_cap,
                  const float* fake, int64_t f_ld, int f_rows, const int32_t* f_idx, const int32_t* f_seg, int f_cap,
                  int cols, int n_seg, int k, const double* r_radius2, const double* f_radius2,
                  int32_t* f_count /* or NULL */, int32_t* r_hit /* or NULL */, double* r_min2 /* or NULL */,
                  int64_t* totals /* [n_seg, 8] */, void* work, size_t work_bytes, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Distances between the joint distributions of the shower observables: the Frechet distance between fitted
 * Gaussians and the polynomial-kernel MMD of Kansal et al. 2023 ("Evaluating generative models in high energy
 * physics") -- csrc/distance.hip.
 * ---------------------------------------------------------------------------------------- */
/* Every pointer is a DEVICE pointer; no host sync, everything runs on `stream`.  Outside the limits, with a NULL
 * required pointer or too small a workspace: ES_ERR_ARG before any launch, and nothing is written.  Segments follow
 * es_wasserstein_1d (see es_knn_radius above): rows idx[seg[2s] .. seg[2s+1]), idx NULL: the rows themselves, the
 * bounds clamped to [0, rows], every row index to [0, rows); segments may overlap.  No float atomics: partial sums
 * per chunk / tile go to the workspace and are added in a fixed order, so a rerun is bit-equal.  All arithmetic is
 * fp64 (products and sums may be fused).
 *
 * es_segment_moments.  x [rows][ld], fp32 or fp64 (x_f64 != 0) with unit column stride, 1 <= cols <= ES_MOMENTS_MAX_COLS,
 * cols <= ld, 1 <= rows <= ES_DIST_MAX_ROWS, 1 <= n_seg <= ES_DIST_MAX_SEG.  For segment s with the n members x_p:
 *   count[s] (int32 [n_seg]) = n
 *   mean[s][c] (fp64 [n_seg][cols]) = sum_p x_p[c] / n                                   (NaN when n == 0)
 *   cov[s][i][j] (fp64 [n_seg][cols][cols]) = sum_p (x_p[i] - mean[i]) (x_p[j] - mean[j]) / (n - 1)   (NaN when n < 2)
 * i.e. np.cov(rowvar=False): two passes, centred on the rounded mean.  The upper triangle i <= j is computed and
 * mirrored, so cov[i][j] and cov[j][i] are the same bits.  Order of a sum: the members are cut into ES_MOMENTS_CHUNKS
 * runs of max(64, ceil(n / ES_MOMENTS_CHUNKS)) consecutive members; within a run eight (mean) or one (cov) strided
 * sequential chains, added in order; the runs in order.
 * work: es_segment_moments_workspace(n_seg, cols) bytes (0: outside the limits): the runs' partial sums.
 *
 * es_frechet.  n problems (1 <= n <= ES_DIST_MAX_SEG, 1 <= cols <= ES_MOMENTS_MAX_COLS), problem i the moments
 * mean_a[i][cols], cov_a[i][cols][cols], mean_b[i], cov_b[i] as es_segment_moments writes them (cov symmetric; the
 * upper triangle is read).  out[i] (fp64 [n][4]) = { d2, |dmu|^2, tr A + tr B, tr (A B)^1/2 } with
 *   d2 = |dmu|^2 + tr A + tr B - 2 tr (A B)^1/2,
 *   tr (A B)^1/2 = sum_k sqrt(max(m_k, 0)), m_k the eigenvalues of the symmetric A^1/2 B A^1/2,
 *   A^1/2 = V diag(sqrt(max(l_k, 0))) V^T from the eigendecomposition A = V diag(l) V^T.
 * Both decompositions are cyclic Jacobi in fp64 (rotation skipped when |a_pq| <= 2^-56 sqrt(|a_pp a_qq|), at most 30
 * sweeps), one workgroup per problem with the matrices in LDS.  A problem with a NaN anywhere in its moments gives
 * NaN in all four outputs.
 *
 * es_mmd_poly.  real / fake fp32 [rows][ld] with their own ld / rows / idx / seg / cap (the host upper bound of a
 * segment's length, which sizes the grid and the workspace; longer segments are cut to it) and the same n_seg;
 * 1 <= cols <= ES_MMD_MAX_COLS, 1 <= degree <= ES_MMD_MAX_DEGREE, 1 <= rows, cap <= ES_DIST_MAX_ROWS,
 * 1 <= n_seg <= ES_DIST_MAX_SEG.  With k(u, v) = (gamma <u, v> + coef0)^degree (<u, v> the fp64 sum over the columns
 * in order of the widened fp32 entries, the power by degree - 1 multiplications), for segment s with the real
 * members x_i, i < m, and the generated members y_j, j < n:
 *   sums[s] (fp64 [n_seg][4]) = { S_xx = sum_{i != j} k(x_i, x_j), S_yy = sum_{i != j} k(y_i, y_j),
 *                                 S_xy = sum_{i, j} k(x_i, y_j), 0 }
 *   counts[s] (int32 [n_seg][2]) = { m, n }
 * The diagonal of S_xx / S_yy is excluded by member position, not subtracted.  No kernel value is stored: one grid
 * walks 128 x 128 tiles of all three matrices of all segments, a thread adds its 8 x 8 pairs tile after tile, the
 * threads of a workgroup are added by a butterfly and the workgroups' partials in tile order by a second launch.
 * The unbiased MMD^2 = S_xx / (m (m - 1)) + S_yy / (n (n - 1)) - 2 S_xy / (m n) is left to the host.
 * work: es_mmd_poly_workspace(n_seg, r_cap, f_cap) bytes (0: outside the limits): the workgroups' partials. */
#define ES_DIST_MAX_ROWS (1 << 20)
#define ES_DIST_MAX_SEG 1024
#define ES_MOMENTS_MAX_COLS 32
#define ES_MOMENTS_CHUNKS 16
#define ES_MMD_MAX_COLS 64
#define ES_MMD_MAX_DEGREE 8
size_t es_segment_moments_workspace(int n_seg, int cols);
size_t es_mmd_poly_workspace(int n_seg, int r_cap, int f_cap);
int es_segment_moments(const void* x, int x_f64, int64_t ld, int rows, int cols,
                       const int32_t* idx /* [rows] or NULL */, const int32_t* seg /* [n_seg, 2] */, int n_seg,
                       int32_t* count /* [n_seg] */, double* mean /* [n_seg, cols] */,
                       double* cov /* [n_seg, cols, cols] */, void* work, size_t work_bytes, es_stream_t stream);
int es_frechet(const double* mean_a, const double* cov_a, const double* mean_b, const double* cov_b, int n, int cols,
               double* out /* [n, 4] */, es_stream_t stream);
int es_mmd_poly(const float* real, int64_t r_ld, int r_rows, const int32_t* r_idx, const int32_t* r_seg, int r_cap,
                const float* fake, int64_t f_ld, int f_rows, const int32_t* f_idx, const int32_t* f_seg, int f_cap,
                int cols, int n_seg, int degree, double gamma, double coef0, double* sums /* [n_seg, 4] */,
                int32_t* counts /* [n_seg, 2] */, void* work, size_t work_bytes, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sliced Wasserstein distance of whole images -- csrc/sliced.hip.  The 1-D distances of the projected columns
 * are es_wasserstein_1d's (channels = n_proj, ld = out_ld), the moments over the directions es_segment_moments'.
 * ---------------------------------------------------------------------------------------- */
/* es_sliced_project.  x [n,1,h,w] (any strides, fp32 or bf16, widened exactly); pixel (i, j) is element
 * d = i * w + j of D = h * w.  theta [n_proj][theta_ld] fp64, theta_ld >= D.  out[b * out_ld + p] (fp64,
 * out_ld >= n_proj) = sum_d x[b][d] * theta[p][d]; the columns n_proj .. out_ld and the rows from n on are not
 * written.  The sum runs on v_mfma_f64_16x16x4_f64: every output element is ONE accumulator chain from +0.0 over
 * the k-steps d0 = 0, 4, 8, ... in ascending order (four products a step, added by the instruction), D padded to a
 * multiple of 4 with +0.0 operands; no split over D, no atomics.  A result is bit-equal across reruns and does
 * not depend on n, on n_proj, on the row's position in the batch, on the direction's position in theta or on the
 * strides.  With n_proj <= 256 every image is read from memory once.
 * 1 <= D <= ES_SLICED_MAX_D, 1 <= n_proj <= ES_SLICED_MAX_PROJ, n <= 2^20, c == 1; outside that, with a NULL
 * pointer, theta_ld < D or out_ld < n_proj: ES_ERR_ARG before any launch.  n == 0: ES_OK without a launch.
 *
 * es_sliced_directions.  theta [n_proj][theta_ld] fp64 (theta_ld >= d; columns from d on are not written): row p is
 * the draws p * D2 .. p * D2 + d - 1 of es_randn(., n_proj * D2, seed, stream_id), D2 = d rounded up to even,
 * widened to fp64 and divided by the square root of their fp64 sum of squares.  That sum: thread t of 256 adds
 * the squares of draws t, t + 256, ... in that order, the 64 lanes of a wave by a butterfly, the four waves in
 * order; bit-equal across reruns.  1 <= d <= ES_SLICED_MAX_D, 1 <= n_proj <= ES_SLICED_MAX_PROJ. */
#define ES_SLICED_MAX_D 4096
#define ES_SLICED_MAX_PROJ 1024
int es_sliced_project(const es_view_t* x, es_dtype_t dt, const void* xp, const double* theta, int64_t theta_ld,
                      int n_proj, double* out, int64_t out_ld, es_stream_t stream);
int es_sliced_directions(double* theta, int64_t theta_ld, int n_proj, int d, uint64_t seed, uint32_t stream_id,
                         es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Classifier two-sample test: exact rank statistics (csrc/rank.hip) and ridge-penalised logistic regression per
 * segment (csrc/classifier.hip).
 * ---------------------------------------------------------------------------------------- */
/* es_rank_stats.  The arguments, the segment rule, the clamping, the caps, the limits and the workspace rule are
 * es_wasserstein_1d's: u / v fp64 [rows][ld] (ld >= channels), DEVICE idx / seg, host u_cap / v_cap, one launch
 * with each problem sorted in LDS while u_cap + v_cap <= ES_WS_LDS_MAX, global-memory passes over `work`
 * (es_rank_stats_workspace bytes) up to 2^20, ES_ERR_ARG above that or with too small a workspace and nothing is
 * launched.  Values must be finite.  For column c of segment s with the nu values u_i and the nv values v_j:
 *   out[(s * channels + c) * 4 ..] (int64) = { nu, nv, U2, KS }
 *   U2 = sum over the pairs (i, j) of 2 [u_i > v_j] + [u_i == v_j]: U2 / (2 nu nv) is the ROC AUC of u against v
 *        (the Mann-Whitney U statistic of u is U2 / 2), ties counted half;
 *   KS = max over the distinct values a of |cu(a) nv - cv(a) nu|, cu(a) / cv(a) the counts of values <= a:
 *        KS / (nu nv) is the two-sample Kolmogorov-Smirnov statistic.
 * A segment empty on either side gives { nu, nv, 0, 0 }.  -0.0 and +0.0 are the same value.  Integer arithmetic
 * throughout (nu nv <= 2^38); counts are looked at only where a run of equal values starts or ends, so the order
 * the sort leaves inside a run cannot matter; no atomics; a rerun is bit-equal. */
size_t es_rank_stats_workspace(int n_seg, int channels, int u_cap, int v_cap);
int es_rank_stats(const double* u, int64_t u_ld, int u_rows, const int32_t* u_idx, const int32_t* u_seg,
                  const double* v, int64_t v_ld, int v_rows, const int32_t* v_idx, const int32_t* v_seg,
                  int n_seg, int channels, int u_cap, int v_cap, int64_t* out /* [n_seg * channels, 4] */,
                  void* work, size_t work_bytes, es_stream_t stream);
/* es_logit_fit / es_logit_scores.  real / fake [rows][ld] with their own ld / rows / idx / seg / cap as for
 * es_mmd_poly (same segment rule, same n_seg, cap the host upper bound of a segment's length), fp32 or fp64 for
 * both (x_f64 != 0), 1 <= cols <= ES_LOGIT_MAX_COLS, cols <= ld, 1 <= rows, cap <= ES_DIST_MAX_ROWS,
 * 1 <= n_seg <= ES_DIST_MAX_SEG.  Outside the limits, with a NULL required pointer or too small a workspace:
 * ES_ERR_ARG before any launch.  Values must be finite.
 *
 * Per segment s the m real members carry y = 1 and the k generated members y = 0; with n = m + k, z~ = (1, z) and
 * theta = (b, w) the objective is
 *   F(theta) = (1/n) sum_i [softplus(t_i) - y_i t_i] + (l2 / (2 n)) |w|^2,   t_i = b + <w, z_i>
 * (the intercept unpenalised, l2 = scikit-learn's 1 / C, softplus without overflow).
 *
 * es_logit_fit minimises F from theta = 0 by Newton steps in fp64: g = (1/n) Z~^T (p - y) + (l2/n) (0, w),
 * H = (1/n) Z~^T diag(p (1 - p)) Z~ + (l2/n) diag(0, 1..1), the step d = -H^-1 g by a Cholesky factorisation in the
 * kernel.  A step is safeguarded on F: theta + d is taken when F(theta + d) <= F(theta) (1 + (n + 64) 2^-52), i.e.
 * F did not increase beyond its own rounding; otherwise the point of least F < F(theta) among theta + 2^-j d,
 * j = 1 .. 7 (all evaluated in the same pass), and g, H are re-evaluated there.  The fit stops with status 1 once
 * |g|_inf <= gtol, with status 0 after max_iter (1 .. ES_LOGIT_MAX_ITER) moves, when no trial point lowers F or
 * when the factorisation meets a pivot <= 0 (possible only with l2 = 0); theta is always the last accepted point
 * and |g|_inf, F belong to it.  A segment empty on either side is degenerate: status -1, theta NaN.
 *   theta (fp64 [n_seg][cols + 1]) intercept first
 *   stat  (fp64 [n_seg][4]) = { F, |g|_inf, iterations (moves taken), status }
 * The host issues 1 + 2 (max_iter + 1) launches and never synchronises; a per-segment device flag turns the
 * launches after the stop into early-outs.  Members are numbered real first; blocks of ES_LOGIT_BLOCK_ROWS
 * (es_logit_block_rows()) consecutive members go to one workgroup each, whose partial g, H, F go to the workspace;
 * one workgroup per segment adds them in block order, solves and updates in the next launch.  No float atomics,
 * every sum in a fixed order: a rerun is bit-equal.
 * work: es_logit_fit_workspace(n_seg, cols, r_cap, f_cap) bytes (0: outside the limits).
 *
 * es_logit_scores.  The same tables and segments plus theta as es_logit_fit writes it.  The score of a member is
 * t = b + sum_c w_c z_c, one fused multiply-add per column in ascending order from t = b.  Layout: the score of
 * real member i of segment s is r_scores[s * r_cap + i], of generated member j f_scores[s * f_cap + j] (fp64
 * [n_seg][cap]; entries past a segment's length are not written), and r_oseg / f_oseg (int32 [n_seg][2]) receive
 * the bounds (s * cap, s * cap + length), so that
 *   es_rank_stats(r_scores, 1, n_seg * r_cap, NULL, r_oseg, f_scores, 1, n_seg * f_cap, NULL, f_oseg, n_seg, 1,
 *                 r_cap, f_cap, ..)
 * reads every segment's scores back without a host-side length (n_seg * cap <= 2^31 - 1).
 *   sums (fp64 [n_seg][4]) = { real members with t > 0, generated members with t <= 0,
 *                              sum of softplus(-t) over the real members, sum of softplus(t) over the generated }
 * Order of a sum: blocks of 256 consecutive members, inside a block a butterfly over the 64 lanes and the four
 * waves in order, the blocks in order.  A NaN theta gives NaN scores and sums { 0, 0, NaN, NaN }.
 * work: es_logit_scores_workspace(n_seg, r_cap, f_cap) bytes (0: outside the limits). */
#define ES_LOGIT_MAX_COLS 80
#define ES_LOGIT_MAX_ITER 100
#define ES_LOGIT_BLOCK_ROWS 256
int es_logit_block_rows(void);
size_t es_logit_fit_workspace(int n_seg, int cols, int r_cap, int f_cap);
size_t es_logit_scores_workspace(int n_seg, int r_cap, int f_cap);
int es_logit_fit(const void* real, int64_t r_ld, int r_rows, const int32_t* r_idx, const int32_t* r_seg, int r_cap,
                 const void* fake, int64_t f_ld, int f_rows, const int32_t* f_idx, const int32_t* f_seg, int f_cap,
                 int x_f64, int cols, int n_seg, double l2, double gtol, int max_iter,
                 double* theta /* [n_seg, cols + 1] */, double* stat /* [n_seg, 4] */, void* work, size_t work_bytes,
                 es_stream_t stream);
int es_logit_scores(const void* real, int64_t r_ld, int r_rows, const int32_t* r_idx, const int32_t* r_seg, int r_cap,
                    const void* fake, int64_t f_ld, int f_rows, const int32_t* f_idx, const int32_t* f_seg, int f_cap,
                    int x_f64, int cols, int n_seg, const double* theta /* [n_seg, cols + 1] */,
                    double* r_scores /* [n_seg, r_cap] */, double* f_scores /* [n_seg, f_cap] */,
                    int32_t* r_oseg /* [n_seg, 2] */, int32_t* f_oseg /* [n_seg, 2] */, double* sums /* [n_seg, 4] */,
                    void* work, size_t work_bytes, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Conditional fidelity: order statistics per segment (csrc/quantile.hip) and rows to condition bins
 * (csrc/bins.hip); the two rules are csrc/quantile_rule.h.
 * ---------------------------------------------------------------------------------------- */
/* es_segment_quantiles.  The arguments, the segment rule, the clamping, the caps, the limits and the workspace rule
 * are es_wasserstein_1d's: u / v fp64 [rows][ld] (ld >= channels), DEVICE idx / seg, host u_cap / v_cap, one launch
 * with each problem sorted in LDS while u_cap + v_cap <= ES_WS_LDS_MAX, global-memory passes over `work`
 * (es_segment_quantiles_workspace bytes) up to 2^20, ES_ERR_ARG above that or with too small a workspace and nothing
 * is launched.  Values must be finite.
 * probs is the ONE HOST pointer of the call: n_q probabilities (1 <= n_q <= ES_QUANTILE_MAX_Q), copied into the
 * launch arguments before the call returns; a probability outside [0, 1] or NaN gives ES_ERR_ARG before any launch.
 * For column c of segment s, side 0 the u values and side 1 the v values, a side having n values
 * x_(0) <= .. <= x_(n-1):
 *   count[s * 2 + side] (int32) = n
 *   out[((s * channels + c) * 2 + side) * n_q + k] (fp64) = the quantile at probs[k] by numpy's default rule:
 *     h = probs[k] * (n - 1) (one fp64 multiplication), lo = floor(h), g = h - lo, hi = min(lo + 1, n - 1),
 *     a = x_(lo), b = x_(hi), d = b - a, the result is g >= 0.5 ? b - d * (1 - g) : a + d * g,
 *   every operation rounded on its own (no fused multiply-add): bit-equal to np.quantile(x, probs[k]).
 * A side with n == 0 has NaN in all its n_q entries; the other side is still computed.  v == NULL with v_rows == 0
 * and v_cap == 0 is the one-sample form (v_ld, v_idx, v_seg are not read; side 1 is empty everywhere).
 * Both sides come out of ONE tagged sort of the problem (the sort of es_wasserstein_1d); the j-th order statistic
 * of a side is the key at the position whose own tag is the side's and whose exclusive prefix count of that tag is
 * j.  -0.0 and +0.0 are the same value and read as +0.0, so equal keys are equal values and the order the sort
 * leaves inside a run cannot matter; no atomics; a rerun is bit-equal. */
#define ES_QUANTILE_MAX_Q 16
size_t es_segment_quantiles_workspace(int n_seg, int channels, int u_cap, int v_cap);
int es_segment_quantiles(const double* u, int64_t u_ld, int u_rows, const int32_t* u_idx, const int32_t* u_seg,
                         const double* v, int64_t v_ld, int v_rows, const int32_t* v_idx, const int32_t* v_seg,
                         int n_seg, int channels, int u_cap, int v_cap, const double* probs /* HOST [n_q] */, int n_q,
                         double* out /* [n_seg * channels, 2, n_q] */, int32_t* count /* [n_seg, 2] */, void* work,
                         size_t work_bytes, es_stream_t stream);
/* es_bin_dispatch.  x [rows] with element stride ld, fp32 or fp64 (x_f64 != 0; fp32 is widened exactly), finite;
 * edges DEVICE fp64 [n_bins - 1], ascending, equal neighbours allowed (NULL when n_bins == 1); expert DEVICE int32
 * [rows] or NULL (then n_experts must be 1).  1 <= n_bins <= ES_BINS_MAX, n_classes = n_bins * (expert ? n_experts
 * : 1) <= 1024, 1 <= rows <= 2^20; outside that, with a NULL required pointer or too small a workspace: ES_ERR_ARG
 * before any launch.
 *   bin(x) = the number of edges strictly below x = np.searchsorted(edges, x, side="left"): the intervals are
 *            pandas' (a, b], a value equal to an edge belongs to the lower bin;
 *   class  = bin, or clamp(expert, 0, n_experts - 1) * n_bins + bin with an expert vector.
 *   bin  (int32 [rows], may be NULL) = bin(x) of every row
 *   perm (int32 [rows]), offs (int32 [n_classes + 1]) in es_router_dispatch's layout: the rows grouped by class,
 *        each group in ascending row order, offs[c] the start of class c, offs[n_classes] = rows.
 * The answer is np.argsort(class, kind="stable") and the cumulative counts, and it does not depend on the order
 * in which anything lands: there is no atomic.  Three launches over chunks of 1024 rows -- per chunk a sort in LDS
 * of (class, local row) that gives every row its rank inside its class and the chunk's class counts, one scan of
 * the counts in (class, chunk) order, one scatter -- and no host synchronisation: every pointer is a device pointer.
 * work: es_bin_dispatch_workspace(rows, n_classes) bytes (0: outside the limits). */
#define ES_BINS_MAX 64
size_t es_bin_dispatch_workspace(int rows, int n_classes);
int es_bin_dispatch(const void* x, int x_f64, int64_t ld, int rows, const double* edges, int n_bins,
                    const int32_t* expert, int n_experts, int32_t* bin /* [rows] or NULL */, int32_t* perm /* [rows] */,
                    int32_t* offs /* [n_classes + 1] */, void* work, size_t work_bytes, es_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Simulation (inference) path: conditions in, calorimeter images out -- the reference's prediction
 * helpers (train/utils.py:179-266: generate, expm1, per-expert scatter into batch order) over the
 * eval-mode generators (neutron/generator.py:13-36 BatchNorm -> LeakyReLU chains).
 * ---------------------------------------------------------------------------------------- */
/* Eval-mode BatchNorm as a per-channel affine: scale[c] = gamma[c] * rsqrt(running_var[c] + eps),
 * shift[c] = beta[c] - running_mean[c] * scale[c] (gamma / beta NULL: 1 / 0).  Replaces the
 * aten::rsqrt / mul / sub of an eval-mode native_batch_norm (neutron/generator.py:13,19,26,31,35). */
int es_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
               int C, float eps, float* scale, float* shift, es_stream_t stream);
/* es_bn_fold for n <= ES_BN_FOLD_MAX BatchNorms (all those of one generator) in ONE launch; the arrays
 * are host arrays of device pointers / sizes, as es_sn_power_iter_batch takes them.  Same values as
 * n single calls, bit for bit. */
#define ES_BN_FOLD_MAX 8
int es_bn_fold_batch(int n, const float* const* gamma, const float* const* beta, const float* const* running_mean,
                     const float* const* running_var, const int* C, const float* eps, float* const* scale,
                     float* const* shift, es_stream_t stream);
/* Last pass of a routed simulation for one expert (train/utils.py:208-266: relu is the generator's
 * last layer, np.expm1 of the prediction, `predictions[indices] = ...` scatter; train/utils.py:62-78
 * channel sums).  x: the expert's pre-activation last-conv output [cap,1,H,W] fp32 (any strides); for
 * i < min(live[0], cap) (live NULL: cap): v = relu(x[i]); image perm[start[0] + i] of the
 * batch-ordered out [N,H,W] fp32 (dense) = v, or expm1(v) when photons != 0; sums[(perm[start[0] + i]) * 5
 * .. + 4] (fp64) = the five masked sums of expm1(v), same masks and summation order as es_channel_sums
 * with log_domain = 1.  out or sums may be NULL; perm NULL: identity (image i). */
int es_sim_finish(const es_view_t* x, const void* xp, const int32_t* live, const int32_t* perm,
                  const int32_t* start, int photons, float* out, double* sums, es_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EXPERTSIM_HIP_H */
