// Host side of the convolution entries (include/expertsim_hip.h): descriptor checks, the GEMM view of the
// three convolutions, the plan of a call (conv_plan.h) and every es_conv2d_* entry.  Host code only: no
// kernel, and no HIP call except the one read of the launch status that ends each C-ABI entry.  The
// kernels are in conv_igemm_bf16.hip / conv_igemm_f32.hip (conv_igemm_kernel.h), conv_thin.hip and the
// ring files (ring_plan.h), each behind a launch function.
#include <algorithm>
#include <cstdlib>

#include "conv_plan.h"

// direct kernels for one-input-channel / one-output-channel convolutions (conv_thin.hip): 1 launched
// (call.path gets PATH_THIN), 0 not a thin conv
int es_thin_conv_fwd(const es_conv_desc_t* d, es_dtype_t dt, const void* x, const int64_t xs[4], const void* wk,
                     const float* bias, void* y, es_dtype_t ydt, const int64_t ys[4], ConvCall& call, hipStream_t st);
int es_thin_conv_dgrad(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4],
                       const void* wd, void* dx, es_dtype_t dxdt, const int64_t dxs[4], float beta,
                       ConvCall& call, hipStream_t st);
int es_thin_conv_wgrad(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4], const void* x,
                       const int64_t xs[4], float* dw, ConvCall& call, hipStream_t st);

bool g_es_det = false;

extern "C" int es_set_deterministic(int on) {
  const int old = g_es_det;
  g_es_det = on != 0;
  return old;
}

// ---------------------------------------------------------------------------------------- the plan
int conv_plan(const ConvArgs& a, int mode, es_dtype_t dt, bool avec, bool bvec, const ConvCall& call,
              const RingSwitches& sw, bool det_mode, ConvPlan& p) {
  const es_conv_desc_t& d = a.d;
  p = ConvPlan{};
  p.k_per_split = a.Kd;
  p.det = a.det;
  p.det_ws = a.det_ws;
  p.det_splits = call.det_splits;
  // sub-pixel FWD / DGRAD: only the ring kernels read mode 2 / 3 packed weights
  if (d.subpixel && mode != MODE_WGRAD) {
    p.route = dt == ES_F32 ? ROUTE_RING_F32 : ROUTE_RING_BF16;
    return ES_OK;
  }
  ES_CHECK_ARG(dt == ES_F32 || dt == ES_BF16, "conv: unsupported dtype %d", (int)dt);
  if (d.stride > 2) avec = bvec = false;   // vector DGRAD gather handles strides 1 and 2
  const int eb = dt == ES_BF16 ? 2 : 4;
  const int BK = 128 / eb;                 // K-step: 128 operand bytes per row
  int ring = ROUTE_NONE;                   // the ring asked before the 4-wave route
  auto routed = [&](const ConvKey& key, int bm, int bn, int splits) {
    p.route = ring ? ring : key.family;
    p.fallback = ring ? key.family : ROUTE_NONE;
    p.key = key;
    p.grid[0] = (a.M + bm - 1) / bm; p.grid[1] = (a.Ng + bn - 1) / bn; p.grid[2] = splits;
    return ES_OK;
  };
  if (eb == 2 && mode != MODE_WGRAD) {
    // LDS-DMA path: one tap x 64 channels per K-step, big enough to fill the chip without split-K
    const int nch = mode == MODE_FWD ? d.C : d.K;
    const int tiles = ((a.M + 127) / 128) * ((a.Ng + 127) / 128);
    const bool splitk_better = a.dense_f32_out && tiles < 256 && a.Kd / 64 >= 16;   // see below
    // (an affine-epilogue FWD, es_conv2d_fwd_affine, also takes the ring below 128 rows: its tiles pad
    // the rows, and only the ring kernels carry that epilogue)
    const bool small_aff = mode == MODE_FWD && a.M < 128 && call.aff != nullptr;
    if (avec && bvec && nch % 64 == 0 && d.stride <= 2 && d.hmap == nullptr && (a.M >= 128 || small_aff) &&
        !splitk_better && sw.glds) {
      if (a.Kd % 64 == 0) ring = ROUTE_RING_BF16;
      if (!small_aff) return routed(glds_key(mode, 128, a.Ng > 64 ? 128 : 64), 128, a.Ng > 64 ? 128 : 64, 1);
    }
  }
  if (eb == 4 && mode != MODE_WGRAD) {
    // fp32 parity mode: the 8-wave LDS-DMA ring kernels on v_mfma_f32_16x16x4_f32 (conv_ring_f32.hip)
    // for real convolutions whose K-steps are one tap x 32 channels
    const int nch = mode == MODE_FWD ? d.C : d.K;
    // (the gathered grid's pixels per image: >= 8 keeps the row tiles' padding small; the aux
    // regressor's conv4 has a 1 x 15 output and a 3 x 17 input; linears take the pixel view)
    const int gpix = mode == MODE_FWD ? d.P * d.Q : d.Hu * d.Wu;
    const bool small_aff = mode == MODE_FWD && a.M < 128 && call.aff != nullptr && sw.f32_split > 0;
    if (avec && bvec && nch % 32 == 0 && a.Kd % 32 == 0 && d.stride <= 2 && d.hmap == nullptr && gpix >= 8 &&
        (a.M >= 128 || small_aff) && sw.glds)
      ring = ROUTE_RING_F32;
  }
  // tile choice: 128x128 for big GEMMs, 64x64 when either side is small, or when the output is
  // split over K anyway (few tiles, long K: more, smaller workgroups)
  const int tiles128 = ((a.M + 127) / 128) * ((a.Ng + 127) / 128);
  // (deterministic mode: only with a partial workspace, es_conv2d_fwd_det / es_conv2d_dgrad_det)
  const bool splitk_case = mode != MODE_WGRAD && a.dense_f32_out && tiles128 < 256 && (a.Kd + BK - 1) / BK >= 16 &&
                           !(eb == 4 && det_mode && call.det_ws == nullptr);
  // 128 x 128 only with enough tiles to fill the chip: a small GEMM (the discriminator / router /
  // aux linears at batch 512) is latency-bound per K-step, so more, smaller workgroups finish sooner
  const bool big = a.M >= 128 && a.Ng >= 96 && !splitk_case && tiles128 >= 128;
  // narrow fp32 GEMMs (the discriminator's 32->16 conv: FWD / DGRAD with N <= 32, WGRAD with
  // M = 16 output channels): a 64 x 64 tile wastes half or 3/4 of every MFMA; 128 x 32 and
  // 32 x 128 tiles keep the 2 x 2 wave grid with one 16-row (column) fragment per wave
  const bool narrow_n = eb == 4 && mode != MODE_WGRAD && a.Ng <= 32 && !splitk_case;
  const bool narrow_m = eb == 4 && mode == MODE_WGRAD && a.M <= 32 && !big;
  const int BM = big ? 128 : (narrow_n ? 128 : (narrow_m ? 32 : 64));
  const int BN = big ? 128 : (narrow_n ? 32 : (narrow_m ? 128 : 64));
  if (eb == 2 && mode == MODE_WGRAD && !a.det && avec && bvec && sw.glds) {
    ring = ROUTE_RING_BF16;
    if (d.K % 128 == 0 && d.C % 128 == 0 && d.stride <= 2 && d.hmap == nullptr) {
      const int t128 = (a.M / 128) * (a.Ng / 128);
      const int ks = (a.Kd + 63) / 64;
      int want = (2048 + t128 - 1) / t128;
      want = std::max(1, std::min(want, ks / 4 > 0 ? ks / 4 : 1));
      p.k_per_split = ((ks + want - 1) / want) * 64;
      return routed(wgrad_glds_key(), 128, 128, (a.Kd + p.k_per_split - 1) / p.k_per_split);   // (whole tiles)
    }
  }
  int splits = 1;
  const int tiles = ((a.M + BM - 1) / BM) * ((a.Ng + BN - 1) / BN);
  const int ksteps = (a.Kd + BK - 1) / BK;
  if (mode == MODE_WGRAD) {
    int want = (2048 + tiles - 1) / tiles;            // ~2048 workgroups
    want = std::max(1, std::min(want, ksteps / 4 > 0 ? ksteps / 4 : 1));  // >= 4 K-steps per split
    if (a.det) {   // deterministic: one partial slot per split, within the caller's workspace
      const int64_t slot = (int64_t)a.M * a.Ng;
      want = (int)std::max<int64_t>(1, std::min<int64_t>(want, call.det_floats / slot));
    }
    p.k_per_split = ((ksteps + want - 1) / want) * BK;
    splits = (a.Kd + p.k_per_split - 1) / p.k_per_split;
    if (a.det) p.det_splits = splits;
  } else if (splitk_case) {
    // few output tiles and a long K (the linears at batch 512): split K over ~1024 workgroups,
    // at least 4 K-steps each
    int want = std::min((1024 + tiles - 1) / tiles, ksteps / 4);
    const bool det = call.det_ws != nullptr;
    if (det) want = (int)std::min<int64_t>(want, call.det_floats / ((int64_t)a.M * a.Ng));
    if (want > 1) {
      p.k_per_split = ((ksteps + want - 1) / want) * BK;
      splits = (a.Kd + p.k_per_split - 1) / p.k_per_split;
      p.splitk = splits > 1;
      if (det && p.splitk) {   // ordered: split z stores into its own slot, es_splitk_reduce sums
        p.det = 1;
        p.det_ws = call.det_ws;
        p.det_splits = splits;
      } else {
        p.zero_out = p.splitk;   // atomics into a zeroed output
      }
    }
  }
  return routed(igemm_key(eb, mode, BM, BN, avec, bvec), BM, BN, splits);
}

void conv_apply(const ConvPlan& p, ConvArgs& a, ConvCall& call) {
  a.k_per_split = p.k_per_split;
  a.splitk = p.splitk;
  a.det = p.det;
  a.det_ws = p.det_ws;
  call.det_splits = p.det_splits;
}

// Plans, asks the ring the plan names, else launches the plan.  Every attempt runs on copies that the
// call takes over only when it was launched.
int conv_dispatch(const ConvArgs& a, int mode, es_dtype_t dt, bool avec, bool bvec, ConvCall& call, hipStream_t st) {
  ConvPlan p;
  if (int e = conv_plan(a, mode, dt, avec, bvec, call, es_conv_switches(), g_es_det, p)) return e;
  if (p.route == ROUTE_RING_BF16 || p.route == ROUTE_RING_F32) {
    ConvArgs r = a;
    ConvCall rcall = call;
    r.k_per_split = a.Kd;
    r.splitk = 0;
    const int rc = p.route == ROUTE_RING_F32 ? es_conv_ring_launch_f32(r, mode, rcall, st)
                                             : es_conv_ring_launch(r, mode, rcall, st);
    if (rc > 0) {
      call = rcall;
      return ES_OK;
    }
    ES_CHECK_ARG(p.fallback != ROUTE_NONE, "conv: sub-pixel operands not dense NHWC (ring kernels required)");
    if (rc < 0) return ES_ERR_ARG;   // (the ring's message stands)
  }
  ConvArgs l = a;
  ConvCall lcall = call;
  conv_apply(p, l, lcall);
  const int rc = p.key.eb == 2 ? conv_igemm_bf16_launch(p, l, st) : conv_igemm_f32_launch(p, l, st);
  if (rc < 0) return ES_ERR_HIP;
  ES_CHECK_ARG(rc > 0, "conv: no kernel for family %d eb %d mode %d tile %d x %d avec %d bvec %d", p.key.family, p.key.eb,
               p.key.mode, p.key.bm, p.key.bn, p.key.avec, p.key.bvec);
  call = lcall;
  return ES_OK;
}

namespace {

void fill_divs(ConvArgs& a) {
  a.fC = mkdiv(a.d.C); a.fS = mkdiv(a.d.S); a.fK = mkdiv(a.d.K); a.fQ = mkdiv(a.d.Q);
  a.fP = mkdiv(a.d.P); a.fWu = mkdiv(a.d.Wu); a.fHu = mkdiv(a.d.Hu);
  a.fUh = mkdiv(a.d.up_h > 0 ? a.d.up_h : 1); a.fUw = mkdiv(a.d.up_w > 0 ? a.d.up_w : 1);
  a.fRSK = mkdiv(a.d.R * a.d.S * a.d.K); a.fW = mkdiv(a.d.W); a.fH = mkdiv(a.d.H);
}

// 16-byte vector access along an operand dimension of n values with element stride `stride`
bool vec16(es_dtype_t dt, int64_t stride, int n) { return stride == 1 && n % (dt == ES_BF16 ? 8 : 4) == 0; }

// strides (n, c, h, w) describe a dense [n][h][w][c] tensor (rows of c contiguous values)
bool dense_rows(const int64_t s[4], int c, int h, int w) {
  return s[1] == 1 && (w == 1 || s[3] == c) && (h == 1 || s[2] == (int64_t)w * c) && s[0] == (int64_t)h * w * c;
}

int check_desc(const es_conv_desc_t* d) {
  ES_CHECK_ARG(d && d->N > 0 && d->C > 0 && d->K > 0 && d->R > 0 && d->S > 0 && d->stride > 0,
               "conv: bad descriptor");
  ES_CHECK_ARG(d->P == (d->Hu + 2 * d->pad - d->R) / d->stride + 1 &&
                   d->Q == (d->Wu + 2 * d->pad - d->S) / d->stride + 1,
               "conv: output size %dx%d inconsistent with input %dx%d k%dx%d s%d p%d", d->P, d->Q,
               d->Hu, d->Wu, d->R, d->S, d->stride, d->pad);
  ES_CHECK_ARG((d->hmap == nullptr) == (d->wmap == nullptr), "conv: hmap/wmap must both be set");
  ES_CHECK_ARG((d->up_h > 0) == (d->up_w > 0), "conv: up_h/up_w must both be set");
  ES_CHECK_ARG(d->up_h <= 0 || (d->Hu == d->H * d->up_h && d->Wu == d->W * d->up_w),
               "conv: Hu/Wu must equal H*up_h / W*up_w");
  ES_CHECK_ARG(d->hmap || d->up_h > 0 || (d->Hu == d->H && d->Wu == d->W), "conv: Hu/Wu != H/W without maps");
  const int64_t M1 = (int64_t)d->N * d->P * d->Q, M2 = (int64_t)d->N * d->Hu * d->Wu;
  ES_CHECK_ARG(M1 < (1ll << 31) && M2 < (1ll << 31), "conv: problem too large for int32 rows");
  return ES_OK;
}

// ---------------------------------------------------------------- executed-work tally (es_conv_exec_flops)
// per host thread (the probe reads the thread that issued the convs)
thread_local double g_exec_flops[3] = {0.0, 0.0, 0.0};
// classifies the path a call took (call.path) and adds its executed FLOPs
void tally(const es_conv_desc_t* d, es_dtype_t dt, const ConvCall& call) {
  double f = 2.0 * d->N * d->P * d->Q * (double)d->K * d->C * d->R * d->S;
  if (call.path & PATH_SUBPIXEL) f *= (double)es_subpixel_taps(d->R, d->S) / (4.0 * d->R * d->S);
  if (call.path & PATH_THIN) g_exec_flops[2] += f;
  else if (dt == ES_BF16) g_exec_flops[0] += f;
  else if (call.path & PATH_SPLIT) g_exec_flops[0] += 6.0 * f;
  else g_exec_flops[1] += f;
}

// Ends one conv entry: the entry's one read of the launch status (sticky until read), then the tally,
// only when the entry succeeded (failed calls issue no work).  Returns the entry's answer.
int finish(const char* entry, const es_conv_desc_t* d, es_dtype_t dt, const ConvCall& call, int rc) {
  if (rc != ES_OK) return rc;
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    es_set_error("%s: %s", entry, hipGetErrorString(e));
    return ES_ERR_HIP;
  }
  tally(d, dt, call);
  return ES_OK;
}

}  // namespace

// ------------------------------------------------------------ the three convolutions, per call context
int conv_fwd(const es_conv_desc_t* d, es_dtype_t dt, const void* x, const int64_t xs[4], const void* wk,
             const float* bias, void* y, es_dtype_t ydt, const int64_t ys[4], ConvCall& call, hipStream_t st) {
  if (int e = check_desc(d)) return e;
  if (d->subpixel) ES_CHECK_ARG(es_conv_subpixel_ok(d, dt), "conv fwd: sub-pixel weights for a conv the sub-pixel path cannot run");
  if (es_thin_conv_fwd(d, dt, x, xs, wk, bias, y, ydt, ys, call, st)) return ES_OK;
  ConvArgs a{};
  a.d = *d; a.a_src = x; a.b_src = wk; a.out = y; a.bias = bias; a.beta = 0.f;
  a.out_bf16 = ydt == ES_BF16;
  for (int i = 0; i < 4; ++i) { a.as[i] = xs[i]; a.os[i] = ys[i]; }
  a.M = d->N * d->P * d->Q; a.Ng = d->K; a.Kd = d->R * d->S * d->C;
  a.dense_f32_out = ydt == ES_F32 && dense_rows(ys, d->K, d->P, d->Q);
  fill_divs(a);
  return conv_dispatch(a, MODE_FWD, dt, vec16(dt, xs[1], d->C), vec16(dt, 1, a.Kd), call, st);
}

int conv_dgrad(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4], const void* wd,
               void* dxu, es_dtype_t dxdt, const int64_t dxs[4], float beta, ConvCall& call, hipStream_t st) {
  if (int e = check_desc(d)) return e;
  if (d->subpixel) ES_CHECK_ARG(es_conv_subpixel_ok(d, dt), "conv dgrad: sub-pixel weights for a conv the sub-pixel path cannot run");
  if (es_thin_conv_dgrad(d, dt, dy, ys, wd, dxu, dxdt, dxs, beta, call, st)) return ES_OK;
  ConvArgs a{};
  a.d = *d; a.a_src = dy; a.b_src = wd; a.out = dxu; a.bias = nullptr; a.beta = beta;
  a.out_bf16 = dxdt == ES_BF16;
  for (int i = 0; i < 4; ++i) { a.as[i] = ys[i]; a.os[i] = dxs[i]; }
  a.fold = d->up_h > 0;
  a.M = (int)dgrad_rows(*d, d->N); a.Ng = d->C;
  a.Kd = (a.fold ? d->up_h * d->up_w : 1) * d->R * d->S * d->K;
  a.dense_f32_out = dxdt == ES_F32 && beta == 0.f &&
                    dense_rows(dxs, d->C, a.fold ? d->H : d->Hu, a.fold ? d->W : d->Wu);
  fill_divs(a);
  return conv_dispatch(a, MODE_DGRAD, dt, vec16(dt, ys[1], d->K), vec16(dt, 1, a.Kd), call, st);
}

// dw += the weight gradient (packed layout, float atomics); with a deterministic workspace
// (call.det_ws) the call.det_splits raw per-split partials go there instead and the caller reduces them
int conv_wgrad(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4], const void* x,
               const int64_t xs[4], float* dw, ConvCall& call, hipStream_t st) {
  if (int e = check_desc(d)) return e;
  float* out = call.det_ws ? call.det_ws : dw;
  if (es_thin_conv_wgrad(d, dt, dy, ys, x, xs, out, call, st)) return ES_OK;
  ConvArgs a{};
  a.d = *d; a.a_src = dy; a.b_src = x; a.out = out;
  for (int i = 0; i < 4; ++i) { a.as[i] = ys[i]; a.bs[i] = xs[i]; }
  a.M = d->K; a.Ng = d->R * d->S * d->C; a.Kd = d->N * d->P * d->Q;
  a.det = call.det_ws != nullptr;
  fill_divs(a);
  return conv_dispatch(a, MODE_WGRAD, dt, vec16(dt, ys[1], d->K), vec16(dt, xs[1], d->C), call, st);
}

extern "C" int es_conv_exec_flops(double out[3], int reset) {
  ES_CHECK_ARG(out != nullptr, "conv exec flops: NULL out");
  for (int i = 0; i < 3; ++i) {
    out[i] = g_exec_flops[i];
    if (reset) g_exec_flops[i] = 0.0;
  }
  return ES_OK;
}

extern "C" int es_conv2d_fwd(const es_conv_desc_t* d, es_dtype_t dt, const void* x,
                             const int64_t xs[4], const void* wk, const float* bias, void* y,
                             es_dtype_t ydt, const int64_t ys[4], es_stream_t stream) {
  ConvCall call;
  return finish(__func__, d, dt, call, conv_fwd(d, dt, x, xs, wk, bias, y, ydt, ys, call, (hipStream_t)stream));
}

extern "C" int es_conv2d_fwd_stats(const es_conv_desc_t* d, es_dtype_t dt, const void* x, const int64_t xs[4],
                                   const void* wk, const float* bias, void* y, es_dtype_t ydt, const int64_t ys[4],
                                   float* part, int64_t part_floats, int* chunks, es_stream_t stream) {
  ES_CHECK_ARG(part && chunks, "conv fwd stats: part / chunks NULL");
  ConvCall call;
  call.stats_part = part;
  call.stats_floats = part_floats;
  const int rc = finish(__func__, d, dt, call, conv_fwd(d, dt, x, xs, wk, bias, y, ydt, ys, call, (hipStream_t)stream));
  *chunks = call.stats_chunks;
  return rc;
}

// es_conv2d_fwd with y = act(scale[k] * (acc + bias[k]) + shift[k]) applied before the rounding, when
// the kernel that runs the conv carries that epilogue (the ring FWD kernels of conv_ring_kernel.h in bf16
// and split-fp32); otherwise y is es_conv2d_fwd's and *fused = 0.
extern "C" int es_conv2d_fwd_affine(const es_conv_desc_t* d, es_dtype_t dt, const void* x, const int64_t xs[4],
                                    const void* wk, const float* bias, const es_affine_t* epi, void* y,
                                    es_dtype_t ydt, const int64_t ys[4], int* fused, es_stream_t stream) {
  ES_CHECK_ARG(epi && epi->scale && epi->shift && fused, "conv fwd affine: epi / scale / shift / fused NULL");
  ES_CHECK_ARG(epi->act == ES_ACT_NONE || epi->act == ES_ACT_RELU || epi->act == ES_ACT_LRELU,
               "conv fwd affine: unknown activation %d", epi->act);
  ConvCall call;
  call.aff = epi;
  const int rc = finish(__func__, d, dt, call, conv_fwd(d, dt, x, xs, wk, bias, y, ydt, ys, call, (hipStream_t)stream));
  *fused = rc == ES_OK ? call.aff_fused : 0;
  return rc;
}

extern "C" int es_conv2d_dgrad(const es_conv_desc_t* d, es_dtype_t dt, const void* dy,
                               const int64_t ys[4], const void* wd, void* dxu, es_dtype_t dxdt,
                               const int64_t dxs[4], float beta, es_stream_t stream) {
  ConvCall call;
  return finish(__func__, d, dt, call, conv_dgrad(d, dt, dy, ys, wd, dxu, dxdt, dxs, beta, call, (hipStream_t)stream));
}

extern "C" int es_conv2d_dgrad_bnred(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4],
                                     const void* wd, void* dx, es_dtype_t dxdt, const int64_t dxs[4],
                                     const void* x, const es_norm_t* nm, const es_chain_t* ch, float* part,
                                     int64_t part_floats, int* chunks, es_stream_t stream) {
  ES_CHECK_ARG(part && chunks && x && nm && ch, "conv dgrad bnred: NULL argument");
  ConvCall call;
  call.bnr_x = x; call.bnr_nm = nm; call.bnr_ch = ch;
  call.bnr_part = part;
  call.bnr_floats = part_floats;
  const int rc = finish(__func__, d, dt, call, conv_dgrad(d, dt, dy, ys, wd, dx, dxdt, dxs, 0.f, call, (hipStream_t)stream));
  *chunks = call.bnr_chunks;
  return rc;
}

extern "C" int es_conv2d_wgrad(const es_conv_desc_t* d, es_dtype_t dt, const void* dy,
                               const int64_t ys[4], const void* x, const int64_t xs[4], float* dw,
                               es_stream_t stream) {
  ConvCall call;
  return finish(__func__, d, dt, call, conv_wgrad(d, dt, dy, ys, x, xs, dw, call, (hipStream_t)stream));
}

// ------------------------------------------------------------------------- deterministic WGRAD
// (parity mode) dW = beta * dW + conv weight gradient, written in the torch layout [K][C][R][S] with
// a fixed summation order: the K splits store raw partials into the caller's workspace (no float
// atomics) and one ordered reduce sums them.  fp32 shapes the ring takes run wgrad_f32_kernel
// (conv_mfma.hip); the rest run the register-staged / thin kernels with per-split partials.
namespace {
// generic path: partial slots offered = clamp(2^26 floats / slot, 8, 2048) (small thin-conv slots
// keep their ~1024 blocks; the big linear slots stay within ~256 MB)
int64_t generic_det_floats(const es_conv_desc_t* d) {
  const int64_t per = (int64_t)d->K * d->R * d->S * d->C;
  return per * std::max<int64_t>(8, std::min<int64_t>(2048, (1ll << 26) / per));
}

ConvCall det_call(void* ws, int64_t ws_bytes) {
  ConvCall call;
  call.det_ws = (float*)ws;
  call.det_floats = ws_bytes / (int64_t)sizeof(float);
  return call;
}
}  // namespace

extern "C" int64_t es_conv2d_wgrad_det_ws_bytes(const es_conv_desc_t* d, es_dtype_t dt, const int64_t ys[4],
                                                const int64_t xs[4]) {
  if (!d || check_desc(d)) return -1;
  int64_t f = -1;
  if (dt == ES_F32) f = es_wgrad_f32_ring_floats(*d, ys, xs);
  if (f < 0) f = generic_det_floats(d);
  return f * (int64_t)sizeof(float);
}

extern "C" int es_conv2d_wgrad_det(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4],
                                   const void* x, const int64_t xs[4], float* dw, float beta, void* ws,
                                   int64_t ws_bytes, es_stream_t stream) {
  if (int e = check_desc(d)) return e;
  ES_CHECK_ARG(dw && ws, "conv wgrad det: NULL dw / workspace");
  const hipStream_t st = (hipStream_t)stream;
  ConvCall call = det_call(ws, ws_bytes);
  if (dt == ES_F32) {
    const int rc = es_wgrad_f32_ring(*d, dy, ys, x, xs, dw, beta, call, st);
    if (rc < 0) return ES_ERR_ARG;
    if (rc > 0) return finish(__func__, d, dt, call, ES_OK);
  }
  ES_CHECK_ARG(call.det_floats >= (int64_t)d->K * d->R * d->S * d->C, "conv wgrad det: workspace below one partial");
  if (int rc = conv_wgrad(d, dt, dy, ys, x, xs, dw, call, st)) return rc;
  ES_CHECK_ARG(call.det_splits > 0, "conv wgrad det: no partials written");
  es_wgrad_reduce_plain(call.det_ws, call.det_splits, d->K, d->C, d->R, d->S, dw, beta, st);
  return finish(__func__, d, dt, call, ES_OK);
}

// deterministic split-K FWD / DGRAD (the fp32 linears with few output tiles and a long K: the
// generator's fc2 dgrad, K = 21632 / 92160): the splits store partials into ws, one ordered sum
// (call.det_splits == 0: no split, the kernel wrote the output itself)
namespace {
constexpr int kDetSplitK = 16;
}  // namespace

extern "C" int64_t es_conv2d_splitk_ws_bytes(const es_conv_desc_t* d, int mode) {
  if (!d || check_desc(d) || (mode != MODE_FWD && mode != MODE_DGRAD)) return -1;
  const int64_t M = mode == MODE_FWD ? (int64_t)d->N * d->P * d->Q : dgrad_rows(*d, d->N);
  const int64_t Ng = mode == MODE_FWD ? d->K : d->C;
  return M * Ng * kDetSplitK * (int64_t)sizeof(float);
}

extern "C" int es_conv2d_fwd_det(const es_conv_desc_t* d, es_dtype_t dt, const void* x, const int64_t xs[4],
                                 const void* wk, const float* bias, void* y, es_dtype_t ydt, const int64_t ys[4],
                                 void* ws, int64_t ws_bytes, es_stream_t stream) {
  ES_CHECK_ARG(ws, "conv fwd det: NULL workspace");
  ConvCall call = det_call(ws, ws_bytes);
  if (int rc = conv_fwd(d, dt, x, xs, wk, bias, y, ydt, ys, call, (hipStream_t)stream)) return rc;
  if (call.det_splits)
    splitk_reduce_launch(call.det_ws, call.det_splits, (int64_t)d->N * d->P * d->Q * d->K, (float*)y, (hipStream_t)stream);
  return finish(__func__, d, dt, call, ES_OK);
}

extern "C" int es_conv2d_dgrad_det(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4],
                                   const void* wd, void* dxu, es_dtype_t dxdt, const int64_t dxs[4], void* ws,
                                   int64_t ws_bytes, es_stream_t stream) {
  ES_CHECK_ARG(ws, "conv dgrad det: NULL workspace");
  ConvCall call = det_call(ws, ws_bytes);
  if (int rc = conv_dgrad(d, dt, dy, ys, wd, dxu, dxdt, dxs, 0.f, call, (hipStream_t)stream)) return rc;
  if (call.det_splits)
    splitk_reduce_launch(call.det_ws, call.det_splits, dgrad_rows(*d, d->N) * d->C, (float*)dxu, (hipStream_t)stream);
  return finish(__func__, d, dt, call, ES_OK);
}
