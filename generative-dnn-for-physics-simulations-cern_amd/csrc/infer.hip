// Simulation (inference) kernels: conditions in, calorimeter images out.
//   es_bn_fold / es_bn_fold_batch   an eval-mode BatchNorm as a per-channel affine (scale, shift), the
//                                   operand of es_conv2d_fwd_affine's epilogue (neutron/generator.py:13-36)
//   es_sim_finish                   relu -> (expm1) -> scatter into batch order (+ the five channel sums)
//                                   of one expert's rows (train/utils.py:179-266, 62-78)
// Both are memory-bound single passes: the fold moves 24 bytes per channel; the finish reads
// H*W*4 bytes and writes H*W*4 + 40 bytes per live image.
#include "common.h"

namespace {

struct FoldJobs {
  const float* gamma[ES_BN_FOLD_MAX];
  const float* beta[ES_BN_FOLD_MAX];
  const float* mean[ES_BN_FOLD_MAX];
  const float* var[ES_BN_FOLD_MAX];
  float* scale[ES_BN_FOLD_MAX];
  float* shift[ES_BN_FOLD_MAX];
  int C[ES_BN_FOLD_MAX];
  float eps[ES_BN_FOLD_MAX];
  int blk0[ES_BN_FOLD_MAX + 1];   // first block of each job (prefix sums of ceil(C / 256))
  int n;
};

// (rsqrtf then one multiply, shift as an fma-free product and subtraction: the single and the batched
// launch run this one function, so they agree bit for bit)
__device__ __forceinline__ void fold_one(const float* gamma, const float* beta, const float* mean, const float* var,
                                         float eps, int c, float* scale, float* shift) {
  const float sc = (gamma ? gamma[c] : 1.f) * rsqrtf(var[c] + eps);
  scale[c] = sc;
  shift[c] = __fsub_rn(beta ? beta[c] : 0.f, __fmul_rn(mean[c], sc));
}

__global__ void __launch_bounds__(256) bn_fold_kernel(FoldJobs j) {
  int k = 0;
  while (k + 1 < j.n && (int)blockIdx.x >= j.blk0[k + 1]) ++k;   // (block-uniform)
  const int c = ((int)blockIdx.x - j.blk0[k]) * 256 + threadIdx.x;
  if (c < j.C[k]) fold_one(j.gamma[k], j.beta[k], j.mean[k], j.var[k], j.eps[k], c, j.scale[k], j.shift[k]);
}

// One wave per live image, four images per block, the pixel walk and the fp64 accumulation of
// channel_sums_kernel (eval.hip): the sums equal es_channel_sums(log_domain = 1) of the stored
// log-domain image.
__global__ void __launch_bounds__(256) sim_finish_kernel(const float* __restrict__ x, int cap, int h, int w, int64_t sn,
                                                         int64_t sh, int64_t sw, const int32_t* __restrict__ live,
                                                         const int32_t* __restrict__ perm,
                                                         const int32_t* __restrict__ start, int photons,
                                                         float* __restrict__ out, double* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int img = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (img >= live_rows(live, cap)) return;    // whole wave exits together (no block barrier below)
  const int dst = perm ? perm[start[0] + img] : img;
  const float* p = x + (int64_t)img * sn;
  const int mid_r = h >> 1, mid_c = w >> 1;
  const int hw = h * w;
  float* o = out ? out + (int64_t)dst * hw : nullptr;
  int r = lane / w, c = lane - (lane / w) * w;
  const int dr = 64 / w, dc = 64 - (64 / w) * w;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = lane; i < hw; i += 64) {
    const float v = fmaxf(p[r * sh + c * sw], 0.f);
    const float e = expm1f(v);
    if (o) o[i] = photons ? e : v;
    int ch;
    if (((r + c) & 1) == 0) ch = 4;
    else ch = (r < mid_r ? 2 : 0) + (c < mid_c ? 0 : 1);
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[k] += (ch == k) ? (double)e : 0.0;
    r += dr;
    c += dc;
    if (c >= w) { c -= w; ++r; }
  }
  if (sums == nullptr) return;
#pragma unroll
  for (int k = 0; k < 5; ++k) acc[k] = wave_sum_d(acc[k]);
  if (lane < 5) {
    double v = acc[0];
#pragma unroll
    for (int k = 1; k < 5; ++k) v = (lane == k) ? acc[k] : v;
    sums[(int64_t)dst * 5 + lane] = v;
  }
}

}  // namespace

extern "C" int es_bn_fold_batch(int n, const float* const* gamma, const float* const* beta,
                                const float* const* running_mean, const float* const* running_var, const int* C,
                                const float* eps, float* const* scale, float* const* shift, es_stream_t stream) {
  ES_CHECK_ARG(n >= 0 && n <= ES_BN_FOLD_MAX, "bn_fold_batch: n = %d outside [0, %d]", n, ES_BN_FOLD_MAX);
  if (n == 0) return ES_OK;
  ES_CHECK_ARG(gamma && beta && running_mean && running_var && C && eps && scale && shift, "bn_fold_batch: NULL array");
  FoldJobs j{};
  j.n = n;
  j.blk0[0] = 0;
  for (int i = 0; i < n; ++i) {
    ES_CHECK_ARG(C[i] > 0 && running_mean[i] && running_var[i] && scale[i] && shift[i],
                 "bn_fold_batch: job %d has no channels or a NULL pointer", i);
    j.gamma[i] = gamma[i]; j.beta[i] = beta[i]; j.mean[i] = running_mean[i]; j.var[i] = running_var[i];
    j.scale[i] = scale[i]; j.shift[i] = shift[i]; j.C[i] = C[i]; j.eps[i] = eps[i];
    j.blk0[i + 1] = j.blk0[i] + (C[i] + 255) / 256;
  }
  hipLaunchKernelGGL(bn_fold_kernel, dim3(j.blk0[n]), dim3(256), 0, (hipStream_t)stream, j);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                          int C, float eps, float* scale, float* shift, es_stream_t stream) {
  return es_bn_fold_batch(1, &gamma, &beta, &running_mean, &running_var, &C, &eps, &scale, &shift, stream);
}

extern "C" int es_sim_finish(const es_view_t* x, const void* xp, const int32_t* live, const int32_t* perm,
                             const int32_t* start, int photons, float* out, double* sums, es_stream_t stream) {
  ES_CHECK_ARG(x && xp, "sim_finish: null argument");
  ES_CHECK_ARG(x->c == 1, "sim_finish: images must have one channel (got %d)", x->c);
  ES_CHECK_ARG(x->h > 0 && x->w > 0, "sim_finish: empty image %dx%d", x->h, x->w);
  ES_CHECK_ARG(x->n >= 0, "sim_finish: negative count");
  ES_CHECK_ARG(perm == nullptr || start != nullptr, "sim_finish: perm without start");
  if (x->n == 0 || (out == nullptr && sums == nullptr)) return ES_OK;
  hipLaunchKernelGGL(sim_finish_kernel, dim3((x->n + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const float*)xp,
                     x->n, x->h, x->w, x->s[0], x->s[2], x->s[3], live, perm, start, photons, out, sums);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
