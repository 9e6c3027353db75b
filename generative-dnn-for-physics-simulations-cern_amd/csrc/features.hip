// Shower-shape observables of a calorimeter image (train/utils.py:81-112):
//   calculate_image_features          train/utils.py:85-112  largest column sum, largest row sum, centre of
//                                                            the hit mask (v > 0) in x and y, hit-pixel count
//   get_max_value_image_coordinates   train/utils.py:81-82   (row, col) of the first maximum, row-major
//   np.expm1 of the log1p-domain images                      moe.py:646, train/utils.py:198 (fused here, the
//                                                            float32 expm1f of es_channel_sums / es_sim_finish)
//
// One wave per image, four images per 256-thread block (two per 128-thread block once four staged images
// pass 64 KiB of LDS).  Pass 1: every lane walks the image with a 64-pixel stride (coalesced row-major
// loads, each pixel read from HBM once), stores the float32 value into the wave's LDS tile and keeps the
// integer hit count, the integer index sums of the hits and its own first maximum.  Pass 2 reads the tile
// twice: lane j sums column j over i = 0..h-1 and lane i sums row i over j = 0..w-1, both in fp64, in that
// order, starting from +0.0 (so a sum is never -0.0).  The wave then reduces with shuffles only: max of the
// sums (exact in any order), integer adds, and (value, index) pairs with the smaller index winning a tie.
// No atomics; an image's result depends on its pixels alone.
//
// LDS row pitch: w | 1 floats (the smallest odd number >= w).  The column walk has a lane-to-lane stride of
// one float and is conflict-free under any pitch.  The row walk has a lane-to-lane stride of one row:
// ds_read_b32 banks are (dword address) mod 32 over each 32-lane half, and an odd pitch is coprime with 32,
// so the 32 lanes of a half fall on 32 different banks (pitch 64 would put all of them on one bank, a
// 32-way conflict; pitch 44 on 8 banks).  Tile: h * (w | 1) * 4 bytes per image, 7.9 KB at 44x44.
// HBM-bound: h*w*sizeof(dtype) bytes read and 48 bytes written per image.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int FEAT_MAX_DIM = 64;
constexpr int FEAT_LDS_MAX = 65536;

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

template <typename T>
__global__ void __launch_bounds__(256) image_features_kernel(const T* __restrict__ x, int n, int h, int w,
                                                             int64_t sn, int64_t sh, int64_t sw, int log_domain,
                                                             double* __restrict__ feat, int32_t* __restrict__ peak) {
  extern __shared__ float tile_all[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int img = blockIdx.x * (blockDim.x >> 6) + wid;
  const int pitch = w | 1;
  float* tile = tile_all + wid * h * pitch;
  const bool live = img < n;                  // wave-uniform; a dead wave only joins the barrier
  const int hw = h * w;
  int cnt = 0, sx = 0, sy = 0;
  float best_v = -INFINITY;
  int best_i = INT_MAX;                       // INT_MAX: this lane has seen no pixel
  if (live) {
    const T* p = x + (int64_t)img * sn;
    // pixel index i = lane + 64k, tracked as (row, col) without a division per pixel
    int r = lane / w, c = lane - (lane / w) * w;
    const int dr = 64 / w, dc = 64 - (64 / w) * w;
    for (int i = lane; i < hw; i += 64) {
      float v = to_f(p[r * sh + c * sw]);
      if (log_domain) v = expm1f(v);          // float32 expm1, as numpy on the float32 array
      tile[r * pitch + c] = v;
      const bool hit = v > 0.f;
      cnt += hit ? 1 : 0;
      sx += hit ? c : 0;
      sy += hit ? r : 0;
      if (best_i == INT_MAX || v > best_v) { best_v = v; best_i = i; }   // i ascends: the first maximum stays
      r += dr;
      c += dc;
      if (c >= w) { c -= w; ++r; }
    }
  }
  __syncthreads();
  if (!live) return;
  double col = -INFINITY, row = -INFINITY;
  if (feat) {
    if (lane < w) {
      col = 0.0;
      for (int i = 0; i < h; ++i) col += (double)tile[i * pitch + lane];
    }
    if (lane < h) {
      row = 0.0;
      const float* q = tile + lane * pitch;
      for (int j = 0; j < w; ++j) row += (double)q[j];
    }
    col = wave_max_d(col);
    row = wave_max_d(row);
    cnt = wave_sum_i(cnt);
    sx = wave_sum_i(sx);
    sy = wave_sum_i(sy);
  }
  if (peak) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best_v, o, 64);
      const int oi = __shfl_xor(best_i, o, 64);
      if (ov > best_v || (ov == best_v && oi < best_i)) { best_v = ov; best_i = oi; }
    }
  }
  if (lane == 0) {
    if (feat) {
      double* f = feat + (int64_t)img * 5;
      f[0] = col;
      f[1] = row;
      f[2] = cnt > 0 ? (double)sx / (double)cnt : (double)w / 2.0;
      f[3] = cnt > 0 ? (double)sy / (double)cnt : (double)h / 2.0;
      f[4] = (double)cnt;
    }
    if (peak) {
      peak[(int64_t)img * 2] = best_i / w;
      peak[(int64_t)img * 2 + 1] = best_i - (best_i / w) * w;
    }
  }
}

}  // namespace

extern "C" int es_image_features(const es_view_t* x, es_dtype_t dt, const void* xp, int log_domain, double* feat,
                                 int32_t* peak, es_stream_t stream) {
  ES_CHECK_ARG(x && xp, "image_features: null argument");
  ES_CHECK_ARG(feat || peak, "image_features: both outputs are NULL");
  ES_CHECK_ARG(x->c == 1, "image_features: images must have one channel (got %d)", x->c);
  ES_CHECK_ARG(x->h >= 1 && x->w >= 1 && x->h <= FEAT_MAX_DIM && x->w <= FEAT_MAX_DIM,
               "image_features: image %dx%d outside 1..%d", x->h, x->w, FEAT_MAX_DIM);
  ES_CHECK_ARG(x->n >= 0, "image_features: negative count");
  if (x->n == 0) return ES_OK;
  const int tile_bytes = x->h * (x->w | 1) * (int)sizeof(float);
  const int per_block = 4 * tile_bytes <= FEAT_LDS_MAX ? 4 : 2;
  const dim3 grid((x->n + per_block - 1) / per_block), block(64 * per_block);
  const size_t lds = (size_t)per_block * tile_bytes;
  if (dt == ES_BF16)
    hipLaunchKernelGGL(image_features_kernel<bf16>, grid, block, lds, (hipStream_t)stream, (const bf16*)xp, x->n,
                       x->h, x->w, x->s[0], x->s[2], x->s[3], log_domain, feat, peak);
  else
    hipLaunchKernelGGL(image_features_kernel<float>, grid, block, lds, (hipStream_t)stream, (const float*)xp, x->n,
                       x->h, x->w, x->s[0], x->s[2], x->s[3], log_domain, feat, peak);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
