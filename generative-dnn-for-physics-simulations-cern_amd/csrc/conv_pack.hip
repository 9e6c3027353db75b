// Weight packing for the convolution kernels: the fp32 master [K][C][R][S] into the GEMM layouts of
// FWD / DGRAD (plain, sub-pixel, split-fp32 planes), one by one or batched, and the packed weight
// gradient back into the torch layout.
#include <algorithm>

#include "conv_common.h"

namespace {
// sub-pixel combined weight W'_t[d][e] (t = 2a + b) at (k, c): sum over the covered taps
__device__ __forceinline__ float subpixel_weight(const float* __restrict__ w, int k, int c, int C, int R, int S,
                                                 int t, int dd, int ee) {
  const int a = t >> 1, b = t & 1;
  const int r0 = max(0, 2 * dd - a), r1 = min(R - 1, 2 * dd - a + 1);
  const int s0 = max(0, 2 * ee - b), s1 = min(S - 1, 2 * ee - b + 1);
  float v = 0.f;
  for (int r = r0; r <= r1; ++r)
    for (int s = s0; s <= s1; ++s) v += w[(((int64_t)k * C + c) * R + r) * S + s];
  return v;
}

// taps of class t: dh = ((a + R - 1) >> 1) + 1, dw likewise
__host__ __device__ __forceinline__ int64_t es_weight_planes_offset_d(int64_t n) { return (n * 4 + 255) / 256 * 256; }
__device__ __forceinline__ int sp_dh(int t, int R) { return (((t >> 1) + R - 1) >> 1) + 1; }
__device__ __forceinline__ int sp_dw(int t, int S) { return (((t & 1) + S - 1) >> 1) + 1; }

template <typename T>
__global__ void pack_subpixel_kernel(const float* __restrict__ w, int K, int C, int R, int S, int mode,
                                     const float* inv_scale, T* out) {
  int tap0[5];
  tap0[0] = 0;
  for (int t = 0; t < 4; ++t) tap0[t + 1] = tap0[t] + sp_dh(t, R) * sp_dw(t, S);
  const int taps = tap0[4];
  const int64_t n = (int64_t)K * C * taps;
  const float sc = inv_scale ? 1.f / inv_scale[0] : 1.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int k, c, tap;
    if (mode == 2) {   // class blocks [K][d][e][C]
      const int64_t kc = (int64_t)K * C;
      tap = 0;
      int t = (i >= tap0[1] * kc) + (i >= tap0[2] * kc) + (i >= tap0[3] * kc);
      const int64_t rem = i - tap0[t] * kc;
      const int nde = sp_dh(t, R) * sp_dw(t, S);
      k = (int)(rem / ((int64_t)nde * C));
      const int r2 = (int)(rem - (int64_t)k * nde * C);
      const int de = r2 / C;
      c = r2 - de * C;
      tap = tap0[t] + de;
    } else {           // [C][tap][K]
      c = (int)(i / ((int64_t)taps * K));
      const int r2 = (int)(i - (int64_t)c * taps * K);
      tap = r2 / K;
      k = r2 - tap * K;
    }
    const int t = (tap >= tap0[1]) + (tap >= tap0[2]) + (tap >= tap0[3]);
    const int de = tap - tap0[t], dw = sp_dw(t, S);
    const int dd = de / dw, ee = de - dd * dw;
    out[i] = from_f<T>(subpixel_weight(w, k, c, C, R, S, t, dd, ee) * sc);
  }
}

template <typename T>
__global__ void pack_weight_kernel(const float* __restrict__ w, int K, int C, int R, int S, int mode,
                                   const float* inv_scale, const int32_t* col_perm, T* out) {
  const int64_t n = (int64_t)K * C * R * S;
  const float sc = inv_scale ? 1.f / inv_scale[0] : 1.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    // i indexes the OUTPUT layout
    int k, c, r, s;
    const uint32_t i32 = (uint32_t)i;   // n < 2^31 (host-checked): 32-bit index math
    if (mode == 0) {  // [K][R][S][C]
      uint32_t t = i32 / C; c = i32 - t * C; s = t % S; t /= S; r = t % R; k = t / R;
    } else {          // [C][R][S][K]
      uint32_t t = i32 / K; k = i32 - t * K; s = t % S; t /= S; r = t % R; c = t / R;
    }
    const int cs = col_perm ? col_perm[c] : c;
    out[i] = from_f<T>(w[(((int64_t)k * C + cs) * R + r) * S + s] * sc);
  }
}

// mode 1 without a column permutation is a transpose of the fp32 master viewed as [K][C*R*S]
// into [C*R*S][K]: through a 64 x 64 LDS tile both sides stay row-contiguous (the element-wise
// kernel above read the master with a stride of C*R*S floats: 74 us for the 21632 x 256 linear)
template <typename T>
__global__ void __launch_bounds__(256) pack_t_kernel(const float* __restrict__ w, int rows, int cols,
                                                     const float* inv_scale, T* __restrict__ out) {
  __shared__ float tile[64][65];
  const float sc = inv_scale ? 1.f / inv_scale[0] : 1.f;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 64; i += 4) {
    const int r = r0 + ty + i, c = c0 + tx;
    if (r < rows && c < cols) tile[ty + i][tx] = w[(int64_t)r * cols + c];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 64; i += 4) {
    const int c = c0 + ty + i, r = r0 + tx;
    if (r < rows && c < cols) out[(int64_t)c * rows + r] = from_f<T>(tile[tx][ty + i] * sc);
  }
}

__global__ void unpack_grad_kernel(const float* __restrict__ dw, int K, int C, int R, int S,
                                   const int32_t* col_perm, float* grad, float beta) {
  const int64_t n = (int64_t)K * C * R * S;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    // i indexes dw layout [K][R][S][C]
    uint32_t t = (uint32_t)i / C;
    const int c = (int)((uint32_t)i - t * C);
    const int s = t % S; t /= S; const int r = t % R; const int k = t / R;
    const int cs = col_perm ? col_perm[c] : c;
    float* g = grad + (((int64_t)k * C + cs) * R + r) * S + s;
    *g = (beta != 0.f ? beta * *g : 0.f) + dw[i];
  }
}
// same, and the packed accumulator is left zeroed for the next weight gradient (each element is
// read and cleared by the one thread that owns it): no zero-fill launch per weight gradient
__global__ void unpack_grad_clear_kernel(float* __restrict__ dw, int K, int C, int R, int S, float* grad,
                                         float beta) {
  const int64_t n = (int64_t)K * C * R * S;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t t = (uint32_t)i / C;
    const int c = (int)((uint32_t)i - t * C);
    const int s = t % S; t /= S; const int r = t % R; const int k = t / R;
    float* g = grad + (((int64_t)k * C + c) * R + r) * S + s;
    const float v = dw[i];
    dw[i] = 0.f;
    *g = (beta != 0.f ? beta * *g : 0.f) + v;
  }
}
}  // namespace

extern "C" int es_pack_conv_weight(const float* w, int K, int C, int R, int S, int mode,
                                   const float* inv_scale, const int32_t* col_perm, void* out,
                                   es_dtype_t dt, es_stream_t stream) {
  ES_CHECK_ARG(mode >= 0 && mode <= 3, "pack: bad mode");
  if (mode >= 2) {
    ES_CHECK_ARG(col_perm == nullptr, "pack: sub-pixel modes take no column permutation");
    const int64_t n = (int64_t)K * C * es_subpixel_taps(R, S);
    ES_CHECK_ARG(n < (1ll << 31), "pack: weight too large");
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
    if (dt == ES_F32)
      hipLaunchKernelGGL(pack_subpixel_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                         w, K, C, R, S, mode, inv_scale, (float*)out);
    else
      hipLaunchKernelGGL(pack_subpixel_kernel<bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                         w, K, C, R, S, mode, inv_scale, (bf16*)out);
    ES_CHECK_LAUNCH();
    return ES_OK;
  }
  const int64_t n = (int64_t)K * C * R * S;
  ES_CHECK_ARG(n < (1ll << 31), "pack: weight too large");
  if (mode == 1 && col_perm == nullptr && (int64_t)C * R * S < 65535 * 64) {
    const int cols = C * R * S;
    const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((K + 63) / 64));
    if (dt == ES_F32)
      hipLaunchKernelGGL(pack_t_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, w, K, cols, inv_scale,
                         (float*)out);
    else
      hipLaunchKernelGGL(pack_t_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, w, K, cols, inv_scale,
                         (bf16*)out);
    ES_CHECK_LAUNCH();
    return ES_OK;
  }
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  if (dt == ES_F32)
    hipLaunchKernelGGL(pack_weight_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       w, K, C, R, S, mode, inv_scale, col_perm, (float*)out);
  else
    hipLaunchKernelGGL(pack_weight_kernel<bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       w, K, C, R, S, mode, inv_scale, col_perm, (bf16*)out);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

// Split-fp32 planes of a packed fp32 weight (es_conv_set_f32_split(2)): every 32-element block g
// of the packing becomes 192 bytes at planes + 192 g: three planes of 32 bf16, x0 = rne(x),
// x1 = rne(x - x0), x2 = x - x0 - x1 (exact), position 8 u + j of a plane holding element
// 4 u + j (j < 4) or 16 + 4 u + j - 4 of the block: the k order of the ring kernels' A fragments.
__global__ void pack_planes_kernel(const float* __restrict__ w, int64_t nblk, bf16* __restrict__ planes) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nblk * 32; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = i >> 5;
    const int q = (int)(i & 31), u = q >> 3, j = q & 7;
    const float x = w[g * 32 + (j < 4 ? 4 * u + j : 16 + 4 * u + j - 4)];
    const bf16 h = (bf16)x;
    const float r = x - (float)h;
    const bf16 m = (bf16)r;
    const bf16 l = (bf16)(r - (float)m);
    bf16* o = planes + g * 96 + q;
    o[0] = h;
    o[32] = m;
    o[64] = l;
  }
}

extern "C" int64_t es_weight_planes_offset(int64_t n) { return (n * 4 + 255) / 256 * 256; }

namespace {
// Batched packing (es_pack_conv_weights): blockIdx.y = job; each thread computes packed element i
// with the element-wise kernels' index math and writes it in the job's dtype, and for split-fp32
// jobs also its three bf16 plane values (the inverse of pack_planes_kernel's k permutation: block
// position p -> plane slot 8 (p / 4) + p % 4 for p < 16, 8 ((p - 16) / 4) + 4 + p % 4 otherwise).
constexpr int PACK_MAXJ = 32;
struct PackJobs {
  es_pack_job_t j[PACK_MAXJ];
};
__global__ void __launch_bounds__(256) pack_batch_kernel(PackJobs jobs) {
  const es_pack_job_t& jb = jobs.j[blockIdx.y];
  const int K = jb.K, C = jb.C, R = jb.R, S = jb.S, mode = jb.mode;
  int tap0[5] = {0, 0, 0, 0, 0};
  int64_t n;
  if (mode >= 2) {
    for (int t = 0; t < 4; ++t) tap0[t + 1] = tap0[t] + sp_dh(t, R) * sp_dw(t, S);
    n = (int64_t)K * C * tap0[4];
  } else {
    n = (int64_t)K * C * R * S;
  }
  const int64_t nplan = jb.planes ? (n / 32) * 32 : 0;
  bf16* planes = (bf16*)((char*)jb.out + es_weight_planes_offset_d(n));
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v;
    if (mode >= 2) {
      int k, c, tap;
      if (mode == 2) {
        const int64_t kc = (int64_t)K * C;
        const int t = (i >= tap0[1] * kc) + (i >= tap0[2] * kc) + (i >= tap0[3] * kc);
        const int64_t rem = i - tap0[t] * kc;
        const int nde = sp_dh(t, R) * sp_dw(t, S);
        k = (int)(rem / ((int64_t)nde * C));
        const int r2 = (int)(rem - (int64_t)k * nde * C);
        const int de = r2 / C;
        c = r2 - de * C;
        tap = tap0[t] + de;
      } else {
        const int taps = tap0[4];
        c = (int)(i / ((int64_t)taps * K));
        const int r2 = (int)(i - (int64_t)c * taps * K);
        tap = r2 / K;
        k = r2 - tap * K;
      }
      const int t = (tap >= tap0[1]) + (tap >= tap0[2]) + (tap >= tap0[3]);
      const int de = tap - tap0[t], dw = sp_dw(t, S);
      const int dd = de / dw, ee = de - dd * dw;
      v = subpixel_weight(jb.w, k, c, C, R, S, t, dd, ee);
    } else {
      int k, c, r, s_;
      const uint32_t i32 = (uint32_t)i;
      if (mode == 0) {
        uint32_t t = i32 / C; c = i32 - t * C; s_ = t % S; t /= S; r = t % R; k = t / R;
      } else {
        uint32_t t = i32 / K; k = i32 - t * K; s_ = t % S; t /= S; r = t % R; c = t / R;
      }
      v = jb.w[(((int64_t)k * C + c) * R + r) * S + s_];
    }
    if (jb.dt == ES_BF16) {
      ((bf16*)jb.out)[i] = (bf16)v;
    } else {
      ((float*)jb.out)[i] = v;
      if (i < nplan) {
        const int p = (int)(i & 31);
        const int q = p < 16 ? 8 * (p >> 2) + (p & 3) : 8 * ((p - 16) >> 2) + 4 + (p & 3);
        const bf16 h = (bf16)v;
        const float rr = v - (float)h;
        const bf16 m = (bf16)rr;
        const bf16 l = (bf16)(rr - (float)m);
        bf16* o = planes + (i >> 5) * 96 + q;
        o[0] = h;
        o[32] = m;
        o[64] = l;
      }
    }
  }
}
}  // namespace

extern "C" int es_pack_conv_weights(const es_pack_job_t* jobs, int n, es_stream_t stream) {
  ES_CHECK_ARG(n >= 0 && (n == 0 || jobs != nullptr), "pack batch: bad job list");
  hipStream_t st = (hipStream_t)stream;
  PackJobs batch{};
  int nb = 0;
  int64_t maxn = 0;
  auto flush = [&]() -> int {
    if (nb == 0) return ES_OK;
    const int blocks = (int)std::min<int64_t>((maxn + 255) / 256, 512);
    hipLaunchKernelGGL(pack_batch_kernel, dim3(blocks, nb), dim3(256), 0, st, batch);
    ES_CHECK_LAUNCH();
    nb = 0;
    maxn = 0;
    return ES_OK;
  };
  for (int q = 0; q < n; ++q) {
    const es_pack_job_t& jb = jobs[q];
    ES_CHECK_ARG(jb.w && jb.out && jb.mode >= 0 && jb.mode <= 3 && jb.K > 0 && jb.C > 0 && jb.R > 0 && jb.S > 0,
                 "pack batch: bad job %d", q);
    ES_CHECK_ARG(jb.dt == ES_F32 || jb.dt == ES_BF16, "pack batch: job %d dtype", q);
    ES_CHECK_ARG(!jb.planes || jb.dt == ES_F32, "pack batch: planes need an fp32 packing (job %d)", q);
    const int64_t ne = (int64_t)jb.K * jb.C * (jb.mode >= 2 ? es_subpixel_taps(jb.R, jb.S) : jb.R * jb.S);
    ES_CHECK_ARG(ne < (1ll << 31), "pack batch: weight too large (job %d)", q);
    if (jb.mode == 1 && (int64_t)jb.C * jb.R * jb.S >= 4096) {
      // a large transpose (the wide linears): the LDS-tiled kernel, then its planes
      if (int rc = es_pack_conv_weight(jb.w, jb.K, jb.C, jb.R, jb.S, 1, nullptr, nullptr, jb.out, (es_dtype_t)jb.dt,
                                       stream))
        return rc;
      if (jb.planes)
        if (int rc = es_pack_weight_planes((const float*)jb.out, ne, jb.out, stream)) return rc;
      continue;
    }
    batch.j[nb++] = jb;
    maxn = std::max(maxn, ne);
    if (nb == PACK_MAXJ)
      if (int rc = flush()) return rc;
  }
  return flush();
}

extern "C" int es_pack_weight_planes(const float* packed, int64_t n, void* base, es_stream_t stream) {
  const int64_t nblk = n / 32;
  if (nblk == 0) return ES_OK;
  const int blocks = (int)std::min<int64_t>((nblk * 32 + 255) / 256, 4096);
  hipLaunchKernelGGL(pack_planes_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, packed, nblk,
                     (bf16*)((char*)base + es_weight_planes_offset(n)));
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_unpack_conv_grad_clear(float* dw, int K, int C, int R, int S, float* grad, float beta,
                                         es_stream_t stream) {
  const int64_t n = (int64_t)K * C * R * S;
  ES_CHECK_ARG(n < (1ll << 31), "unpack: weight too large");
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(unpack_grad_clear_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dw, K, C, R, S,
                     grad, beta);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_unpack_conv_grad(const float* dw, int K, int C, int R, int S,
                                   const int32_t* col_perm, float* grad, float beta,
                                   es_stream_t stream) {
  const int64_t n = (int64_t)K * C * R * S;
  ES_CHECK_ARG(n < (1ll << 31), "unpack: weight too large");
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(unpack_grad_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dw, K, C,
                     R, S, col_perm, grad, beta);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
