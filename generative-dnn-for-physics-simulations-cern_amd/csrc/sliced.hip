// Sliced Wasserstein distance of whole images: the projection of n images of D = h * w pixels
// onto n_proj directions in fp64, and the unit directions themselves.  The 1-D distances of the projected columns
// are es_wasserstein_1d's (wasserstein.hip, untouched), the moments over the directions es_segment_moments'.
//
// es_sliced_project: out[b][p] = sum_d x[b][d] * theta[p][d], an n x D x n_proj GEMM on v_mfma_f64_16x16x4_f64.
//   A (16 images x 4 pixels) and B (4 pixels x 16 directions) take the f32 16x16x4 lane map, one f64 per lane:
//   lane l holds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15].  C/D is the f64 map: register r of lane l is
//   row (l >> 4) + 4 r, column l & 15 (the f32 formula (l >> 4) * 4 + r runs clean and is wrong).
//   Workgroup: 256 threads, SL_BM = 32 images x SL_BP = 256 directions; wave w owns the direction tiles
//   w, w + 4, w + 8, w + 12 of the workgroup's chunk and both image tiles: 8 accumulators of 4 f64.  With
//   n_proj <= 256 the grid has one column, so every image is read from HBM once.
//   Staging: SL_KC = 16 pixels at a time.  The images go to LDS as fp32 (bf16 widened exactly) and are widened
//   to fp64 on the load into the A operand, the directions as fp64; one image chunk in LDS serves every
//   direction tile of the workgroup.  The next chunk's global loads are issued into registers before the
//   current chunk's MFMAs and stored to LDS after them (one LDS buffer, two barriers per chunk).
//   Order: every output element is ONE accumulator chain from +0.0 over the k-steps d0 = 0, 4, 8, ... in
//   ascending order -- no split over D, no atomics.  Pixels from D to the next multiple of 4 are +0.0 operands,
//   never read from memory; the tile rows past n and the tile columns past n_proj repeat the last live one and
//   are not stored.  An element's value is a function of its image row and its direction alone: bit-equal on
//   rerun, whatever n, n_proj, the positions or the strides.
//
// es_sliced_directions: one workgroup per direction; the d draws of the row (es_randn's: randn_pair
//   below) go to LDS, thread t adds the fp64 squares of draws t, t + 256, ... in that order, block_sum_d adds
//   the threads in a fixed order, and every draw is divided by the square root of that sum.
#include "common.h"
#include "segment.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int SL_THREADS = 256;
constexpr int SL_BM = 32;                  // images of a workgroup: two 16-row tiles
constexpr int SL_BP = 256;                 // directions of a workgroup: up to sixteen 16-column tiles
constexpr int SL_KC = 16;                  // pixels staged at a time: four k-steps
constexpr int SL_APITCH = SL_KC + 1;       // floats; odd, so the 16 rows of a fragment fall on different banks
constexpr int SL_BPITCH = SL_KC + 1;       // doubles
constexpr int SL_TILES = SL_BP / 16;       // direction tiles of a workgroup
constexpr int SL_WAVES = SL_THREADS / 64;
constexpr int SL_TPW = SL_TILES / SL_WAVES;   // direction tiles of a wave
constexpr int SL_MAX_D = ES_SLICED_MAX_D;
constexpr int SL_MAX_PROJ = ES_SLICED_MAX_PROJ;
constexpr int SL_MAX_N = 1 << 20;

// Draws 2q and 2q + 1 of es_randn's stream `sid`: randn_kernel's pair (misc.hip) restated term for term over the
// shared philox4x32_10, so that the training step's objects stay as they are; tests/test_sliced_gpu.py holds the
// directions to es_randn's own draws.
__device__ __forceinline__ void randn_pair(uint64_t seed, uint32_t sid, int64_t q, float& even, float& odd) {
  u32x4 r = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), sid, 0x5EED0001u, (uint32_t)seed,
                          (uint32_t)(seed >> 32));
  const float u1 = ((r.x >> 8) + 1) * (1.f / 16777217.f);   // (0, 1]
  const float u2 = (r.y >> 8) * (1.f / 16777216.f);
  const float rad = sqrtf(-2.f * logf(u1));
  float s, c;
  sincosf(6.2831853071795864f * u2, &s, &c);
  even = rad * c;
  odd = rad * s;
}

template <typename T>
__global__ void __launch_bounds__(SL_THREADS)
sliced_project_kernel(const T* __restrict__ x, int n, int h, int w, int64_t sn, int64_t sh, int64_t sw,
                      const double* __restrict__ theta, int64_t theta_ld, int n_proj, double* __restrict__ out,
                      int64_t out_ld) {
  __shared__ float sA[SL_BM * SL_APITCH];
  __shared__ double sB[SL_BP * SL_BPITCH];
  const int D = h * w;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b0 = blockIdx.x * SL_BM, p0 = blockIdx.y * SL_BP;
  const int np = n_proj - p0 < SL_BP ? n_proj - p0 : SL_BP;     // live directions of this workgroup, >= 1
  const int ntile = (np + 15) >> 4;

  // staging: thread -> pixel sk of the chunk, image rows sr and sr + 16, direction sr of every live tile
  const int sk = tid & 15, sr = tid >> 4;
  float ra[2];
  double rb[SL_TILES];
  // Rows past n and directions past n_proj are clamped to the last live one: in-bounds reads whose products land
  // in output elements that are never stored.  Only the pixels past D must be +0.0 on both sides.
  const int rlast = n - 1 - b0, plast = np - 1;
  const T* xrow[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int br = sr + 16 * r;
    xrow[r] = x + (int64_t)(b0 + (br < rlast ? br : rlast)) * sn;
  }
  auto fetch = [&](int d0) {
    const int d = d0 + sk;
    const bool dok = d < D;
    const int i = d / w, j = d - i * w;
    const int64_t off = (int64_t)i * sh + (int64_t)j * sw;
#pragma unroll
    for (int r = 0; r < 2; ++r) ra[r] = dok ? to_f(xrow[r][off]) : 0.f;
#pragma unroll
    for (int t = 0; t < SL_TILES; ++t) {
      if (t < ntile) {                                           // block-uniform
        const int p = 16 * t + sr;
        rb[t] = dok ? theta[(int64_t)(p0 + (p < plast ? p : plast)) * theta_ld + d] : 0.0;
      }
    }
  };

  f64x4 acc[2][SL_TPW];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int t = 0; t < SL_TPW; ++t) acc[r][t] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int fr = lane & 15, fk = lane >> 4;                       // fragment row / column and k of this lane
  fetch(0);
  for (int d0 = 0; d0 < D; d0 += SL_KC) {
#pragma unroll
    for (int r = 0; r < 2; ++r) sA[(sr + 16 * r) * SL_APITCH + sk] = ra[r];
#pragma unroll
    for (int t = 0; t < SL_TILES; ++t)
      if (t < ntile) sB[(16 * t + sr) * SL_BPITCH + sk] = rb[t];
    __syncthreads();
    if (d0 + SL_KC < D) fetch(d0 + SL_KC);
    const int rem = D - d0;
    const int ksteps = rem >= SL_KC ? SL_KC / 4 : (rem + 3) >> 2;  // block-uniform
    for (int kk = 0; kk < ksteps; ++kk) {
      const double a0 = (double)sA[fr * SL_APITCH + 4 * kk + fk];
      const double a1 = (double)sA[(fr + 16) * SL_APITCH + 4 * kk + fk];
#pragma unroll
      for (int t = 0; t < SL_TPW; ++t) {
        const int tile = wid + SL_WAVES * t;
        if (tile < ntile) {                                      // wave-uniform
          const double b = sB[(16 * tile + fr) * SL_BPITCH + 4 * kk + fk];
          acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][t], 0, 0, 0);
          acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // C/D, the f64 map: register g of lane l is row (l >> 4) + 4 g, column l & 15
#pragma unroll
  for (int t = 0; t < SL_TPW; ++t) {
    const int p = 16 * (wid + SL_WAVES * t) + fr;
    if (p >= np) continue;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int b = b0 + 16 * r + fk + 4 * g;
        if (b < n) out[(int64_t)b * out_ld + p0 + p] = acc[r][t][g];
      }
    }
  }
}

__global__ void __launch_bounds__(SL_THREADS)
sliced_directions_kernel(double* __restrict__ theta, int64_t theta_ld, int d, uint64_t seed, uint32_t sid) {
  __shared__ float draws[SL_MAX_D];
  __shared__ double shd[SL_WAVES];
  const int p = blockIdx.x, half = (d + 1) >> 1;                  // D2 / 2 pairs a row
  for (int i = threadIdx.x; i < half; i += SL_THREADS) {
    float even, odd;
    randn_pair(seed, sid, (int64_t)p * half + i, even, odd);
    draws[2 * i] = even;
    if (2 * i + 1 < d) draws[2 * i + 1] = odd;
  }
  __syncthreads();
  double ss = 0.0;
  for (int e = threadIdx.x; e < d; e += SL_THREADS) {
    const double v = (double)draws[e];
    ss += v * v;                                                  // the square of a widened fp32 is exact
  }
  const double norm = sqrt(block_sum_d(ss, shd));
  for (int e = threadIdx.x; e < d; e += SL_THREADS) theta[(int64_t)p * theta_ld + e] = (double)draws[e] / norm;
}

}  // namespace

extern "C" int es_sliced_project(const es_view_t* x, es_dtype_t dt, const void* xp, const double* theta,
                                 int64_t theta_ld, int n_proj, double* out, int64_t out_ld, es_stream_t stream) {
  ES_CHECK_ARG(x && xp && theta && out, "sliced_project: null argument");
  ES_CHECK_ARG(dt == ES_F32 || dt == ES_BF16, "sliced_project: dtype %d", (int)dt);
  ES_CHECK_ARG(x->c == 1, "sliced_project: images must have one channel (got %d)", x->c);
  ES_CHECK_ARG(x->h >= 1 && x->w >= 1 && (int64_t)x->h * x->w <= SL_MAX_D, "sliced_project: image %dx%d outside 1..%d pixels",
               x->h, x->w, SL_MAX_D);
  ES_CHECK_ARG(n_proj >= 1 && n_proj <= SL_MAX_PROJ, "sliced_project: n_proj=%d outside 1..%d", n_proj, SL_MAX_PROJ);
  ES_CHECK_ARG(x->n >= 0 && x->n <= SL_MAX_N, "sliced_project: n=%d outside 0..%d", x->n, SL_MAX_N);
  ES_CHECK_ARG(theta_ld >= (int64_t)x->h * x->w, "sliced_project: theta_ld=%lld below %d pixels", (long long)theta_ld,
               x->h * x->w);
  ES_CHECK_ARG(out_ld >= n_proj, "sliced_project: out_ld=%lld below n_proj=%d", (long long)out_ld, n_proj);
  if (x->n == 0) return ES_OK;
  const dim3 grid((x->n + SL_BM - 1) / SL_BM, (n_proj + SL_BP - 1) / SL_BP), block(SL_THREADS);
  if (dt == ES_BF16)
    hipLaunchKernelGGL(sliced_project_kernel<bf16>, grid, block, 0, (hipStream_t)stream, (const bf16*)xp, x->n, x->h,
                       x->w, x->s[0], x->s[2], x->s[3], theta, theta_ld, n_proj, out, out_ld);
  else
    hipLaunchKernelGGL(sliced_project_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)xp, x->n, x->h,
                       x->w, x->s[0], x->s[2], x->s[3], theta, theta_ld, n_proj, out, out_ld);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_sliced_directions(double* theta, int64_t theta_ld, int n_proj, int d, uint64_t seed,
                                    uint32_t stream_id, es_stream_t stream) {
  ES_CHECK_ARG(theta, "sliced_directions: null argument");
  ES_CHECK_ARG(d >= 1 && d <= SL_MAX_D, "sliced_directions: d=%d outside 1..%d", d, SL_MAX_D);
  ES_CHECK_ARG(n_proj >= 1 && n_proj <= SL_MAX_PROJ, "sliced_directions: n_proj=%d outside 1..%d", n_proj, SL_MAX_PROJ);
  ES_CHECK_ARG(theta_ld >= d, "sliced_directions: theta_ld=%lld below d=%d", (long long)theta_ld, d);
  hipLaunchKernelGGL(sliced_directions_kernel, dim3(n_proj), dim3(SL_THREADS), 0, (hipStream_t)stream, theta, theta_ld,
                     d, seed, stream_id);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
