// Distances between joint distributions of the shower observables: per-segment mean and
// covariance, the Frechet distance between the fitted Gaussians and the all-pairs sums of a polynomial kernel
// behind the unbiased MMD^2 (Kansal et al. 2023).  include/expertsim_hip.h defines every entry to the letter;
// this header says how the work is laid out.
//
// es_segment_moments: three launches.  mo_mean_kernel, grid (run, segment): thread (row lane t >> 5, column
// t & 31) walks every eighth member of its run, the eight lanes are added in order through LDS.  mo_cov_kernel,
// same grid: the mean is rebuilt from the runs' partials (the same order, so the same bits, in every
// workgroup), 64 members at a time are centred into LDS and thread t walks them for the pairs (i <= j) number
// t, t + 256, t + 512.  mo_final_kernel, one workgroup per segment: the runs in order, the divisions, the
// mirror and the NaN rules.
//
// es_frechet: fr_kernel, one wave per problem, A, B, V and two scratch matrices in LDS (pitch 33).  Lane r owns
// row r.  The cyclic Jacobi is es_pca_project's rotation and threshold, but it is a second copy: that one keeps
// V in global memory and ends in its own sort / sign epilogue inside the kernel, and moving it to a header would
// mean recompiling it inside another function; this file leaves embedding.hip alone so that es_pca_project's
// bits cannot move.
//
// es_mmd_poly: mm_pair_kernel is fidelity.hip's pair walk with a dot product in place of the squared
// difference: grid (A tile, run of B tiles, 3 * segment + matrix), matrix 0 = real x real, 1 = generated x
// generated, 2 = real x generated; 256 threads hold 8 x 8 pairs each in fp64, the columns come through LDS in
// chunks of 16 (fp32, column-major, widened on load).  The Gram tile runs on the fp64 vector FMA, not on
// v_mfma_f64_16x16x4_f64: K is the number of observables (10 here, at most 64), so a pair costs `cols` FMAs
// and then degree + 1 dependent vector operations of epilogue (scale, power, masked add) that no MFMA takes
// over, and K = 10 would be padded to 12.  After a tile every thread adds its live pairs (not on the diagonal
// of a symmetric matrix, by member position) to its running sum; at the end the workgroup is added by a
// butterfly and the waves in order, and one partial per workgroup goes to the workspace.  mm_final_kernel,
// one workgroup per segment, adds the partials of the live tiles in a fixed order.
#include <math.h>

#include "common.h"
#include "segment.h"

namespace {

constexpr int DS_MAX_ROWS = ES_DIST_MAX_ROWS;
constexpr int DS_MAX_SEG = ES_DIST_MAX_SEG;
constexpr size_t DS_ALIGN = 16;

// ------------------------------------------------------------------------------------------ moments
constexpr int MO_COLS = ES_MOMENTS_MAX_COLS;             // 32
constexpr int MO_PAIRS = MO_COLS * (MO_COLS + 1) / 2;    // 528 pairs i <= j
constexpr int MO_CH = ES_MOMENTS_CHUNKS;
constexpr int MO_THREADS = 256;
constexpr int MO_STAGE = 64;                             // members centred into LDS at a time
constexpr int MO_PITCH = MO_COLS + 1;
constexpr int MO_PER = (MO_PAIRS + MO_THREADS - 1) / MO_THREADS;   // pairs of a thread
static_assert(MO_COLS == 32 && MO_THREADS == 8 * MO_COLS, "thread = (row lane, column)");

struct MoArgs {
  const void* x; int f64; int64_t ld; int rows, cols;
  const int32_t* idx; const int32_t* seg;
  double* pmean;                                         // [n_seg][MO_CH][MO_COLS]
  double* pcov;                                          // [n_seg][MO_CH][MO_PAIRS]
  int32_t* count; double* mean; double* cov;
};

__device__ __forceinline__ double mo_load(const MoArgs& g, int64_t off) {
  return g.f64 ? ((const double*)g.x)[off] : (double)((const float*)g.x)[off];
}
// members of a run
__device__ __forceinline__ int mo_run(int n) {
  const int L = (n + MO_CH - 1) / MO_CH;
  return L < MO_STAGE ? MO_STAGE : L;
}
// the mean of column c from the runs' partials, the runs in order
__device__ __forceinline__ double mo_mean(const MoArgs& g, int s, int c, int n) {
  double t = 0.0;
#pragma unroll
  for (int k = 0; k < MO_CH; ++k) t += g.pmean[((int64_t)s * MO_CH + k) * MO_COLS + c];
  return t / (double)n;
}
// pair number q of the upper triangle, row by row
__device__ __forceinline__ void mo_pair(int q, int cols, int& i, int& j) {
  i = 0;
  while (q >= cols - i) {
    q -= cols - i;
    ++i;
  }
  j = i + q;
}

__global__ void __launch_bounds__(MO_THREADS) mo_mean_kernel(MoArgs g) {
  __shared__ double red[8][MO_COLS];
  const int t = threadIdx.x, c = t & 31, rl = t >> 5, k = blockIdx.x, s = blockIdx.y;
  const SegSpan sg = seg_span(g.seg, s, g.rows);
  const int L = mo_run(sg.n);
  const int64_t a = (int64_t)k * L;
  const int lo = a < sg.n ? (int)a : sg.n, hi = a + L < sg.n ? (int)(a + L) : sg.n;
  double acc = 0.0;
  if (c < g.cols)
    for (int p = lo + rl; p < hi; p += 8) acc += mo_load(g, (int64_t)seg_row(g.idx, sg.b + p, g.rows) * g.ld + c);
  red[rl][c] = acc;
  __syncthreads();
  if (t < MO_COLS) {
    double v = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) v += red[r][t];
    g.pmean[((int64_t)s * MO_CH + k) * MO_COLS + t] = v;
  }
}

__global__ void __launch_bounds__(MO_THREADS) mo_cov_kernel(MoArgs g) {
  __shared__ double mu[MO_COLS];
  __shared__ double d[MO_STAGE * MO_PITCH];
  const int t = threadIdx.x, k = blockIdx.x, s = blockIdx.y, cols = g.cols;
  const SegSpan sg = seg_span(g.seg, s, g.rows);
  const int L = mo_run(sg.n);
  const int64_t a = (int64_t)k * L;
  const int lo = a < sg.n ? (int)a : sg.n, hi = a + L < sg.n ? (int)(a + L) : sg.n;
  const int npairs = cols * (cols + 1) / 2;
  if (t < MO_COLS) mu[t] = (t < cols && sg.n > 0) ? mo_mean(g, s, t, sg.n) : 0.0;
  int pi[MO_PER], pj[MO_PER];
  double acc[MO_PER];
#pragma unroll
  for (int u = 0; u < MO_PER; ++u) {
    acc[u] = 0.0;
    pi[u] = pj[u] = 0;
    if (t + u * MO_THREADS < npairs) mo_pair(t + u * MO_THREADS, cols, pi[u], pj[u]);
  }
  for (int p0 = lo; p0 < hi; p0 += MO_STAGE) {         // block-uniform
    __syncthreads();                                    // mu is in place; the last stage's reads are done
#pragma unroll
    for (int m = 0; m < MO_STAGE * MO_COLS / MO_THREADS; ++m) {
      const int e = t + m * MO_THREADS, r = e >> 5, c = e & 31;
      double v = 0.0;
      if (c < cols && p0 + r < hi)
        v = mo_load(g, (int64_t)seg_row(g.idx, sg.b + p0 + r, g.rows) * g.ld + c) - mu[c];
      d[r * MO_PITCH + c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < MO_PER; ++u) {
      double v = acc[u];
      for (int r = 0; r < MO_STAGE; ++r) v = fma(d[r * MO_PITCH + pi[u]], d[r * MO_PITCH + pj[u]], v);
      acc[u] = v;
    }
  }
#pragma unroll
  for (int u = 0; u < MO_PER; ++u)
    if (t + u * MO_THREADS < npairs) g.pcov[((int64_t)s * MO_CH + k) * MO_PAIRS + t + u * MO_THREADS] = acc[u];
}

__global__ void __launch_bounds__(MO_THREADS) mo_final_kernel(MoArgs g) {
  const int t = threadIdx.x, s = blockIdx.x, cols = g.cols;
  const SegSpan sg = seg_span(g.seg, s, g.rows);
  const int n = sg.n, npairs = cols * (cols + 1) / 2;
  if (t == 0) g.count[s] = n;
  if (t < cols) g.mean[(int64_t)s * cols + t] = n > 0 ? mo_mean(g, s, t, n) : (double)NAN;
  for (int q = t; q < npairs; q += MO_THREADS) {
    int i, j;
    mo_pair(q, cols, i, j);
    double v = (double)NAN;
    if (n >= 2) {
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < MO_CH; ++k) sum += g.pcov[((int64_t)s * MO_CH + k) * MO_PAIRS + q];
      v = sum / ((double)n - 1.0);
    }
    double* c = g.cov + (int64_t)s * cols * cols;
    c[i * cols + j] = v;
    c[j * cols + i] = v;
  }
}

// ------------------------------------------------------------------------------------------ Frechet
constexpr int FR_N = ES_MOMENTS_MAX_COLS;
constexpr int FR_P = FR_N + 1;                           // LDS pitch of a matrix
constexpr int FR_MAX_SWEEPS = 30;
constexpr double FR_ROT_TOL = 1.3877787807814457e-17;    // 2^-56

// Cyclic Jacobi on the symmetric n x n matrix A (LDS); with VEC, V starts as the identity and ends with the
// eigenvectors in its columns.  One wave; lane r owns row r of A and V; every lane computes the same rotation
// from broadcast reads, so every branch is wave-uniform.  The eigenvalues end on A's diagonal.
template <bool VEC>
__device__ void fr_jacobi(double* A, double* V, int n, int r) {
  if (VEC && r < n)
    for (int c = 0; c < n; ++c) V[r * FR_P + c] = r == c ? 1.0 : 0.0;
  __syncthreads();
  for (int sweep = 0; sweep < FR_MAX_SWEEPS; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * FR_P + q], app = A[p * FR_P + p], aqq = A[q * FR_P + q];
        if (apq == 0.0 || fabs(apq) <= FR_ROT_TOL * sqrt(fabs(app) * fabs(aqq))) continue;
        rotated = true;
        const double theta = (aqq - app) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
        __syncthreads();                                 // every lane has read the three entries
        if (r < n) {
          const double akp = A[r * FR_P + p], akq = A[r * FR_P + q];
          A[r * FR_P + p] = c * akp - sn * akq;
          A[r * FR_P + q] = sn * akp + c * akq;
          if (VEC) {
            const double vp = V[r * FR_P + p], vq = V[r * FR_P + q];
            V[r * FR_P + p] = c * vp - sn * vq;
            V[r * FR_P + q] = sn * vp + c * vq;
          }
        }
        __syncthreads();
        if (r < n) {
          const double apk = A[p * FR_P + r], aqk = A[q * FR_P + r];
          A[p * FR_P + r] = c * apk - sn * aqk;
          A[q * FR_P + r] = sn * apk + c * aqk;
        }
        __syncthreads();
        if (r == 0) {
          A[p * FR_P + q] = 0.0;
          A[q * FR_P + p] = 0.0;
        }
        __syncthreads();
      }
    if (!rotated) break;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(64) fr_kernel(const double* __restrict__ mean_a, const double* __restrict__ cov_a,
                                                const double* __restrict__ mean_b, const double* __restrict__ cov_b,
                                                int n, double* __restrict__ out) {
  __shared__ double A[FR_N * FR_P];                      // A, then its eigenvalues on the diagonal
  __shared__ double B[FR_N * FR_P];
  __shared__ double V[FR_N * FR_P];
  __shared__ double H[FR_N * FR_P];                      // A^1/2
  __shared__ double T[FR_N * FR_P];                      // B A^1/2, then A^1/2 B A^1/2
  __shared__ double root[FR_N];
  __shared__ double dm[FR_N];
  const int r = threadIdx.x, i = blockIdx.x;
  const double* ca = cov_a + (int64_t)i * n * n;
  const double* cb = cov_b + (int64_t)i * n * n;
  bool bad = false;
  if (r < n) {
    const double ma = mean_a[(int64_t)i * n + r], mb = mean_b[(int64_t)i * n + r];
    dm[r] = ma - mb;
    bad = bad || ma != ma || mb != mb;
    for (int c = 0; c < n; ++c) {                        // the upper triangle, mirrored
      const double a = r <= c ? ca[r * n + c] : ca[c * n + r];
      const double b = r <= c ? cb[r * n + c] : cb[c * n + r];
      A[r * FR_P + c] = a;
      B[r * FR_P + c] = b;
      bad = bad || a != a || b != b;
    }
  }
  double* o = out + (int64_t)i * 4;
  if (__ballot(bad) != 0ull) {                           // wave-uniform
    if (r < 4) o[r] = (double)NAN;
    return;
  }
  __syncthreads();
  double dmu2 = 0.0, trs = 0.0;                          // the same in every lane: column order
  for (int c = 0; c < n; ++c) dmu2 = fma(dm[c], dm[c], dmu2);
  for (int c = 0; c < n; ++c) trs += A[c * FR_P + c];
  for (int c = 0; c < n; ++c) trs += B[c * FR_P + c];

  fr_jacobi<true>(A, V, n, r);
  if (r < n) {
    const double l = A[r * FR_P + r];
    root[r] = l > 0.0 ? sqrt(l) : 0.0;
  }
  __syncthreads();
  if (r < n)                                             // H = V diag(root) V^T
    for (int c = 0; c < n; ++c) {
      double v = 0.0;
      for (int k = 0; k < n; ++k) v = fma(V[r * FR_P + k] * root[k], V[c * FR_P + k], v);
      H[r * FR_P + c] = v;
    }
  __syncthreads();
  if (r < n)                                             // T = B H
    for (int c = 0; c < n; ++c) {
      double v = 0.0;
      for (int k = 0; k < n; ++k) v = fma(B[r * FR_P + k], H[k * FR_P + c], v);
      T[r * FR_P + c] = v;
    }
  __syncthreads();
  if (r < n)                                             // A = H T (A's own content is no longer needed)
    for (int c = 0; c < n; ++c) {
      double v = 0.0;
      for (int k = 0; k < n; ++k) v = fma(H[r * FR_P + k], T[k * FR_P + c], v);
      A[r * FR_P + c] = v;
    }
  __syncthreads();
  if (r < n)                                             // symmetric to the bit: T = (A + A^T) / 2
    for (int c = 0; c < n; ++c) T[r * FR_P + c] = 0.5 * (A[r * FR_P + c] + A[c * FR_P + r]);
  __syncthreads();
  fr_jacobi<false>(T, nullptr, n, r);
  double trr = 0.0;
  for (int c = 0; c < n; ++c) {
    const double m = T[c * FR_P + c];
    trr += m > 0.0 ? sqrt(m) : 0.0;
  }
  if (r == 0) {
    o[0] = (dmu2 + trs) - 2.0 * trr;
    o[1] = dmu2;
    o[2] = trs;
    o[3] = trr;
  }
}

// ------------------------------------------------------------------------------------------ polynomial-kernel sums
constexpr int MM_TILE = 128;                // rows of either side in a workgroup's tile
constexpr int MM_THREADS = 256;             // 16 x 16 threads of 8 x 8 pairs
constexpr int MM_KC = 16;                   // columns of a staged chunk
constexpr int MM_LD = MM_TILE + 4;          // floats of a staged column: rows stay 16-byte aligned
constexpr int MM_SIDE = MM_KC * MM_LD;
constexpr int MM_MAX_SPLIT = 16;            // runs of B tiles per (matrix, A tile)
constexpr int MM_TARGET_WG = 512;           // workgroups per matrix the split aims at

struct MmSide {
  const float* x; int64_t ld; int rows; const int32_t* idx; const int32_t* seg; int cap;
};
struct MmArgs {
  MmSide r, f;
  int cols, degree, tiles, split, per;      // tiles: A tiles of the grid; per: B tiles of one run
  double gamma, coef0;
  double* part;                             // [3 * n_seg][tiles][split]
  double* sums; int32_t* counts;
};

__device__ __forceinline__ SegSpan mm_seg(const MmSide& sd, int s) { return seg_span(sd.seg, s, sd.rows, sd.cap); }
// element offset of member i of the segment (n >= 1); a member past the end reads the last one's row
__device__ __forceinline__ int64_t mm_off(const MmSide& sd, SegSpan sg, int i) {
  return (int64_t)seg_row(sd.idx, sg.b + (i < sg.n ? i : sg.n - 1), sd.rows) * sd.ld;
}

__global__ void __launch_bounds__(MM_THREADS, 2) mm_pair_kernel(MmArgs g) {
  __shared__ __attribute__((aligned(16))) float st[2 * MM_SIDE];   // [side][column][row]
  __shared__ int64_t offA[MM_TILE];
  __shared__ int64_t offB[MM_TILE];
  __shared__ double red[MM_THREADS / 64];

  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int s = blockIdx.z / 3, mat = blockIdx.z - 3 * s, run = blockIdx.y, p0 = blockIdx.x * MM_TILE;
  const MmSide& A = mat == 1 ? g.f : g.r;
  const MmSide& B = mat == 0 ? g.r : g.f;
  const bool sym = mat < 2;
  const SegSpan sa = mm_seg(A, s), sb = mm_seg(B, s);
  if (p0 >= sa.n) return;                   // block-uniform: a tile past the live length writes no partial

  if (t < MM_TILE) offA[t] = mm_off(A, sa, p0 + t);
  const int nq = (sb.n + MM_TILE - 1) / MM_TILE;
  const int t_lo = run * g.per, t_hi = t_lo + g.per < nq ? t_lo + g.per : nq;
  const int sc = t & 15, sr = t >> 4;       // staging: column of the chunk, first row (then every 16th)
  const int nch = (g.cols + MM_KC - 1) / MM_KC;
  const double gamma = g.gamma, coef0 = g.coef0;
  const int degree = g.degree;
  double total = 0.0;

  for (int qt = t_lo; qt < t_hi; ++qt) {
    const int q0 = qt * MM_TILE;
    __syncthreads();                        // the last tile's reads of offB are done
    if (t < MM_TILE) offB[t] = mm_off(B, sb, q0 + t);

    double acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = 0.0;

    for (int ch = 0; ch < nch; ++ch) {
      __syncthreads();                      // offA / offB are in place; the last chunk's reads are done
      {
        const int cn = ch * MM_KC + sc;
        const bool ok = cn < g.cols;
        const int c = ok ? cn : g.cols - 1;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const float va = A.x[offA[sr + 16 * m] + c], vb = B.x[offB[sr + 16 * m] + c];
          st[sc * MM_LD + sr + 16 * m] = ok ? va : 0.f;
          st[MM_SIDE + sc * MM_LD + sr + 16 * m] = ok ? vb : 0.f;
        }
      }
      __syncthreads();
#pragma unroll 2
      for (int cc = 0; cc < MM_KC; ++cc) {
        const f32x4 a0 = *(const f32x4*)(st + cc * MM_LD + ty * 4);
        const f32x4 a1 = *(const f32x4*)(st + cc * MM_LD + 64 + ty * 4);
        const f32x4 b0 = *(const f32x4*)(st + MM_SIDE + cc * MM_LD + tx * 4);
        const f32x4 b1 = *(const f32x4*)(st + MM_SIDE + cc * MM_LD + 64 + tx * 4);
        const double a[8] = {(double)a0[0], (double)a0[1], (double)a0[2], (double)a0[3],
                             (double)a1[0], (double)a1[1], (double)a1[2], (double)a1[3]};
        const double b[8] = {(double)b0[0], (double)b0[1], (double)b0[2], (double)b0[3],
                             (double)b1[0], (double)b1[1], (double)b1[2], (double)b1[3]};
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
      }
    }

    // ---- the tile's 8 x 8 dot products of this thread are complete: kernel values, live pairs only
    double tile = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int p = p0 + ty * 4 + (i & 3) + 64 * (i >> 2);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int q = q0 + tx * 4 + (j & 3) + 64 * (j >> 2);
        const double v = fma(gamma, acc[i][j], coef0);
        double kv = v;
        for (int e = 1; e < degree; ++e) kv *= v;
        const bool live = p < sa.n && q < sb.n && !(sym && p == q);
        tile += live ? kv : 0.0;
      }
    }
    total += tile;
  }

  total = wave_sum_d(total);
  if ((t & 63) == 0) red[t >> 6] = total;
  __syncthreads();
  if (t == 0) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < MM_THREADS / 64; ++w) v += red[w];
    g.part[((int64_t)blockIdx.z * g.tiles + blockIdx.x) * g.split + run] = v;
  }
}

// per segment: the partials of the live A tiles of each matrix, thread t every 256th in order, then the block
__global__ void __launch_bounds__(256) mm_final_kernel(MmArgs g) {
  __shared__ double red[256 / 64];
  const int s = blockIdx.x, t = threadIdx.x;
  const SegSpan sr = mm_seg(g.r, s), sf = mm_seg(g.f, s);
  for (int mat = 0; mat < 3; ++mat) {
    const int na = mat == 1 ? sf.n : sr.n;
    const int live = ((na + MM_TILE - 1) / MM_TILE) * g.split;
    const double* in = g.part + ((int64_t)(3 * s + mat) * g.tiles) * g.split;
    double v = 0.0;
    for (int e = t; e < live; e += 256) v += in[e];
    v = block_sum_d(v, red);
    if (t == 0) g.sums[(int64_t)s * 4 + mat] = v;
  }
  if (t == 0) {
    g.sums[(int64_t)s * 4 + 3] = 0.0;
    g.counts[2 * s] = sr.n;
    g.counts[2 * s + 1] = sf.n;
  }
}

// ------------------------------------------------------------------------------------------ host side
int mm_tiles(int cap) { return (cap + MM_TILE - 1) / MM_TILE; }
// runs of B tiles: enough workgroups per matrix to fill the chip, at most one run per tile
int mm_split(int tiles) {
  int sp = MM_TARGET_WG / tiles;
  sp = sp < MM_MAX_SPLIT ? sp : MM_MAX_SPLIT;
  sp = sp < tiles ? sp : tiles;
  return sp > 1 ? sp : 1;
}
bool ds_side_ok(int rows, int cap, int n_seg) {
  return rows >= 1 && rows <= DS_MAX_ROWS && cap >= 1 && cap <= DS_MAX_ROWS && n_seg >= 1 && n_seg <= DS_MAX_SEG;
}

}  // namespace

extern "C" size_t es_segment_moments_workspace(int n_seg, int cols) {
  if (n_seg < 1 || n_seg > DS_MAX_SEG || cols < 1 || cols > MO_COLS) return 0;
  Carver c(nullptr, DS_ALIGN);
  c.take<double>((size_t)n_seg * MO_CH * MO_COLS);
  c.take<double>((size_t)n_seg * MO_CH * MO_PAIRS);
  return c.bytes();
}

extern "C" size_t es_mmd_poly_workspace(int n_seg, int r_cap, int f_cap) {
  if (!ds_side_ok(1, r_cap, n_seg) || !ds_side_ok(1, f_cap, n_seg)) return 0;
  const int tiles = mm_tiles(r_cap > f_cap ? r_cap : f_cap);
  Carver c(nullptr, DS_ALIGN);
  c.take<double>((size_t)3 * n_seg * tiles * mm_split(tiles));
  return c.bytes();
}

extern "C" int es_segment_moments(const void* x, int x_f64, int64_t ld, int rows, int cols, const int32_t* idx,
                                  const int32_t* seg, int n_seg, int32_t* count, double* mean, double* cov,
                                  void* work, size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(x && seg && count && mean && cov, "segment_moments: null argument");
  ES_CHECK_ARG(cols >= 1 && cols <= MO_COLS && ld >= cols, "segment_moments: cols=%d ld=%lld outside 1 <= cols <= %d, "
               "cols <= ld", cols, (long long)ld, MO_COLS);
  ES_CHECK_ARG(rows >= 1 && rows <= DS_MAX_ROWS && n_seg >= 1 && n_seg <= DS_MAX_SEG,
               "segment_moments: rows=%d n_seg=%d outside 1 <= rows <= %d, 1 <= n_seg <= %d", rows, n_seg, DS_MAX_ROWS,
               DS_MAX_SEG);
  const size_t need = es_segment_moments_workspace(n_seg, cols);
  ES_CHECK_ARG(work && work_bytes >= need, "segment_moments: workspace of %zu bytes, %zu needed", work_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  Carver c(work, DS_ALIGN);
  MoArgs g = {};
  g.x = x; g.f64 = x_f64 != 0; g.ld = ld; g.rows = rows; g.cols = cols; g.idx = idx; g.seg = seg;
  g.pmean = c.take<double>((size_t)n_seg * MO_CH * MO_COLS);
  g.pcov = c.take<double>((size_t)n_seg * MO_CH * MO_PAIRS);
  g.count = count; g.mean = mean; g.cov = cov;
  hipLaunchKernelGGL(mo_mean_kernel, dim3(MO_CH, n_seg), dim3(MO_THREADS), 0, st, g);
  hipLaunchKernelGGL(mo_cov_kernel, dim3(MO_CH, n_seg), dim3(MO_THREADS), 0, st, g);
  hipLaunchKernelGGL(mo_final_kernel, dim3(n_seg), dim3(MO_THREADS), 0, st, g);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_frechet(const double* mean_a, const double* cov_a, const double* mean_b, const double* cov_b, int n,
                          int cols, double* out, es_stream_t stream) {
  ES_CHECK_ARG(mean_a && cov_a && mean_b && cov_b && out, "frechet: null argument");
  ES_CHECK_ARG(n >= 1 && n <= DS_MAX_SEG && cols >= 1 && cols <= FR_N,
               "frechet: n=%d cols=%d outside 1 <= n <= %d, 1 <= cols <= %d", n, cols, DS_MAX_SEG, FR_N);
  hipLaunchKernelGGL(fr_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, mean_a, cov_a, mean_b, cov_b, cols, out);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_mmd_poly(const float* real, int64_t r_ld, int r_rows, const int32_t* r_idx, const int32_t* r_seg,
                           int r_cap, const float* fake, int64_t f_ld, int f_rows, const int32_t* f_idx,
                           const int32_t* f_seg, int f_cap, int cols, int n_seg, int degree, double gamma,
                           double coef0, double* sums, int32_t* counts, void* work, size_t work_bytes,
                           es_stream_t stream) {
  ES_CHECK_ARG(real && fake && r_seg && f_seg && sums && counts, "mmd_poly: null argument");
  ES_CHECK_ARG(cols >= 1 && cols <= ES_MMD_MAX_COLS && r_ld >= cols && f_ld >= cols,
               "mmd_poly: cols=%d r_ld=%lld f_ld=%lld outside 1 <= cols <= %d, cols <= ld", cols, (long long)r_ld,
               (long long)f_ld, ES_MMD_MAX_COLS);
  ES_CHECK_ARG(ds_side_ok(r_rows, r_cap, n_seg) && ds_side_ok(f_rows, f_cap, n_seg),
               "mmd_poly: r_rows=%d r_cap=%d f_rows=%d f_cap=%d n_seg=%d outside 1 <= rows, cap <= %d, "
               "1 <= n_seg <= %d", r_rows, r_cap, f_rows, f_cap, n_seg, DS_MAX_ROWS, DS_MAX_SEG);
  ES_CHECK_ARG(degree >= 1 && degree <= ES_MMD_MAX_DEGREE, "mmd_poly: degree = %d outside 1 .. %d", degree,
               ES_MMD_MAX_DEGREE);
  const size_t need = es_mmd_poly_workspace(n_seg, r_cap, f_cap);
  ES_CHECK_ARG(work && work_bytes >= need, "mmd_poly: workspace of %zu bytes, %zu needed", work_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  MmArgs g = {};
  g.r = {real, r_ld, r_rows, r_idx, r_seg, r_cap};
  g.f = {fake, f_ld, f_rows, f_idx, f_seg, f_cap};
  g.cols = cols;
  g.degree = degree;
  g.tiles = mm_tiles(r_cap > f_cap ? r_cap : f_cap);
  g.split = mm_split(g.tiles);
  g.per = (g.tiles + g.split - 1) / g.split;
  g.gamma = gamma;
  g.coef0 = coef0;
  g.part = (double*)work;
  g.sums = sums;
  g.counts = counts;
  hipLaunchKernelGGL(mm_pair_kernel, dim3(g.tiles, g.split, 3 * n_seg), dim3(MM_THREADS), 0, st, g);
  hipLaunchKernelGGL(mm_final_kernel, dim3(n_seg), dim3(256), 0, st, g);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
