// Conditioning embeddings on the device: PCA and exact, matrix-free t-SNE.
// include/expertsim_hip.h has the definitions; this file has the kernels.
//
// es_pca_project: pca_mean_kernel / pca_cov_kernel (thread (chunk k, column or column pair) walks its rows
// sequentially, es_group_diversity's order; the ES_PREP_CHUNKS partials are added in chunk order through LDS),
// pca_jacobi_kernel (ONE wave: the cols x cols matrix sits in LDS, lane r owns row r of the matrix and of the
// eigenvector matrix; cyclic Jacobi, every lane computes the same rotation from broadcast LDS reads, then the
// lanes update the two columns, then the two rows; sort, sign and the outputs at the end) and pca_scores_kernel.
//
// es_tsne_affinities: tsne_affinity_kernel, one workgroup per row i.  Thread t takes the columns j = t,
// t + 256, ..; d_ij is recomputed from x at every search step (x lives in L2; the pass runs once).  The two row
// sums are fp64, per thread in j order, then a butterfly over the wave and the waves in order.
//
// es_tsne_gradient / es_tsne_run: per iteration
//   tsne_pair_kernel   the hot path.  Grid (row tiles) x (j splits).  A thread owns R rows (x_i, y_i and the
//                      row's scalars in registers); the workgroup stages four tiles of ES_TSNE_TILE columns j in LDS
//                      (x_j padded to PITCH floats, (y_j0, y_j1, b_j, l_j) as one float4, dmin_j) and every lane
//                      reads the same j: a broadcast, no bank conflict by the bank rule.  Pair math fp32 (direct
//                      differences, two v_exp_f32, one v_rcp_f32); fp32 sums along the tile, tile sums added in
//                      fp64 in tile order; one partial per (split, row) goes to the workspace.  R rows per lane
//                      and an unrolled j loop give independent exp / rcp chains.
//   tsne_zsum_kernel   ONE workgroup: every row's splits in split order, the rows in a fixed order: Z (and the
//                      KL's two sums on a check iteration).
//   tsne_update_kernel a thread per row: the splits in split order, the gradient, sklearn's update.
//   tsne_log_kernel    (check iterations) ONE workgroup: the gradient norm, the log row.
// No float atomics anywhere; no host synchronisation.
#include <float.h>
#include <math.h>

#include "common.h"
#include "segment.h"

namespace {

constexpr int EMB_THREADS = 256;
constexpr int EMB_MAX_ROWS = 1 << 20;
constexpr int TSNE_MAX_ROWS = 1 << 17;
constexpr int TSNE_BLOCK = 128;                // threads of a pair workgroup == columns of a stage
constexpr int TSNE_STAGE = 4 * ES_TSNE_TILE;   // columns j staged in LDS at a time: four fp32 chains
constexpr int TSNE_PART = 8;                   // doubles per (split, row): A0 A1 R0 R1 Zr Kp Ps -
constexpr int TSNE_RED = 1024;                 // threads of the single-workgroup reductions
constexpr int PCA_MAX_SWEEPS = 30;
constexpr double PCA_ROT_TOL = 1.3877787807814457e-17;   // 2^-56
constexpr double TSNE_LOG2E = 1.4426950408889634;
static_assert(TSNE_BLOCK == TSNE_STAGE, "one staged column per thread");

// ------------------------------------------------------------------------------------------ PCA
__device__ __forceinline__ int emb_chunk_len(int n) {
  return n <= ES_PREP_SPLIT_MIN ? n : (n + ES_PREP_CHUNKS - 1) / ES_PREP_CHUNKS;
}

template <typename T>
__global__ void __launch_bounds__(EMB_THREADS) pca_mean_kernel(const T* __restrict__ x, int64_t ld, int rows,
                                                               int cols, double* __restrict__ mean) {
#pragma clang fp contract(off)
  __shared__ double part[ES_PREP_CHUNKS][ES_DIAG_MAX_COLS];
  const int tid = threadIdx.x;
  const int L = emb_chunk_len(rows);
  for (int w = tid; w < ES_PREP_CHUNKS * cols; w += EMB_THREADS) {
    const int k = w / cols, c = w - k * cols;
    const int64_t a = (int64_t)k * L, z = a + L;
    const int lo = a < rows ? (int)a : rows, hi = z < rows ? (int)z : rows;
    double acc = 0.0;
    for (int p = lo; p < hi; ++p) acc += (double)x[(int64_t)p * ld + c];
    part[k][c] = acc;
  }
  __syncthreads();
  if (tid < cols) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < ES_PREP_CHUNKS; ++k) t += part[k][tid];
    mean[tid] = t / (double)rows;
  }
}

// cov[c1][c2] for 16 (c1, c2) pairs of the full cols x cols square per workgroup; c1 > c2 is left to its mirror
template <typename T>
__global__ void __launch_bounds__(EMB_THREADS) pca_cov_kernel(const T* __restrict__ x, int64_t ld, int rows,
                                                              int cols, const double* __restrict__ mean,
                                                              double* __restrict__ cov) {
#pragma clang fp contract(off)
  __shared__ double part[ES_PREP_CHUNKS][16];
  const int tid = threadIdx.x, k = tid >> 4, slot = tid & 15;
  const int pair = blockIdx.x * 16 + slot;
  const int c1 = pair / cols, c2 = pair - c1 * cols;
  const bool live = pair < cols * cols && c1 <= c2;
  double acc = 0.0;
  if (live) {
    const int L = emb_chunk_len(rows);
    const int64_t a = (int64_t)k * L, z = a + L;
    const int lo = a < rows ? (int)a : rows, hi = z < rows ? (int)z : rows;
    const double m1 = mean[c1], m2 = mean[c2];
    for (int p = lo; p < hi; ++p) {
      const double d1 = (double)x[(int64_t)p * ld + c1] - m1;
      const double d2 = (double)x[(int64_t)p * ld + c2] - m2;
      const double q = d1 * d2;
      acc += q;
    }
  }
  part[k][slot] = acc;
  __syncthreads();
  if (tid < 16 && live) {
    double t = 0.0;
#pragma unroll
    for (int kk = 0; kk < ES_PREP_CHUNKS; ++kk) t += part[kk][tid];
    const double v = t / ((double)rows - 1.0);
    cov[c1 * cols + c2] = v;
    cov[c2 * cols + c1] = v;
  }
}

// One wave.  A (LDS) starts as cov; V (global, lane r owns row r) as the identity.
__global__ void __launch_bounds__(64) pca_jacobi_kernel(const double* __restrict__ cov, int n, int k,
                                                        double* V, double* __restrict__ components,
                                                        double* __restrict__ ev, double* __restrict__ evr) {
#pragma clang fp contract(off)
  __shared__ double A[ES_DIAG_MAX_COLS * ES_DIAG_MAX_COLS];
  __shared__ double lam[ES_DIAG_MAX_COLS];
  const int r = threadIdx.x;
  if (r < n)
    for (int c = 0; c < n; ++c) {
      A[r * n + c] = cov[r * n + c];
      V[r * n + c] = r == c ? 1.0 : 0.0;
    }
  __syncthreads();
  double trace = 0.0;
  for (int c = 0; c < n; ++c) trace += A[c * n + c];
  for (int sweep = 0; sweep < PCA_MAX_SWEEPS; ++sweep) {
    bool rotated = false;                               // the same in every lane
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q], app = A[p * n + p], aqq = A[q * n + q];
        if (apq == 0.0 || fabs(apq) <= PCA_ROT_TOL * sqrt(fabs(app) * fabs(aqq))) continue;
        rotated = true;
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        __syncthreads();                                // every lane has read the three entries
        if (r < n) {
          const double akp = A[r * n + p], akq = A[r * n + q];
          A[r * n + p] = c * akp - s * akq;
          A[r * n + q] = s * akp + c * akq;
          const double vp = V[r * n + p], vq = V[r * n + q];
          V[r * n + p] = c * vp - s * vq;
          V[r * n + q] = s * vp + c * vq;
        }
        __syncthreads();
        if (r < n) {
          const double apk = A[p * n + r], aqk = A[q * n + r];
          A[p * n + r] = c * apk - s * aqk;
          A[q * n + r] = s * apk + c * aqk;
        }
        __syncthreads();
        if (r == 0) {
          A[p * n + q] = 0.0;
          A[q * n + p] = 0.0;
        }
        __syncthreads();
      }
    if (!rotated) break;
  }
  if (r < n) lam[r] = A[r * n + r];
  __syncthreads();                                      // also makes every lane's row of V visible to the wave
  if (r < n) {
    const double l = lam[r];
    int rank = 0;                                       // decreasing eigenvalue, the lower index first on a tie
    for (int m = 0; m < n; ++m) rank += (lam[m] > l || (lam[m] == l && m < r)) ? 1 : 0;
    if (rank < k) {
      double big = -1.0, sign = 1.0;                    // the entry of largest magnitude positive, first index wins
      for (int c = 0; c < n; ++c) {
        const double v = V[c * n + r];
        if (fabs(v) > big) {
          big = fabs(v);
          sign = v < 0.0 ? -1.0 : 1.0;
        }
      }
      for (int c = 0; c < n; ++c) components[rank * n + c] = sign * V[c * n + r];
      ev[rank] = l;
      evr[rank] = trace > 0.0 ? l / trace : 0.0;
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(EMB_THREADS) pca_scores_kernel(const T* __restrict__ x, int64_t ld, int rows,
                                                                 int cols, int k, const double* __restrict__ mean,
                                                                 const double* __restrict__ components,
                                                                 double* __restrict__ scores) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * EMB_THREADS + threadIdx.x;
  if (i >= (int64_t)rows * k) return;
  const int row = (int)(i / k), m = (int)(i - (int64_t)row * k);
  double acc = 0.0;
  for (int c = 0; c < cols; ++c) {
    const double d = (double)x[(int64_t)row * ld + c] - mean[c];
    const double q = d * components[m * cols + c];
    acc += q;
  }
  scores[i] = acc;
}

// ------------------------------------------------------------------------------------------ t-SNE
// d_ij of the header: fp32, the product rounded, then added, columns in order from +0.0f
__device__ __forceinline__ float tsne_dist_global(const float* __restrict__ xi, const float* __restrict__ xj,
                                                  int cols) {
#pragma clang fp contract(off)
  float acc = 0.0f;
  for (int c = 0; c < cols; ++c) {
    const float t = xi[c] - xj[c];
    const float q = t * t;
    acc = acc + q;
  }
  return acc;
}

__global__ void __launch_bounds__(EMB_THREADS) tsne_affinity_kernel(const float* __restrict__ x, int64_t ld,
                                                                    int rows, int cols, double perplexity,
                                                                    double* __restrict__ beta_out,
                                                                    double* __restrict__ log_s,
                                                                    float* __restrict__ dmin_out,
                                                                    int32_t* __restrict__ steps) {
#pragma clang fp contract(off)
  __shared__ float s_xi[ES_DIAG_MAX_COLS];
  __shared__ float s_min[EMB_THREADS / 64];
  __shared__ double s_red[EMB_THREADS / 64];
  const int tid = threadIdx.x, i = blockIdx.x;
  if (tid < cols) s_xi[tid] = x[(int64_t)i * ld + tid];
  __syncthreads();
  float m = INFINITY;
  for (int j = tid; j < rows; j += EMB_THREADS)
    if (j != i) m = fminf(m, tsne_dist_global(s_xi, x + (int64_t)j * ld, cols));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
  if ((tid & 63) == 0) s_min[tid >> 6] = m;
  __syncthreads();
  m = fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3]));
  const double dm = (double)m, target = log(perplexity);
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, b_eval = 1.0, ls_eval = 0.0;
  int n_eval = 0;
  for (int it = 0; it < 100; ++it) {
    double S = 0.0, W = 0.0;
    for (int j = tid; j < rows; j += EMB_THREADS) {
      if (j == i) continue;
      const double dd = (double)tsne_dist_global(s_xi, x + (int64_t)j * ld, cols) - dm;
      const double e = exp(-beta * dd);
      const double q = dd * e;
      S += e;
      W += q;
    }
    S = block_sum_d(S, s_red);
    W = block_sum_d(W, s_red);
    const double lS = log(S);
    const double H = lS + beta * (W / S);
    const double diff = H - target;
    b_eval = beta;
    ls_eval = lS;
    n_eval = it + 1;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  if (tid == 0) {
    beta_out[i] = b_eval;
    log_s[i] = ls_eval;
    dmin_out[i] = m;
    steps[i] = n_eval;
  }
}

// the row scalars of the pair pass: b_i = fl32(beta_i log2 e), l_i = fl32(log_s_i log2 e + log2(2 rows))
__global__ void __launch_bounds__(EMB_THREADS) tsne_prep_kernel(const double* __restrict__ beta,
                                                                const double* __restrict__ log_s, int rows,
                                                                float* __restrict__ b2, float* __restrict__ l2) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * EMB_THREADS + threadIdx.x;
  if (r >= rows) return;
  const double b = beta[r] * TSNE_LOG2E;
  const double l = log_s[r] * TSNE_LOG2E;
  b2[r] = (float)b;
  l2[r] = (float)(l + log2(2.0 * (double)rows));
}

template <int C>
__device__ __forceinline__ float tsne_dist_reg(const float (&xi)[C], const float (&xj)[C]) {
#pragma clang fp contract(off)
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float t = xi[c] - xj[c];
    const float q = t * t;
    acc = acc + q;
  }
  return acc;
}

template <int C, int PITCH, int R, bool KL>
__global__ void __launch_bounds__(TSNE_BLOCK) tsne_pair_kernel(const float* __restrict__ x, int64_t ld, int rows,
                                                               int cols, const float* __restrict__ y,
                                                               const float* __restrict__ b2,
                                                               const float* __restrict__ l2,
                                                               const float* __restrict__ dmin, int split_len,
                                                               double* __restrict__ part) {
  constexpr int NA = KL ? 7 : 5;
  __shared__ __attribute__((aligned(16))) float s_x[TSNE_STAGE * PITCH];
  __shared__ float4 s_m[TSNE_STAGE];
  __shared__ float s_dm[TSNE_STAGE];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * (TSNE_BLOCK * R) + tid;
  const int split = blockIdx.y;
  const int64_t jb = (int64_t)split * split_len, je = jb + split_len;
  const int j_begin = jb < rows ? (int)jb : rows, j_end = je < rows ? (int)je : rows;
  int ri[R];
  float xi[R][C], yi0[R], yi1[R], bi[R], li[R], di[R];
  double D[R][NA];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ri[r] = row0 + r * TSNE_BLOCK;
    const int rc = ri[r] < rows ? ri[r] : rows - 1;
#pragma unroll
    for (int c = 0; c < C; ++c) xi[r][c] = c < cols ? x[(int64_t)rc * ld + c] : 0.0f;
    yi0[r] = y[2 * rc];
    yi1[r] = y[2 * rc + 1];
    bi[r] = b2[rc];
    li[r] = l2[rc];
    di[r] = dmin[rc];
#pragma unroll
    for (int a = 0; a < NA; ++a) D[r][a] = 0.0;
  }
  for (int j0 = j_begin; j0 < j_end; j0 += TSNE_STAGE) {
    const int jn = j_end - j0 < TSNE_STAGE ? j_end - j0 : TSNE_STAGE;
    __syncthreads();                                    // the previous tile has been consumed
    if (tid < jn) {
      const int j = j0 + tid;
#pragma nounroll
      for (int c = 0; c < PITCH; ++c) s_x[tid * PITCH + c] = c < cols ? x[(int64_t)j * ld + c] : 0.0f;
      s_m[tid] = make_float4(y[2 * j], y[2 * j + 1], b2[j], l2[j]);
      s_dm[tid] = dmin[j];
    }
    __syncthreads();
    for (int e0 = 0; e0 < jn; e0 += ES_TSNE_TILE) {
      const int e1n = jn - e0 < ES_TSNE_TILE ? jn - e0 : ES_TSNE_TILE;
      float f[R][NA];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int a = 0; a < NA; ++a) f[r][a] = 0.0f;
#pragma unroll 2
      for (int e = e0; e < e0 + e1n; ++e) {
        float xj[C];
#pragma unroll
        for (int c = 0; c < C; ++c) xj[c] = s_x[e * PITCH + c];
        const float4 mj = s_m[e];
        const float dmj = s_dm[e];
        const int j = j0 + e;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float d = tsne_dist_reg<C>(xi[r], xj);
          const float e1 = __builtin_amdgcn_exp2f(-bi[r] * (d - di[r]) - li[r]);
          const float e2 = __builtin_amdgcn_exp2f(-mj.z * (d - dmj) - mj.w);
          const float dy0 = yi0[r] - mj.x, dy1 = yi1[r] - mj.y;
          const float wr = __builtin_amdgcn_rcpf(1.0f + dy0 * dy0 + dy1 * dy1);
          const bool self = j == ri[r];
          const float p = self ? 0.0f : e1 + e2;
          const float w = self ? 0.0f : wr;
          const float pw = p * w, w2 = w * w;
          f[r][0] += pw * dy0;
          f[r][1] += pw * dy1;
          f[r][2] += w2 * dy0;
          f[r][3] += w2 * dy1;
          f[r][4] += w;
          if (KL) {
            f[r][5] += p * (logf(fmaxf(p, (float)DBL_EPSILON)) - logf(wr));
            f[r][6] += p;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int a = 0; a < NA; ++a) D[r][a] += (double)f[r][a];
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (ri[r] < rows) {
      double* out = part + ((int64_t)split * rows + ri[r]) * TSNE_PART;
#pragma unroll
      for (int a = 0; a < NA; ++a) out[a] = D[r][a];
    }
}

// scal[0] = Z, scal[1] = KL (kl != 0), scal[2] = sum p_ij (kl != 0)
__global__ void __launch_bounds__(TSNE_RED) tsne_zsum_kernel(const double* __restrict__ part, int rows, int nsplit,
                                                             int kl, double* __restrict__ scal) {
#pragma clang fp contract(off)
  __shared__ double sh[TSNE_RED / 64];
  double z = 0.0, kp = 0.0, ps = 0.0;
  for (int r = threadIdx.x; r < rows; r += TSNE_RED) {
    double zr = 0.0, k = 0.0, p = 0.0;
    for (int s = 0; s < nsplit; ++s) {
      const double* q = part + ((int64_t)s * rows + r) * TSNE_PART;
      zr += q[4];
      if (kl) {
        k += q[5];
        p += q[6];
      }
    }
    z += zr;
    kp += k;
    ps += p;
  }
  const double Z = block_sum_d(z, sh);
  double K = 0.0, P = 0.0;
  if (kl) {
    K = block_sum_d(kp, sh);
    P = block_sum_d(ps, sh);
  }
  if (threadIdx.x == 0) {
    scal[0] = Z;
    if (kl) {
      scal[1] = K + log(Z) * P;
      scal[2] = P;
    }
  }
}

__global__ void __launch_bounds__(EMB_THREADS) tsne_update_kernel(const double* __restrict__ part, int rows,
                                                                  int nsplit, const double* __restrict__ scal,
                                                                  double a, double mu, double lr, double min_gain,
                                                                  int do_update, float* __restrict__ y,
                                                                  double* __restrict__ upd,
                                                                  double* __restrict__ gains,
                                                                  double* __restrict__ g_out) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * EMB_THREADS + threadIdx.x;
  if (r >= rows) return;
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < nsplit; ++s) {
    const double* q = part + ((int64_t)s * rows + r) * TSNE_PART;
#pragma unroll
    for (int c = 0; c < 4; ++c) t[c] += q[c];
  }
  const double Z = scal[0];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double att = a * t[c], rep = t[2 + c] / Z;
    const double g = 4.0 * (att - rep);
    g_out[2 * r + c] = g;
    if (do_update) {
      const double u = upd[2 * r + c];
      double gn = gains[2 * r + c];
      const double ug = u * g;
      gn = ug < 0.0 ? gn + 0.2 : gn * 0.8;
      gn = gn < min_gain ? min_gain : gn;
      const double gg = g * gn;
      const double mu_u = mu * u, lr_g = lr * gg;
      const double un = mu_u - lr_g;
      gains[2 * r + c] = gn;
      upd[2 * r + c] = un;
      y[2 * r + c] = (float)((double)y[2 * r + c] + un);
    }
  }
}

// log_row[0] = KL (scal[1]), log_row[1] = |g|_2
__global__ void __launch_bounds__(TSNE_RED) tsne_log_kernel(const double* __restrict__ g, int rows,
                                                            const double* __restrict__ scal,
                                                            double* __restrict__ log_row) {
#pragma clang fp contract(off)
  __shared__ double sh[TSNE_RED / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < 2 * rows; i += TSNE_RED) {
    const double q = g[i] * g[i];
    acc += q;
  }
  const double t = block_sum_d(acc, sh);
  if (threadIdx.x == 0) {
    log_row[0] = scal[1];
    log_row[1] = sqrt(t);
  }
}

bool pca_ok(int rows, int cols, int64_t ld, int k) {
  return cols >= 1 && cols <= ES_DIAG_MAX_COLS && ld >= cols && rows >= 2 && rows <= EMB_MAX_ROWS && k >= 1 && k <= cols;
}
bool tsne_ok(int rows, int cols, int64_t ld) {
  return cols >= 1 && cols <= ES_DIAG_MAX_COLS && ld >= cols && rows >= 2 && rows <= TSNE_MAX_ROWS;
}
int tsne_nsplit(int rows) {
  const int n = (rows + 255) / 256;
  return n < 1 ? 1 : (n > ES_TSNE_MAX_SPLITS ? ES_TSNE_MAX_SPLITS : n);
}
int tsne_split_len(int rows) {
  const int ns = tsne_nsplit(rows), per = (rows + ns - 1) / ns;
  return ((per + TSNE_STAGE - 1) / TSNE_STAGE) * TSNE_STAGE;
}

struct TsneWork {
  double *part, *g, *scal;
  float *b2, *l2;
  size_t bytes;
};
TsneWork tsne_carve(void* work, int rows) {
  Carver c(work, 256);
  TsneWork w;
  w.part = c.take<double>((size_t)tsne_nsplit(rows) * rows * TSNE_PART);
  w.g = c.take<double>((size_t)rows * 2);
  w.scal = c.take<double>(3);             // Z, KL, sum p_ij
  w.b2 = c.take<float>((size_t)rows);
  w.l2 = c.take<float>((size_t)rows);
  w.bytes = c.bytes();
  return w;
}

template <bool KL>
void tsne_launch_pair(const float* x, int64_t ld, int rows, int cols, const float* y, const float* dmin,
                      const TsneWork& w, hipStream_t st) {
  const int ns = tsne_nsplit(rows), sl = tsne_split_len(rows);
  const dim3 block(TSNE_BLOCK);
#define ES_TSNE_PAIR(CC, PP, RR)                                                                                  \
  hipLaunchKernelGGL((tsne_pair_kernel<CC, PP, RR, KL>), dim3((rows + TSNE_BLOCK * RR - 1) / (TSNE_BLOCK * RR), ns), \
                     block, 0, st, x, ld, rows, cols, y, w.b2, w.l2, dmin, sl, w.part)
  if (cols == 9) ES_TSNE_PAIR(9, 12, 2);
  else if (cols <= 16) ES_TSNE_PAIR(16, 16, 2);
  else if (cols <= 32) ES_TSNE_PAIR(32, 32, 1);
  else ES_TSNE_PAIR(64, 64, 1);
#undef ES_TSNE_PAIR
}

}  // namespace

extern "C" size_t es_pca_project_workspace(int cols) {
  if (cols < 1 || cols > ES_DIAG_MAX_COLS) return 0;
  return 2 * (size_t)cols * cols * sizeof(double);
}

extern "C" int es_pca_project(const void* x, int x_f64, int64_t ld, int rows, int cols, int k, double* scores,
                              double* components, double* explained_variance, double* explained_variance_ratio,
                              double* mean, void* work, size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(x && scores && components && explained_variance && explained_variance_ratio && mean,
               "pca_project: null argument");
  ES_CHECK_ARG(x_f64 == 0 || x_f64 == 1, "pca_project: x_f64 = %d, not 0 or 1", x_f64);
  ES_CHECK_ARG(pca_ok(rows, cols, ld, k), "pca_project: rows=%d cols=%d ld=%lld k=%d outside the limits", rows, cols,
               (long long)ld, k);
  const size_t need = es_pca_project_workspace(cols);
  ES_CHECK_ARG(work && work_bytes >= need, "pca_project: workspace of %zu bytes, %zu needed", work_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  double* cov = (double*)work;
  double* V = cov + (size_t)cols * cols;
  const dim3 block(EMB_THREADS), gc((cols * cols + 15) / 16),
      gs((unsigned)(((int64_t)rows * k + EMB_THREADS - 1) / EMB_THREADS));
  if (x_f64) {
    hipLaunchKernelGGL(pca_mean_kernel<double>, dim3(1), block, 0, st, (const double*)x, ld, rows, cols, mean);
    hipLaunchKernelGGL(pca_cov_kernel<double>, gc, block, 0, st, (const double*)x, ld, rows, cols, mean, cov);
  } else {
    hipLaunchKernelGGL(pca_mean_kernel<float>, dim3(1), block, 0, st, (const float*)x, ld, rows, cols, mean);
    hipLaunchKernelGGL(pca_cov_kernel<float>, gc, block, 0, st, (const float*)x, ld, rows, cols, mean, cov);
  }
  hipLaunchKernelGGL(pca_jacobi_kernel, dim3(1), dim3(64), 0, st, cov, cols, k, V, components, explained_variance,
                     explained_variance_ratio);
  if (x_f64)
    hipLaunchKernelGGL(pca_scores_kernel<double>, gs, block, 0, st, (const double*)x, ld, rows, cols, k, mean,
                       components, scores);
  else
    hipLaunchKernelGGL(pca_scores_kernel<float>, gs, block, 0, st, (const float*)x, ld, rows, cols, k, mean,
                       components, scores);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_tsne_affinities(const float* x, int64_t ld, int rows, int cols, double perplexity, double* beta,
                                  double* log_s, float* dmin, int32_t* steps, es_stream_t stream) {
  ES_CHECK_ARG(x && beta && log_s && dmin && steps, "tsne_affinities: null argument");
  ES_CHECK_ARG(tsne_ok(rows, cols, ld), "tsne_affinities: rows=%d cols=%d ld=%lld outside the limits", rows, cols,
               (long long)ld);
  ES_CHECK_ARG(perplexity > 0.0 && perplexity < (double)rows, "tsne_affinities: perplexity=%g outside 0 < p < rows=%d",
               perplexity, rows);
  hipLaunchKernelGGL(tsne_affinity_kernel, dim3(rows), dim3(EMB_THREADS), 0, (hipStream_t)stream, x, ld, rows, cols,
                     perplexity, beta, log_s, dmin, steps);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" size_t es_tsne_workspace(int rows) {
  if (rows < 2 || rows > TSNE_MAX_ROWS) return 0;
  return tsne_carve(nullptr, rows).bytes;
}

extern "C" int es_tsne_gradient(const float* x, int64_t ld, int rows, int cols, const double* beta,
                                const double* log_s, const float* dmin, const float* y, double exaggeration,
                                double* g, double* z_kl, void* work, size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(x && beta && log_s && dmin && y && g && z_kl, "tsne_gradient: null argument");
  ES_CHECK_ARG(tsne_ok(rows, cols, ld), "tsne_gradient: rows=%d cols=%d ld=%lld outside the limits", rows, cols,
               (long long)ld);
  ES_CHECK_ARG(exaggeration > 0.0 && exaggeration <= DBL_MAX, "tsne_gradient: exaggeration=%g", exaggeration);
  const size_t need = es_tsne_workspace(rows);
  ES_CHECK_ARG(work && work_bytes >= need, "tsne_gradient: workspace of %zu bytes, %zu needed", work_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  const TsneWork w = tsne_carve(work, rows);
  const dim3 block(EMB_THREADS), gr((rows + EMB_THREADS - 1) / EMB_THREADS);
  hipLaunchKernelGGL(tsne_prep_kernel, gr, block, 0, st, beta, log_s, rows, w.b2, w.l2);
  tsne_launch_pair<true>(x, ld, rows, cols, y, dmin, w, st);
  hipLaunchKernelGGL(tsne_zsum_kernel, dim3(1), dim3(TSNE_RED), 0, st, w.part, rows, tsne_nsplit(rows), 1, w.scal);
  hipLaunchKernelGGL(tsne_update_kernel, gr, block, 0, st, w.part, rows, tsne_nsplit(rows), w.scal, exaggeration, 0.0,
                     0.0, 0.0, 0, (float*)nullptr, (double*)nullptr, (double*)nullptr, g);
  (void)hipMemcpyAsync(z_kl, w.scal, 2 * sizeof(double), hipMemcpyDeviceToDevice, st);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_tsne_run(const float* x, int64_t ld, int rows, int cols, const double* beta, const double* log_s,
                           const float* dmin, float* y, double* upd, double* gains, int n_iter, int iter0,
                           double exaggeration, int exaggeration_iters, double momentum0, double momentum1,
                           double learning_rate, double min_gain, int check_every, double* log, int log_rows,
                           void* work, size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(x && beta && log_s && dmin && y && upd && gains && log, "tsne_run: null argument");
  ES_CHECK_ARG(tsne_ok(rows, cols, ld), "tsne_run: rows=%d cols=%d ld=%lld outside the limits", rows, cols,
               (long long)ld);
  ES_CHECK_ARG(n_iter >= 0 && iter0 >= 0 && (int64_t)iter0 + n_iter <= INT32_MAX, "tsne_run: n_iter=%d iter0=%d", n_iter,
               iter0);
  ES_CHECK_ARG(exaggeration > 0.0 && exaggeration <= DBL_MAX && exaggeration_iters >= 0 &&
                   check_every >= 1 && learning_rate > 0.0 && learning_rate <= DBL_MAX &&
                   min_gain >= 0.0 && momentum0 >= 0.0 && momentum1 >= 0.0,
               "tsne_run: parameters outside their ranges");
  if (n_iter == 0) return ES_OK;
  const int last = iter0 + n_iter - 1;
  ES_CHECK_ARG(log_rows > last / check_every, "tsne_run: log of %d rows, %d needed", log_rows,
               last / check_every + 1);
  const size_t need = es_tsne_workspace(rows);
  ES_CHECK_ARG(work && work_bytes >= need, "tsne_run: workspace of %zu bytes, %zu needed", work_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  const TsneWork w = tsne_carve(work, rows);
  const int ns = tsne_nsplit(rows);
  const dim3 block(EMB_THREADS), gr((rows + EMB_THREADS - 1) / EMB_THREADS);
  hipLaunchKernelGGL(tsne_prep_kernel, gr, block, 0, st, beta, log_s, rows, w.b2, w.l2);
  for (int t = iter0; t <= last; ++t) {
    const bool early = t < exaggeration_iters;
    const bool check = (t + 1) % check_every == 0 || t == last;
    if (check) tsne_launch_pair<true>(x, ld, rows, cols, y, dmin, w, st);
    else tsne_launch_pair<false>(x, ld, rows, cols, y, dmin, w, st);
    hipLaunchKernelGGL(tsne_zsum_kernel, dim3(1), dim3(TSNE_RED), 0, st, w.part, rows, ns, check ? 1 : 0, w.scal);
    hipLaunchKernelGGL(tsne_update_kernel, gr, block, 0, st, w.part, rows, ns, w.scal, early ? exaggeration : 1.0,
                       early ? momentum0 : momentum1, learning_rate, min_gain, 1, y, upd, gains,
                       w.g);
    if (check)
      hipLaunchKernelGGL(tsne_log_kernel, dim3(1), dim3(TSNE_RED), 0, st, w.g, rows, w.scal,
                         log + 2 * (size_t)(t / check_every));
  }
  ES_CHECK_LAUNCH();
  return ES_OK;
}
