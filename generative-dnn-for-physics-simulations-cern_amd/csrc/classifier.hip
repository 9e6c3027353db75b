// Classifier two-sample test on the device: ridge-penalised logistic regression per segment by safeguarded Newton
// steps in fp64 (es_logit_fit) and the scores of a fitted model (es_logit_scores).  include/expertsim_hip.h defines
// both entries to the letter; this file is how they run.
//
// es_logit_fit.  The rows of a segment are numbered i < m (real, y = 1) then i < m + k (generated, y = 0) and cut
// into blocks of ES_LOGIT_BLOCK_ROWS.  Per pass two launches:
//   lg_pass_kernel, one workgroup per (block, segment): with the segment's point theta and pending step d it stages
//     64 rows at a time in LDS (z~ = (1, z), zero-padded to a multiple of 4 columns), takes t0 = <theta, z~> and
//     td = <d, z~> per row (one thread a row, columns ascending), the loss at the LG_STEPS trial points
//     theta + 2^-j d, and the gradient and Hessian sums AT theta + d: the Hessian as 4 x 4 register tiles of its
//     upper triangle, one thread a tile.  The partials go to the workspace; nothing is shared between workgroups.
//   lg_solve_kernel, one workgroup per segment: adds the blocks' partials in block order, adds the ridge terms, and
//     either accepts theta + d (F did not increase beyond its rounding), or moves to the best shorter trial point
//     and asks for a re-evaluation there (d = 0), then checks |g|_inf <= gtol, factorises H = L L^T in LDS and
//     stores the next step d = -H^-1 g.
// The hand-off is the stream order of the launches.  The host issues 1 + 2 (max_iter + 1) launches and never looks
// at the device; a segment that is done (state flag) makes its workgroups return at once.
// Order of every sum: rows of a 64-row stage in order, stages in order, blocks in order: a rerun is bit-equal.
#include "common.h"
#include "segment.h"

namespace {

constexpr int LG_THREADS = 256;
constexpr int LG_ROWS = ES_LOGIT_BLOCK_ROWS;     // rows of one block
constexpr int LG_STAGE = 64;                     // rows staged in LDS at a time
constexpr int LG_PMAX = ES_LOGIT_MAX_COLS + 1;   // parameters
constexpr int LG_PP = (LG_PMAX + 3) / 4 * 4;     // padded to the tiles: 84
constexpr int LG_LDZ = LG_PP + 1;                // LDS row stride of a staged row (odd: rows fall on other banks)
constexpr int LG_STEPS = 8;                      // trial step lengths 1, 1/2, .. 2^-7
// state of a segment: theta [LG_PP], d [LG_PP], then F, |g|_inf, iterations, status, done, re-evaluating
constexpr int LG_STATE = 2 * LG_PP + 8;
enum { LG_F = 2 * LG_PP, LG_G, LG_IT, LG_STATUS, LG_DONE, LG_REEVAL };

struct LgArgs {
  const void* r; int64_t r_ld; int r_rows; const int32_t* r_idx; const int32_t* r_seg; int r_cap;
  const void* f; int64_t f_ld; int f_rows; const int32_t* f_idx; const int32_t* f_seg; int f_cap;
  int f64, cols;
};

__host__ __device__ __forceinline__ int lg_tiles(int T) { return T * (T + 1) / 2; }
// doubles of one block's partial: the tiles, the gradient, the trial losses
__host__ __device__ __forceinline__ int lg_part(int cols) {
  const int T = (cols + 4) / 4;
  return lg_tiles(T) * 16 + 4 * T + LG_STEPS;
}
__device__ __forceinline__ void lg_tile_of(int t, int T, int& ti, int& tj) {   // tile t of the upper triangle
  ti = 0;
  while (t >= T - ti) { t -= T - ti; ++ti; }
  tj = ti + t;
}

// column c of member i (i < m: real) of the segment
__device__ __forceinline__ double lg_value(const LgArgs& a, SegSpan sr, SegSpan sf, int i, int c) {
  const bool real = i < sr.n;
  const int row = real ? seg_row(a.r_idx, sr.b + i, a.r_rows) : seg_row(a.f_idx, sf.b + i - sr.n, a.f_rows);
  const int64_t off = (int64_t)row * (real ? a.r_ld : a.f_ld) + c;
  const void* x = real ? a.r : a.f;
  return a.f64 ? ((const double*)x)[off] : (double)((const float*)x)[off];
}

// p = sigmoid(t), q = 1 - p, neither by cancellation
__device__ __forceinline__ void lg_pq(double t, double& p, double& q) {
  const double e = exp(-fabs(t)), inv = 1.0 / (1.0 + e);
  if (t >= 0.0) { p = inv; q = e * inv; } else { p = e * inv; q = inv; }
}
// softplus(t) - y t = softplus(-t) for y = 1, softplus(t) for y = 0; no overflow
__device__ __forceinline__ double lg_loss(double t, bool y) {
  const double s = y ? -t : t;
  return fmax(s, 0.0) + log1p(exp(-fabs(s)));
}

__global__ void __launch_bounds__(LG_THREADS) lg_init_kernel(LgArgs a, int n_seg, double* state, double* theta,
                                                             double* stat) {
  const int s = blockIdx.x, P = a.cols + 1;
  const SegSpan sr = seg_span(a.r_seg, s, a.r_rows, a.r_cap), sf = seg_span(a.f_seg, s, a.f_rows, a.f_cap);
  const bool degenerate = sr.n == 0 || sf.n == 0;
  const double nan = __builtin_nan("");
  double* st = state + (int64_t)s * LG_STATE;
  for (int c = threadIdx.x; c < 2 * LG_PP; c += LG_THREADS) st[c] = 0.0;
  for (int c = threadIdx.x; c < P; c += LG_THREADS) theta[(int64_t)s * P + c] = degenerate ? nan : 0.0;
  if (threadIdx.x == 0) {
    st[LG_F] = __builtin_inf();
    st[LG_G] = nan;
    st[LG_IT] = 0.0;
    st[LG_STATUS] = degenerate ? -1.0 : 0.0;
    st[LG_DONE] = degenerate ? 1.0 : 0.0;
    st[LG_REEVAL] = 0.0;
    stat[4 * s + 0] = nan;
    stat[4 * s + 1] = nan;
    stat[4 * s + 2] = 0.0;
    stat[4 * s + 3] = degenerate ? -1.0 : 0.0;
  }
}

__global__ void __launch_bounds__(LG_THREADS) lg_pass_kernel(LgArgs a, int nblk, const double* state, double* part) {
  __shared__ double z[LG_STAGE * LG_LDZ];
  __shared__ double th[LG_PP], dd[LG_PP];
  __shared__ double wr[LG_STAGE], rr[LG_STAGE];
  __shared__ double fj[LG_STAGE * LG_STEPS];
  const int blk = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const double* st = state + (int64_t)s * LG_STATE;
  if (st[LG_DONE] != 0.0) return;                    // block-uniform
  const SegSpan sr = seg_span(a.r_seg, s, a.r_rows, a.r_cap), sf = seg_span(a.f_seg, s, a.f_rows, a.f_cap);
  const int n = sr.n + sf.n, first = blk * LG_ROWS;
  if (first >= n) return;
  const int P = a.cols + 1, T = (P + 3) / 4, PS = 4 * T, ntile = lg_tiles(T);
  for (int c = tid; c < LG_PP; c += LG_THREADS) { th[c] = st[c]; dd[c] = st[LG_PP + c]; }
  int ti = 0, tj = 0;
  if (tid < ntile) lg_tile_of(tid, T, ti, tj);
  double acc[4][4] = {};
  double g = 0.0, fl = 0.0;
  for (int r0 = first; r0 < first + LG_ROWS && r0 < n; r0 += LG_STAGE) {
    __syncthreads();
    for (int e = tid; e < LG_STAGE * PS; e += LG_THREADS) {
      const int r = e / PS, c = e - r * PS, i = r0 + r;
      double v = 0.0;
      if (i < n && c < P) v = c == 0 ? 1.0 : lg_value(a, sr, sf, i, c - 1);
      z[r * LG_LDZ + c] = v;
    }
    __syncthreads();
    if (tid < LG_STAGE) {
      const int r = tid, i = r0 + r;
      double t0 = th[0], td = dd[0], w = 0.0, res = 0.0;
      for (int c = 1; c < P; ++c) {
        const double v = z[r * LG_LDZ + c];
        t0 = fma(th[c], v, t0);
        td = fma(dd[c], v, td);
      }
      const bool live = i < n, y = i < sr.n;
      if (live) {
        double p, q;
        lg_pq(t0 + td, p, q);
        w = p * q;
        res = y ? -q : p;
      }
      wr[r] = w;
      rr[r] = res;
      double scale = 1.0;
#pragma unroll
      for (int j = 0; j < LG_STEPS; ++j) {
        fj[r * LG_STEPS + j] = live ? lg_loss(t0 + scale * td, y) : 0.0;
        scale *= 0.5;
      }
    }
    __syncthreads();
    if (tid < ntile) {
      for (int r = 0; r < LG_STAGE; ++r) {
        const double w = wr[r];
        const double* zr = z + r * LG_LDZ;
        double zb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) zb[j] = zr[4 * tj + j];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double wa = w * zr[4 * ti + i];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fma(wa, zb[j], acc[i][j]);
        }
      }
    }
    if (tid < PS) {
      for (int r = 0; r < LG_STAGE; ++r) g = fma(rr[r], z[r * LG_LDZ + tid], g);
    }
    if (tid >= LG_THREADS - LG_STEPS) {              // the last wave's threads: not the busiest ones
      const int j = tid - (LG_THREADS - LG_STEPS);
      for (int r = 0; r < LG_STAGE; ++r) fl += fj[r * LG_STEPS + j];
    }
  }
  double* out = part + ((int64_t)s * nblk + blk) * lg_part(a.cols);
  if (tid < ntile) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) out[tid * 16 + i * 4 + j] = acc[i][j];
  }
  if (tid < PS) out[ntile * 16 + tid] = g;
  if (tid >= LG_THREADS - LG_STEPS) out[ntile * 16 + PS + tid - (LG_THREADS - LG_STEPS)] = fl;
}

__global__ void __launch_bounds__(LG_THREADS) lg_solve_kernel(LgArgs a, int nblk, int it, int max_iter, double l2,
                                                              double gtol, double* state, const double* part,
                                                              double* theta, double* stat) {
  __shared__ double H[LG_PP * LG_LDZ];
  __shared__ double g[LG_PP], b[LG_PP], x[LG_PP], th[LG_PP], dd[LG_PP], F[LG_STEPS];
  __shared__ int fail;
  const int s = blockIdx.x, tid = threadIdx.x;
  double* st = state + (int64_t)s * LG_STATE;
  if (st[LG_DONE] != 0.0) return;                    // block-uniform
  const SegSpan sr = seg_span(a.r_seg, s, a.r_rows, a.r_cap), sf = seg_span(a.f_seg, s, a.f_rows, a.f_cap);
  const int n = sr.n + sf.n, nb = (n + LG_ROWS - 1) / LG_ROWS;
  const int P = a.cols + 1, T = (P + 3) / 4, PS = 4 * T, ntile = lg_tiles(T), stride = lg_part(a.cols);
  const double* p0 = part + (int64_t)s * nblk * stride;
  const double inv_n = 1.0 / (double)n, ridge = l2 * inv_n;
  // the state is read here, before the first barrier, and written behind the last one
  const double Fb = st[LG_F], reeval = st[LG_REEVAL], it_in = st[LG_IT], g_in = st[LG_G];
  if (tid == 0) fail = 0;
  for (int c = tid; c < LG_PP; c += LG_THREADS) { th[c] = st[c]; dd[c] = st[LG_PP + c]; }
  // the blocks' partials in block order
  for (int e = tid; e < ntile * 16; e += LG_THREADS) {
    int ti, tj;
    lg_tile_of(e >> 4, T, ti, tj);
    const int row = 4 * ti + ((e >> 2) & 3), col = 4 * tj + (e & 3);
    if (row > col || col >= P) continue;             // a diagonal tile's lower half; the padding
    double v = 0.0;
    for (int k = 0; k < nb; ++k) v += p0[(int64_t)k * stride + e];
    v = v * inv_n + (row == col && row > 0 ? ridge : 0.0);
    H[row * LG_LDZ + col] = v;
    H[col * LG_LDZ + row] = v;
  }
  for (int e = tid; e < PS + LG_STEPS; e += LG_THREADS) {
    double v = 0.0;
    for (int k = 0; k < nb; ++k) v += p0[(int64_t)k * stride + ntile * 16 + e];
    if (e < PS) g[e] = v * inv_n;
    else F[e - PS] = v * inv_n;
  }
  __syncthreads();
  if (tid < LG_STEPS) {                              // the penalty at theta + 2^-j d
    const double al = 1.0 / (double)(1 << tid);
    double q = 0.0;
    for (int c = 1; c < P; ++c) {
      const double w = th[c] + al * dd[c];
      q = fma(w, w, q);
    }
    F[tid] += 0.5 * ridge * q;
  }
  if (tid > 64 && tid < 64 + P) g[tid - 64] += ridge * (th[tid - 64] + dd[tid - 64]);   // the second wave's
  __syncthreads();
  // accept, shorten or stop (every thread takes the same decision from the same LDS values)
  const double slack = ((double)n + 64.0) * 2.220446049250313e-16 * fabs(Fb);
  const bool last = it >= max_iter;
  double iters = it_in, status = 0.0, done = 0.0, Fnew = Fb, gn = g_in;
  double alpha = 0.0;
  bool newton = false;                               // g, H hold at the new theta: test it, take the next step
  if (it == 0 || reeval != 0.0 || F[0] <= Fb + slack) {
    alpha = 1.0;
    Fnew = F[0];
    newton = true;
    if (it != 0 && reeval == 0.0) iters += 1.0;
  } else if (last) {
    done = 1.0;
  } else {
    int best = 0;
    for (int j = 1; j < LG_STEPS; ++j)
      if (F[j] < Fnew) { Fnew = F[j]; best = j; }
    if (best == 0) {
      done = 1.0;                                    // no trial point lowers F: stalled
    } else {
      alpha = 1.0 / (double)(1 << best);
      iters += 1.0;
    }
  }
  if (newton) {
    double m = 0.0;
    for (int c = 0; c < P; ++c) m = fmax(m, fabs(g[c]));
    gn = m;
    if (!(gn > gtol)) { status = 1.0; done = 1.0; }
    else if (last) done = 1.0;
  }
  const bool solve = newton && done == 0.0;
  if (solve) {
    // H = L L^T in place (lower triangle), right-looking
    for (int j = 0; j < P; ++j) {
      const double djj = H[j * LG_LDZ + j];
      if (!(djj > 0.0)) {
        if (tid == 0) fail = 1;
        break;                                       // uniform: every thread reads the same pivot
      }
      const double ljj = sqrt(djj);
      __syncthreads();
      for (int i = j + tid; i < P; i += LG_THREADS) H[i * LG_LDZ + j] = i == j ? ljj : H[i * LG_LDZ + j] / ljj;
      __syncthreads();
      const int rem = P - j - 1;
      for (int e = tid; e < rem * rem; e += LG_THREADS) {
        const int i = j + 1 + e / rem, k = j + 1 + e % rem;
        if (k <= i) H[i * LG_LDZ + k] -= H[i * LG_LDZ + j] * H[k * LG_LDZ + j];
      }
      __syncthreads();
    }
    __syncthreads();
    if (fail == 0) {
      for (int c = tid; c < P; c += LG_THREADS) b[c] = -g[c];
      __syncthreads();
      for (int j = 0; j < P; ++j) {                  // L y = -g
        const double yj = b[j] / H[j * LG_LDZ + j];
        __syncthreads();
        if (tid == 0) b[j] = yj;
        for (int i = j + 1 + tid; i < P; i += LG_THREADS) b[i] -= H[i * LG_LDZ + j] * yj;
        __syncthreads();
      }
      for (int j = P - 1; j >= 0; --j) {             // L^T x = y
        const double xj = b[j] / H[j * LG_LDZ + j];
        __syncthreads();
        if (tid == 0) x[j] = xj;
        for (int i = tid; i < j; i += LG_THREADS) b[i] -= H[j * LG_LDZ + i] * xj;
        __syncthreads();
      }
    }
  }
  const bool failed = solve && fail != 0;            // the factorisation broke down: stop where we are
  if (failed) done = 1.0;
  __syncthreads();
  for (int c = tid; c < P; c += LG_THREADS) {
    const double t = th[c] + alpha * dd[c];
    st[c] = t;
    st[LG_PP + c] = solve && !failed ? x[c] : 0.0;
    theta[(int64_t)s * P + c] = t;
  }
  if (tid == 0) {
    st[LG_F] = Fnew;
    st[LG_G] = gn;
    st[LG_IT] = iters;
    st[LG_STATUS] = status;
    st[LG_DONE] = done;
    st[LG_REEVAL] = (!newton && done == 0.0) ? 1.0 : 0.0;
    stat[4 * s + 0] = Fnew;
    stat[4 * s + 1] = gn;
    stat[4 * s + 2] = iters;
    stat[4 * s + 3] = status;
  }
}

// ------------------------------------------------------------------------------------------ scores
constexpr int SC_THREADS = 256;

__global__ void __launch_bounds__(SC_THREADS) lg_score_kernel(LgArgs a, int nblk, const double* theta,
                                                              double* r_scores, double* f_scores, double* part) {
  __shared__ double th[LG_PMAX];
  __shared__ double shd[SC_THREADS / 64];
  const int blk = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, P = a.cols + 1;
  const SegSpan sr = seg_span(a.r_seg, s, a.r_rows, a.r_cap), sf = seg_span(a.f_seg, s, a.f_rows, a.f_cap);
  const int n = sr.n + sf.n, i = blk * SC_THREADS + tid;
  if (blk * SC_THREADS >= n) return;                 // block-uniform
  for (int c = tid; c < P; c += SC_THREADS) th[c] = theta[(int64_t)s * P + c];
  __syncthreads();
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < n) {
    const bool y = i < sr.n;
    double t = th[0];
    for (int c = 1; c < P; ++c) t = fma(th[c], lg_value(a, sr, sf, i, c - 1), t);
    if (y) r_scores[(int64_t)s * a.r_cap + i] = t;
    else f_scores[(int64_t)s * a.f_cap + (i - sr.n)] = t;
    const double loss = lg_loss(t, y);
    if (y) { v[0] = t > 0.0 ? 1.0 : 0.0; v[2] = loss; }
    else { v[1] = t <= 0.0 ? 1.0 : 0.0; v[3] = loss; }
  }
  double* out = part + ((int64_t)s * nblk + blk) * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double t = block_sum_d(v[q], shd);
    if (tid == 0) out[q] = t;
  }
}

__global__ void __launch_bounds__(64) lg_score_sum_kernel(LgArgs a, int nblk, const double* part, int32_t* r_oseg,
                                                          int32_t* f_oseg, double* sums) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const SegSpan sr = seg_span(a.r_seg, s, a.r_rows, a.r_cap), sf = seg_span(a.f_seg, s, a.f_rows, a.f_cap);
  const int n = sr.n + sf.n, nb = (n + SC_THREADS - 1) / SC_THREADS;
  if (tid < 4) {
    double v = 0.0;
    for (int k = 0; k < nb; ++k) v += part[((int64_t)s * nblk + k) * 4 + tid];
    sums[4 * s + tid] = v;
  }
  if (tid == 4) { r_oseg[2 * s] = s * a.r_cap; r_oseg[2 * s + 1] = s * a.r_cap + sr.n; }
  if (tid == 5) { f_oseg[2 * s] = s * a.f_cap; f_oseg[2 * s + 1] = s * a.f_cap + sf.n; }
}

bool lg_limits(int n_seg, int cols, int r_cap, int f_cap) {
  return n_seg >= 1 && n_seg <= ES_DIST_MAX_SEG && cols >= 1 && cols <= ES_LOGIT_MAX_COLS && r_cap >= 1 &&
         r_cap <= ES_DIST_MAX_ROWS && f_cap >= 1 && f_cap <= ES_DIST_MAX_ROWS;
}
int lg_blocks(int r_cap, int f_cap, int per) { return (int)(((int64_t)r_cap + f_cap + per - 1) / per); }

}  // namespace

extern "C" int es_logit_block_rows(void) { return ES_LOGIT_BLOCK_ROWS; }

extern "C" size_t es_logit_fit_workspace(int n_seg, int cols, int r_cap, int f_cap) {
  if (!lg_limits(n_seg, cols, r_cap, f_cap)) return 0;
  Carver cv(nullptr, 256);
  cv.take<double>((size_t)n_seg * LG_STATE);
  cv.take<double>((size_t)n_seg * lg_blocks(r_cap, f_cap, LG_ROWS) * lg_part(cols));
  return cv.bytes();
}

extern "C" size_t es_logit_scores_workspace(int n_seg, int r_cap, int f_cap) {
  if (!lg_limits(n_seg, 1, r_cap, f_cap)) return 0;
  return (size_t)n_seg * lg_blocks(r_cap, f_cap, SC_THREADS) * 4 * sizeof(double);
}

#define LG_CHECK_TABLES(name)                                                                                       \
  ES_CHECK_ARG(real && fake && r_seg && f_seg, name ": null argument");                                             \
  ES_CHECK_ARG(cols >= 1 && cols <= ES_LOGIT_MAX_COLS && r_ld >= cols && f_ld >= cols,                              \
               name ": cols=%d r_ld=%lld f_ld=%lld outside 1 <= cols <= %d, cols <= ld", cols, (long long)r_ld,     \
               (long long)f_ld, ES_LOGIT_MAX_COLS);                                                                 \
  ES_CHECK_ARG(r_rows >= 1 && r_rows <= ES_DIST_MAX_ROWS && f_rows >= 1 && f_rows <= ES_DIST_MAX_ROWS &&            \
                   lg_limits(n_seg, cols, r_cap, f_cap),                                                            \
               name ": r_rows=%d r_cap=%d f_rows=%d f_cap=%d n_seg=%d outside 1 <= rows, cap <= %d, "               \
                    "1 <= n_seg <= %d", r_rows, r_cap, f_rows, f_cap, n_seg, ES_DIST_MAX_ROWS, ES_DIST_MAX_SEG)

extern "C" int es_logit_fit(const void* real, int64_t r_ld, int r_rows, const int32_t* r_idx, const int32_t* r_seg,
                            int r_cap, const void* fake, int64_t f_ld, int f_rows, const int32_t* f_idx,
                            const int32_t* f_seg, int f_cap, int x_f64, int cols, int n_seg, double l2, double gtol,
                            int max_iter, double* theta, double* stat, void* work, size_t work_bytes,
                            es_stream_t stream) {
  LG_CHECK_TABLES("logit_fit");
  ES_CHECK_ARG(theta && stat, "logit_fit: null argument");
  ES_CHECK_ARG(max_iter >= 1 && max_iter <= ES_LOGIT_MAX_ITER, "logit_fit: max_iter = %d outside 1 .. %d", max_iter,
               ES_LOGIT_MAX_ITER);
  ES_CHECK_ARG(l2 >= 0.0 && gtol >= 0.0, "logit_fit: l2 = %g, gtol = %g (neither may be negative or NaN)", l2, gtol);
  const size_t need = es_logit_fit_workspace(n_seg, cols, r_cap, f_cap);
  ES_CHECK_ARG(work && work_bytes >= need, "logit_fit: workspace of %zu bytes, %zu needed", work_bytes, need);
  const int nblk = lg_blocks(r_cap, f_cap, LG_ROWS);
  Carver cv(work, 256);
  double* state = cv.take<double>((size_t)n_seg * LG_STATE);
  double* part = cv.take<double>((size_t)n_seg * nblk * lg_part(cols));
  const LgArgs a = {real, r_ld, r_rows, r_idx, r_seg, r_cap, fake, f_ld, f_rows, f_idx, f_seg, f_cap, x_f64 != 0, cols};
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lg_init_kernel, dim3(n_seg), dim3(LG_THREADS), 0, st, a, n_seg, state, theta, stat);
  for (int it = 0; it <= max_iter; ++it) {
    hipLaunchKernelGGL(lg_pass_kernel, dim3(nblk, n_seg), dim3(LG_THREADS), 0, st, a, nblk, state, part);
    hipLaunchKernelGGL(lg_solve_kernel, dim3(n_seg), dim3(LG_THREADS), 0, st, a, nblk, it, max_iter, l2, gtol, state,
                       part, theta, stat);
  }
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_logit_scores(const void* real, int64_t r_ld, int r_rows, const int32_t* r_idx, const int32_t* r_seg,
                               int r_cap, const void* fake, int64_t f_ld, int f_rows, const int32_t* f_idx,
                               const int32_t* f_seg, int f_cap, int x_f64, int cols, int n_seg, const double* theta,
                               double* r_scores, double* f_scores, int32_t* r_oseg, int32_t* f_oseg, double* sums,
                               void* work, size_t work_bytes, es_stream_t stream) {
  LG_CHECK_TABLES("logit_scores");
  ES_CHECK_ARG(theta && r_scores && f_scores && r_oseg && f_oseg && sums, "logit_scores: null argument");
  ES_CHECK_ARG((int64_t)n_seg * r_cap <= INT_MAX && (int64_t)n_seg * f_cap <= INT_MAX,
               "logit_scores: n_seg x cap = %d x max(%d, %d) above 2^31 - 1", n_seg, r_cap, f_cap);
  const size_t need = es_logit_scores_workspace(n_seg, r_cap, f_cap);
  ES_CHECK_ARG(work && work_bytes >= need, "logit_scores: workspace of %zu bytes, %zu needed", work_bytes, need);
  const int nblk = lg_blocks(r_cap, f_cap, SC_THREADS);
  const LgArgs a = {real, r_ld, r_rows, r_idx, r_seg, r_cap, fake, f_ld, f_rows, f_idx, f_seg, f_cap, x_f64 != 0, cols};
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lg_score_kernel, dim3(nblk, n_seg), dim3(SC_THREADS), 0, st, a, nblk, theta, r_scores, f_scores,
                     (double*)work);
  hipLaunchKernelGGL(lg_score_sum_kernel, dim3(n_seg), dim3(64), 0, st, a, nblk, (const double*)work, r_oseg, f_oseg,
                     sums);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
