// Clustering on the device (the proton sets' expert_number column, scikit-learn's KMeans(algorithm="lloyd"))
// and the confusion matrix behind the router-agreement numbers.  include/expertsim_hip.h defines every entry
// to the letter; this header says how the work is laid out.
//
// x [rows][ld] fp32 or fp64, unit column stride; all value arithmetic fp64, contraction off, no float atomics.
//
// Distances (es_kmeans_assign, and the candidate distances of es_kmeans_plusplus): one wave per row, the
// waves of the grid striding over the rows.  Lane l adds (x[c] - centre[c])^2 for c = l, l + 64, .. in that
// order from +0.0 and the wave closes with the wave_sum_d butterfly, so a wave instruction loads 256
// contiguous bytes of an fp32 row (512 of an fp64 row).  KM_KC = 8 centres share one sweep over the row; more
// centres take ceil(K / 8) sweeps, of which the later ones hit the cache the first filled.  The centres are
// staged in LDS when K * cols * 8 <= 64 KiB (the proton shape with K = 4: 53760 bytes) and read from global
// memory (L2) above.
// Sums over rows (the inertia, a candidate's potential): km_reduce -- chunks of 4096 rows, 1024 threads, thread
// t adds t, t + 1024, t + 2048, t + 3072 from +0.0, block_sum_d; the chunk sums likewise in a second launch.
//
// es_kmeans_update: a second pass over x.  The rows are cut into n_c = min(256, ceil(rows / 256),
// max(1, floor(2^24 / (K cols)))) chunks of L = ceil(rows / n_c); a 128-thread workgroup per (chunk, 128-column tile) walks its rows in order and adds
// each into the LDS row of its label (a thread owns its column, so the order is the row order; 512 contiguous
// bytes of an fp32 row per wave pair).  A one-workgroup launch counts the labels (integer LDS atomics) and, for
// every empty cluster, picks its row; the last launches close the chunk sums in chunk order, apply the
// relocation, scale and write the squared shift.
//
// es_confusion_matrix: an int32 LDS histogram per workgroup, merged by 64-bit integer atomics on global memory.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "segment.h"

namespace {

constexpr int KM_MAX_COLS = ES_KMEANS_MAX_COLS;
constexpr int KM_MAX_K = ES_KMEANS_MAX_K;
constexpr int KM_MAX_ROWS = ES_KMEANS_MAX_ROWS;
constexpr int KM_KC = 8;                    // centres per sweep over a row
constexpr int KM_DIST_THREADS = 512;        // 8 rows per workgroup step
constexpr int KM_LDS_CENTRES = 65536;       // bytes of centres staged in LDS
constexpr int KM_RED = 4096;                // rows of one reduction chunk
constexpr int KM_TILE = 128;                // columns of one update workgroup
constexpr int KM_CHUNK_MIN = 256;
constexpr int KM_MAX_CHUNKS = 256;
constexpr int KM_MAX_PARTIALS = 1 << 24;   // doubles of chunk sums
constexpr int KM_MAX_TRIALS = 8;            // 2 + int(ln 64) = 6
constexpr int CM_MAX_CELLS = ES_CONFUSION_MAX_CELLS;

int km_red_chunks(int rows) { return (rows + KM_RED - 1) / KM_RED; }
// chunks of the update's row sums: at least 256 rows each, at most 256 chunks and 2^24 chunk sums (128 MiB)
int km_chunks(int rows, int cols, int K) {
  int c = (rows + KM_CHUNK_MIN - 1) / KM_CHUNK_MIN;
  const int fit = KM_MAX_PARTIALS / (K * cols);
  c = c < KM_MAX_CHUNKS ? c : KM_MAX_CHUNKS;
  c = c < fit ? c : fit;
  return c > 1 ? c : 1;
}
int km_tiles(int cols) { return (cols + KM_TILE - 1) / KM_TILE; }
constexpr size_t KM_ALIGN = 16;             // of every array of a workspace

// ------------------------------------------------------------------------------------------ distances
// PP = false: label / dist of the nearest centre (the lowest index wins a tie).
// PP = true:  out[j][row] = min(closest[row], d(row, centre j)) (closest NULL: d itself).
template <typename T, bool PP, bool LDS>
__global__ void __launch_bounds__(KM_DIST_THREADS) kmeans_dist_kernel(
    const T* __restrict__ x, int64_t ld, int rows, int cols, const double* __restrict__ centres, int K,
    int32_t* __restrict__ label, double* __restrict__ dist, const double* __restrict__ closest,
    double* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double km_lds[];
  if (LDS) {
    for (int i = threadIdx.x; i < K * cols; i += KM_DIST_THREADS) km_lds[i] = centres[i];
    __syncthreads();                                  // the only barrier: the row loop below has none
  }
  const int lane = threadIdx.x & 63;
  const int wpb = KM_DIST_THREADS / 64;
  for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < rows; row += gridDim.x * wpb) {
    const T* xr = x + (int64_t)row * ld;
    double best = 0.0;
    int best_k = 0;
    for (int k0 = 0; k0 < K; k0 += KM_KC) {
      double acc[KM_KC];
      int ck[KM_KC];
#pragma unroll
      for (int j = 0; j < KM_KC; ++j) {
        acc[j] = 0.0;
        ck[j] = (k0 + j < K ? k0 + j : K - 1) * cols;   // past K: a valid centre whose sum is not used
      }
#pragma unroll 4
      for (int col = lane; col < cols; col += 64) {
        const double xv = (double)xr[col];
#pragma unroll
        for (int j = 0; j < KM_KC; ++j) {
          const double d = xv - (LDS ? km_lds[ck[j] + col] : centres[ck[j] + col]);
          const double q = d * d;
          acc[j] += q;
        }
      }
#pragma unroll
      for (int j = 0; j < KM_KC; ++j) {
        const double d = wave_sum_d(acc[j]);
        const int k = k0 + j;
        if (k < K) {                                  // wave-uniform
          if (PP) {
            if (lane == 0) {
              const double m = closest ? closest[row] : d;
              out[(int64_t)k * rows + row] = d < m ? d : m;
            }
          } else if (k == 0 || d < best) {
            best = d;
            best_k = k;
          }
        }
      }
    }
    if (!PP && lane == 0) {
      label[row] = best_k;
      dist[row] = best;
    }
  }
}

// ------------------------------------------------------------------------------------------ ordered sums
// part[b][chunk] = the chunk's sum of v[b][rows]; cpart[chunk] = its rows with label != label_old (b == 0 only)
__global__ void __launch_bounds__(1024) kmeans_reduce1_kernel(const double* __restrict__ v, int rows, int nred,
                                                              double* __restrict__ part,
                                                              const int32_t* __restrict__ label,
                                                              const int32_t* __restrict__ label_old,
                                                              int64_t* __restrict__ cpart) {
  __shared__ double sh[16];
  __shared__ int shc;
  const int b = blockIdx.y, chunk = blockIdx.x;
  if (threadIdx.x == 0) shc = 0;
  double a = 0.0;
  int ch = 0;
#pragma unroll
  for (int i = 0; i < KM_RED / 1024; ++i) {
    const int r = chunk * KM_RED + i * 1024 + (int)threadIdx.x;
    if (r < rows) {
      a += v[(int64_t)b * rows + r];
      if (cpart && b == 0) ch += label_old ? (label[r] != label_old[r]) : 1;
    }
  }
  a = block_sum_d(a, sh);                             // its barriers also order shc = 0
  if (cpart && b == 0) {
    if (ch) atomicAdd(&shc, ch);                      // integer: order does not matter
    __syncthreads();
    if (threadIdx.x == 0) cpart[chunk] = shc;
  }
  if (threadIdx.x == 0) part[(int64_t)b * nred + chunk] = a;
}
__global__ void __launch_bounds__(1024) kmeans_reduce2_kernel(const double* __restrict__ part, int nred,
                                                              double* __restrict__ out,
                                                              const int64_t* __restrict__ cpart,
                                                              int64_t* __restrict__ changed) {
  __shared__ double sh[16];
  const int b = blockIdx.x;
  double a = 0.0;
  for (int i = threadIdx.x; i < nred; i += 1024) a += part[(int64_t)b * nred + i];
  a = block_sum_d(a, sh);
  if (threadIdx.x == 0) {
    out[b] = a;
    if (changed && b == 0) {
      int64_t c = 0;
      for (int i = 0; i < nred; ++i) c += cpart[i];
      changed[0] = c;
    }
  }
}

// ------------------------------------------------------------------------------------------ update
__device__ __forceinline__ int km_label(const int32_t* label, int r, int K) {
  const int l = label[r];
  return l < 0 ? 0 : (l >= K ? K - 1 : l);
}

template <typename T>
__global__ void __launch_bounds__(KM_TILE) kmeans_partial_kernel(const T* __restrict__ x, int64_t ld, int rows,
                                                                 int cols, const int32_t* __restrict__ label, int K,
                                                                 int L, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double km_lds[];   // [K][KM_TILE]; a thread owns its column
  const int t = threadIdx.x, col = blockIdx.x * KM_TILE + t, chunk = blockIdx.y;
  const bool live = col < cols;
  for (int k = 0; k < K; ++k) km_lds[k * KM_TILE + t] = 0.0;
  const int lo = chunk * L < rows ? chunk * L : rows, hi = lo + L < rows ? lo + L : rows;
  const T* xc = x + (live ? col : 0);
  int r = lo;
  for (; r + 8 <= hi; r += 8) {
    T v[8];
    int lab[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = live ? xc[(int64_t)(r + j) * ld] : (T)0;
      lab[j] = km_label(label, r + j, K);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) km_lds[lab[j] * KM_TILE + t] += (double)v[j];
  }
  for (; r < hi; ++r) km_lds[km_label(label, r, K) * KM_TILE + t] += live ? (double)xc[(int64_t)r * ld] : 0.0;
  if (live)
    for (int k = 0; k < K; ++k) partial[((int64_t)chunk * K + k) * cols + col] = km_lds[k * KM_TILE + t];
}

// meta (int32): [0, 64) the label counts, [64] n_empty, [128, 192) the empty clusters ascending,
// [192, 256) the row each of them takes (-1: none left)
constexpr int KM_META = 256;

struct KmPick { double d; int r; };
// a is better: the larger dist, the lower row on a tie; r < 0 is no pick
__device__ __forceinline__ bool km_better(double ad, int ar, double bd, int br) {
  if (ar < 0) return false;
  if (br < 0) return true;
  return ad > bd || (ad == bd && ar < br);
}

__global__ void __launch_bounds__(1024) kmeans_count_kernel(const int32_t* __restrict__ label,
                                                            const double* __restrict__ dist, int rows, int K,
                                                            int32_t* __restrict__ meta) {
  __shared__ int cnt[KM_MAX_K];
  __shared__ int empty[KM_MAX_K];
  __shared__ int n_empty_s;
  __shared__ double wd[16];
  __shared__ int wr[16];
  __shared__ double prev_d;
  __shared__ int prev_r;
  const int t = threadIdx.x;
  if (t < KM_MAX_K) cnt[t] = 0;
  __syncthreads();
  for (int r = t; r < rows; r += 1024) atomicAdd(&cnt[km_label(label, r, K)], 1);
  __syncthreads();
  if (t == 0) {
    int n = 0;
    for (int k = 0; k < K; ++k)
      if (cnt[k] == 0) empty[n++] = k;
    n_empty_s = n;
    prev_r = -1;
    prev_d = 0.0;
  }
  __syncthreads();
  const int n_empty = n_empty_s;
  if (t < KM_MAX_K) {
    meta[t] = t < K ? cnt[t] : 0;
    meta[128 + t] = t < n_empty ? empty[t] : -1;
  }
  if (t == 0) meta[64] = n_empty;
  for (int j = 0; j < n_empty; ++j) {                 // block-uniform trip count
    const double pd = prev_d;
    const int pr = prev_r;
    double bd = 0.0;
    int br = -1;
    for (int r = t; r < rows; r += 1024) {
      const double d = dist[r];
      const bool after = pr < 0 || d < pd || (d == pd && r > pr);   // not yet taken, in the pick order
      if (after && km_better(d, r, bd, br)) { bd = d; br = r; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double od = __shfl_xor(bd, o, 64);
      const int orr = __shfl_xor(br, o, 64);
      if (km_better(od, orr, bd, br)) { bd = od; br = orr; }
    }
    __syncthreads();                                  // every thread has read prev_d / prev_r
    if ((t & 63) == 0) { wd[t >> 6] = bd; wr[t >> 6] = br; }
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < 16; ++w)
        if (km_better(wd[w], wr[w], bd, br)) { bd = wd[w]; br = wr[w]; }
      meta[192 + j] = br;
      prev_d = bd;
      prev_r = br < 0 ? INT_MAX : br;                 // nothing left: nothing is after it either
      if (br < 0) prev_d = -1.0;
    }
    __syncthreads();
  }
}

template <typename T>
__global__ void __launch_bounds__(KM_TILE) kmeans_centres_kernel(const T* __restrict__ x, int64_t ld, int rows,
                                                                 int cols, const int32_t* __restrict__ label, int K,
                                                                 int nchunks, const double* __restrict__ partial,
                                                                 const int32_t* __restrict__ meta,
                                                                 const double* __restrict__ c_old,
                                                                 double* __restrict__ c_new,
                                                                 double* __restrict__ shift_part) {
#pragma clang fp contract(off)
  __shared__ double sh[2];
  const int t = threadIdx.x, col = blockIdx.x * KM_TILE + t, k = blockIdx.y;
  const bool live = col < cols;
  double q = 0.0;
  if (live) {
    double s = 0.0;
    for (int ch = 0; ch < nchunks; ++ch) s += partial[((int64_t)ch * K + k) * cols + col];
    int cnt = meta[k];
    int n_empty = meta[64];
    n_empty = n_empty < 0 ? 0 : (n_empty > K ? K : n_empty);
    for (int j = 0; j < n_empty; ++j) {
      const int row = meta[192 + j];
      if (row < 0 || row >= rows) continue;
      const double xv = (double)x[(int64_t)row * ld + col];
      if (meta[128 + j] == k) {
        s = xv;
        cnt = 1;
      } else if (km_label(label, row, K) == k) {
        s -= xv;
        cnt -= 1;
      }
    }
    double c = s;
    if (cnt > 0) {
      const double alpha = 1.0 / (double)cnt;
      c = s * alpha;
    }
    c_new[(int64_t)k * cols + col] = c;
    const double d = c - c_old[(int64_t)k * cols + col];
    q = d * d;
  }
  q = wave_sum_d(q);
  if ((t & 63) == 0) sh[t >> 6] = q;
  __syncthreads();
  if (t == 0) shift_part[(int64_t)k * gridDim.x + blockIdx.x] = sh[0] + sh[1];
}

// out[0] = the n parts: lane l adds l, l + 64, .. from +0.0, then the butterfly
__global__ void __launch_bounds__(64) kmeans_shift_kernel(const double* __restrict__ part, int n,
                                                          double* __restrict__ out) {
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) a += part[i];
  a = wave_sum_d(a);
  if (threadIdx.x == 0) out[0] = a;
}

// ------------------------------------------------------------------------------------------ k-means++
// cand[0 .. T): step 0: the row floor(u[0] * rows); later: searchsorted(cumsum(closest), u[j] * total), clipped.
// cumsum: 1024 segments of Ls = ceil(rows / 1024) rows; local_i = the segment's sequential sum from +0.0 up to
// row i; off_t = the segment totals added in segment order from +0.0; cumsum[i] = off_t + local_i.
__global__ void __launch_bounds__(1024) kmeans_pp_draw_kernel(const double* __restrict__ closest, int rows,
                                                              const double* __restrict__ u, int T, int step,
                                                              int32_t* __restrict__ cand) {
#pragma clang fp contract(off)
  __shared__ double off[1025];
  __shared__ int found[KM_MAX_TRIALS];
  const int t = threadIdx.x;
  if (step == 0) {
    if (t == 0) {
      int r = (int)floor(u[0] * (double)rows);
      cand[0] = r < 0 ? 0 : (r >= rows ? rows - 1 : r);
    }
    return;
  }
  const int Ls = (rows + 1023) / 1024;
  const int lo = (int64_t)t * Ls < rows ? t * Ls : rows, hi = lo + Ls < rows ? lo + Ls : rows;
  double a = 0.0;
  for (int r = lo; r < hi; ++r) a += closest[r];
  off[t + 1] = a;
  if (t < KM_MAX_TRIALS) found[t] = rows - 1;         // the clip: nothing reaches the value
  __syncthreads();
  if (t == 0) {
    double o = 0.0;
    for (int i = 0; i < 1024; ++i) {
      const double seg = off[i + 1];
      off[i] = o;
      o += seg;
    }
    off[1024] = o;
  }
  __syncthreads();
  const double total = off[1024], o = off[t];
  for (int j = 0; j < T; ++j) {
    const double v = u[j] * total;
    if (o + a >= v && hi > lo) {                      // the segment's last cumsum reaches v
      double l = 0.0;
      for (int r = lo; r < hi; ++r) {
        l += closest[r];
        if (o + l >= v) {
          atomicMin(&found[j], r);
          break;
        }
      }
    }
  }
  __syncthreads();
  if (t < T) cand[t] = found[t];
}

template <typename T>
__global__ void __launch_bounds__(256) kmeans_pp_gather_kernel(const T* __restrict__ x, int64_t ld, int rows,
                                                               int cols, const int32_t* __restrict__ cand,
                                                               double* __restrict__ cc) {
  int r = cand[blockIdx.x];
  r = r < 0 ? 0 : (r >= rows ? rows - 1 : r);
  for (int c = threadIdx.x; c < cols; c += 256) cc[(int64_t)blockIdx.x * cols + c] = (double)x[(int64_t)r * ld + c];
}

// the candidate of lowest potential (the first on a tie) becomes centre `step`
__global__ void __launch_bounds__(256) kmeans_pp_select_kernel(const double* __restrict__ pot, int T, int rows,
                                                               int cols, int step, const int32_t* __restrict__ cand,
                                                               const double* __restrict__ cc,
                                                               const double* __restrict__ cdist,
                                                               double* __restrict__ closest,
                                                               double* __restrict__ centres,
                                                               int32_t* __restrict__ index) {
  int best = 0;
  for (int j = 1; j < T; ++j)
    if (pot[j] < pot[best]) best = j;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < rows) closest[i] = cdist[(int64_t)best * rows + i];
  if (i < cols) centres[(int64_t)step * cols + i] = cc[(int64_t)best * cols + i];
  if (i == 0) index[step] = cand[best];
}

// ------------------------------------------------------------------------------------------ confusion matrix
__global__ void __launch_bounds__(256) confusion_kernel(const int32_t* __restrict__ pred,
                                                        const int32_t* __restrict__ target, int64_t n, int n_true,
                                                        int n_pred, unsigned long long* __restrict__ counts,
                                                        unsigned long long* __restrict__ invalid) {
  __shared__ int cell[CM_MAX_CELLS + 1];              // the last cell: pairs outside either range
  const int cells = n_true * n_pred;
  for (int i = threadIdx.x; i <= cells; i += 256) cell[i] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int p = pred[i], t = target[i];
    const bool ok = p >= 0 && p < n_pred && t >= 0 && t < n_true;
    atomicAdd(&cell[ok ? t * n_pred + p : cells], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= cells; i += 256) {
    const int v = cell[i];
    if (v) atomicAdd(i < cells ? counts + i : invalid, (unsigned long long)v);
  }
}

// ------------------------------------------------------------------------------------------ host side
bool km_shape_ok(int64_t ld, int rows, int cols, int K) {
  return rows >= 1 && rows <= KM_MAX_ROWS && cols >= 1 && cols <= KM_MAX_COLS && ld >= cols && K >= 1 &&
         K <= KM_MAX_K && K <= rows;
}

template <bool PP>
void km_launch_dist(const void* x, int x_f64, int64_t ld, int rows, int cols, const double* centres, int K,
                    int32_t* label, double* dist, const double* closest, double* out, hipStream_t st) {
  const size_t cbytes = (size_t)K * cols * sizeof(double);
  const bool use_lds = cbytes <= (size_t)KM_LDS_CENTRES;
  const int wpb = KM_DIST_THREADS / 64;
  int grid = (rows + wpb - 1) / wpb;
  if (grid > 512) grid = 512;                         // the centres are staged once per workgroup
  const size_t lds = use_lds ? cbytes : 0;
#define KM_DIST(T, L)                                                                                         \
  hipLaunchKernelGGL((kmeans_dist_kernel<T, PP, L>), dim3(grid), dim3(KM_DIST_THREADS), lds, st, (const T*)x, ld, \
                     rows, cols, centres, K, label, dist, closest, out)
  if (x_f64 && use_lds) KM_DIST(double, true);
  else if (x_f64) KM_DIST(double, false);
  else if (use_lds) KM_DIST(float, true);
  else KM_DIST(float, false);
#undef KM_DIST
}

// out[b] = the ordered sum of v[b][rows], b < batch; red: batch * nred doubles (+ nred int64 behind them)
void km_launch_reduce(const double* v, int rows, int batch, double* red, double* out, const int32_t* label,
                      const int32_t* label_old, int64_t* cpart, int64_t* changed, hipStream_t st) {
  const int nred = km_red_chunks(rows);
  hipLaunchKernelGGL(kmeans_reduce1_kernel, dim3(nred, batch), dim3(1024), 0, st, v, rows, nred, red, label,
                     label_old, cpart);
  hipLaunchKernelGGL(kmeans_reduce2_kernel, dim3(batch), dim3(1024), 0, st, red, nred, out, cpart, changed);
}

struct KmWork {
  double* red;         // [KM_MAX_TRIALS][nred]
  int64_t* cpart;      // [nred]
  double* partial;     // [nchunks][K][cols]
  double* shift_part;  // [K][tiles]
  int32_t* meta;       // [KM_META]
  size_t bytes;
};
KmWork km_work(void* base, int rows, int cols, int K) {
  const int nred = km_red_chunks(rows);
  Carver c(base, KM_ALIGN);
  KmWork w;
  w.red = c.take<double>((size_t)KM_MAX_TRIALS * nred);
  w.cpart = c.take<int64_t>((size_t)nred);
  w.partial = c.take<double>((size_t)km_chunks(rows, cols, K) * K * cols);
  w.shift_part = c.take<double>((size_t)K * km_tiles(cols));
  w.meta = c.take<int32_t>((size_t)KM_META);
  w.bytes = c.bytes();
  return w;
}

struct PpWork {
  double* red;      // [KM_MAX_TRIALS][nred]
  double* cc;       // [KM_MAX_TRIALS][cols]
  double* cdist;    // [KM_MAX_TRIALS][rows]
  double* closest;  // [rows]
  double* pot;      // [KM_MAX_TRIALS]
  int32_t* cand;    // [KM_MAX_TRIALS]
  size_t bytes;
};
PpWork pp_work(void* base, int rows, int cols) {
  const int nred = km_red_chunks(rows);
  Carver c(base, KM_ALIGN);
  PpWork w;
  w.red = c.take<double>((size_t)KM_MAX_TRIALS * nred);
  w.cc = c.take<double>((size_t)KM_MAX_TRIALS * cols);
  w.cdist = c.take<double>((size_t)KM_MAX_TRIALS * rows);
  w.closest = c.take<double>((size_t)rows);
  w.pot = c.take<double>((size_t)KM_MAX_TRIALS);
  w.cand = c.take<int32_t>((size_t)KM_MAX_TRIALS);
  w.bytes = c.bytes();
  return w;
}

}  // namespace

extern "C" int es_kmeans_trials(int K) { return K >= 1 ? 2 + (int)log((double)K) : 0; }

extern "C" size_t es_kmeans_workspace(int rows, int cols, int K) {
  if (!km_shape_ok(cols, rows, cols, K)) return 0;
  return km_work(nullptr, rows, cols, K).bytes;
}

extern "C" size_t es_kmeans_plusplus_workspace(int rows, int cols, int K) {
  if (!km_shape_ok(cols, rows, cols, K)) return 0;
  return pp_work(nullptr, rows, cols).bytes;
}

extern "C" int es_kmeans_assign(const void* x, int x_f64, int64_t ld, int rows, int cols, const double* centres,
                                int K, const int32_t* label_old, int32_t* label, double* dist, int64_t* changed,
                                double* inertia, void* work, size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(x && centres && label && dist && changed && inertia, "kmeans_assign: null argument");
  ES_CHECK_ARG(x_f64 == 0 || x_f64 == 1, "kmeans_assign: x_f64 = %d, not 0 or 1", x_f64);
  ES_CHECK_ARG(km_shape_ok(ld, rows, cols, K),
               "kmeans_assign: rows=%d cols=%d ld=%lld K=%d outside 1 <= rows <= %d, 1 <= cols <= %d, cols <= ld, "
               "1 <= K <= min(%d, rows)", rows, cols, (long long)ld, K, KM_MAX_ROWS, KM_MAX_COLS, KM_MAX_K);
  ES_CHECK_ARG(label != label_old, "kmeans_assign: label and label_old are the same array");
  const size_t need = es_kmeans_workspace(rows, cols, K);
  ES_CHECK_ARG(work && work_bytes >= need, "kmeans_assign: workspace of %zu bytes, %zu needed", work_bytes, need);
  const KmWork w = km_work(work, rows, cols, K);
  const hipStream_t st = (hipStream_t)stream;
  km_launch_dist<false>(x, x_f64, ld, rows, cols, centres, K, label, dist, nullptr, nullptr, st);
  km_launch_reduce(dist, rows, 1, w.red, inertia, label, label_old, w.cpart, changed, st);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_kmeans_update(const void* x, int x_f64, int64_t ld, int rows, int cols, const int32_t* label,
                                const double* dist, const double* centres_old, int K, double* centres_new,
                                double* shift, void* work, size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(x && label && dist && centres_old && centres_new && shift, "kmeans_update: null argument");
  ES_CHECK_ARG(x_f64 == 0 || x_f64 == 1, "kmeans_update: x_f64 = %d, not 0 or 1", x_f64);
  ES_CHECK_ARG(km_shape_ok(ld, rows, cols, K),
               "kmeans_update: rows=%d cols=%d ld=%lld K=%d outside 1 <= rows <= %d, 1 <= cols <= %d, cols <= ld, "
               "1 <= K <= min(%d, rows)", rows, cols, (long long)ld, K, KM_MAX_ROWS, KM_MAX_COLS, KM_MAX_K);
  ES_CHECK_ARG(centres_new != centres_old, "kmeans_update: centres_new and centres_old are the same array");
  const size_t need = es_kmeans_workspace(rows, cols, K);
  ES_CHECK_ARG(work && work_bytes >= need, "kmeans_update: workspace of %zu bytes, %zu needed", work_bytes, need);
  const KmWork w = km_work(work, rows, cols, K);
  const hipStream_t st = (hipStream_t)stream;
  const int nchunks = km_chunks(rows, cols, K), L = (rows + nchunks - 1) / nchunks, tiles = km_tiles(cols);
  const size_t lds = (size_t)K * KM_TILE * sizeof(double);             // at most 64 KiB
  const dim3 gp(tiles, nchunks), gc(tiles, K), bt(KM_TILE);
  if (x_f64)
    hipLaunchKernelGGL(kmeans_partial_kernel<double>, gp, bt, lds, st, (const double*)x, ld, rows, cols, label, K, L,
                       w.partial);
  else
    hipLaunchKernelGGL(kmeans_partial_kernel<float>, gp, bt, lds, st, (const float*)x, ld, rows, cols, label, K, L,
                       w.partial);
  hipLaunchKernelGGL(kmeans_count_kernel, dim3(1), dim3(1024), 0, st, label, dist, rows, K, w.meta);
  if (x_f64)
    hipLaunchKernelGGL(kmeans_centres_kernel<double>, gc, bt, 0, st, (const double*)x, ld, rows, cols, label, K,
                       nchunks, w.partial, w.meta, centres_old, centres_new, w.shift_part);
  else
    hipLaunchKernelGGL(kmeans_centres_kernel<float>, gc, bt, 0, st, (const float*)x, ld, rows, cols, label, K,
                       nchunks, w.partial, w.meta, centres_old, centres_new, w.shift_part);
  hipLaunchKernelGGL(kmeans_shift_kernel, dim3(1), dim3(64), 0, st, w.shift_part, K * tiles, shift);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_kmeans_plusplus(const void* x, int x_f64, int64_t ld, int rows, int cols, int K, const double* u,
                                  int trials, double* centres, int32_t* index, void* work, size_t work_bytes,
                                  es_stream_t stream) {
  ES_CHECK_ARG(x && u && centres && index, "kmeans_plusplus: null argument");
  ES_CHECK_ARG(x_f64 == 0 || x_f64 == 1, "kmeans_plusplus: x_f64 = %d, not 0 or 1", x_f64);
  ES_CHECK_ARG(km_shape_ok(ld, rows, cols, K),
               "kmeans_plusplus: rows=%d cols=%d ld=%lld K=%d outside 1 <= rows <= %d, 1 <= cols <= %d, cols <= ld, "
               "1 <= K <= min(%d, rows)", rows, cols, (long long)ld, K, KM_MAX_ROWS, KM_MAX_COLS, KM_MAX_K);
  ES_CHECK_ARG(trials >= 1 && trials <= KM_MAX_TRIALS, "kmeans_plusplus: trials = %d outside 1 .. %d", trials,
               KM_MAX_TRIALS);
  const size_t need = es_kmeans_plusplus_workspace(rows, cols, K);
  ES_CHECK_ARG(work && work_bytes >= need, "kmeans_plusplus: workspace of %zu bytes, %zu needed", work_bytes, need);
  const PpWork w = pp_work(work, rows, cols);
  const hipStream_t st = (hipStream_t)stream;
  const int nsel = ((rows > cols ? rows : cols) + 255) / 256;
  for (int step = 0; step < K; ++step) {
    const int T = step == 0 ? 1 : trials;
    hipLaunchKernelGGL(kmeans_pp_draw_kernel, dim3(1), dim3(1024), 0, st, w.closest, rows, u + (int64_t)step * trials,
                       T, step, w.cand);
    if (x_f64)
      hipLaunchKernelGGL(kmeans_pp_gather_kernel<double>, dim3(T), dim3(256), 0, st, (const double*)x, ld, rows, cols,
                         w.cand, w.cc);
    else
      hipLaunchKernelGGL(kmeans_pp_gather_kernel<float>, dim3(T), dim3(256), 0, st, (const float*)x, ld, rows, cols,
                         w.cand, w.cc);
    km_launch_dist<true>(x, x_f64, ld, rows, cols, w.cc, T, nullptr, nullptr, step == 0 ? nullptr : w.closest,
                         w.cdist, st);
    km_launch_reduce(w.cdist, rows, T, w.red, w.pot, nullptr, nullptr, nullptr, nullptr, st);
    hipLaunchKernelGGL(kmeans_pp_select_kernel, dim3(nsel), dim3(256), 0, st, w.pot, T, rows, cols, step, w.cand,
                       w.cc, w.cdist, w.closest, centres, index);
  }
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_confusion_matrix(const int32_t* pred, const int32_t* target, int64_t n, int n_true, int n_pred,
                                   int64_t* counts, int64_t* invalid, es_stream_t stream) {
  ES_CHECK_ARG(counts && invalid, "confusion_matrix: null output");
  ES_CHECK_ARG(n >= 0 && (n == 0 || (pred && target)), "confusion_matrix: n = %lld or null input", (long long)n);
  ES_CHECK_ARG(n_true >= 1 && n_pred >= 1 && (int64_t)n_true * n_pred <= CM_MAX_CELLS,
               "confusion_matrix: %d x %d outside 1 <= n_true * n_pred <= %d", n_true, n_pred, CM_MAX_CELLS);
  const hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(counts, 0, (size_t)n_true * n_pred * sizeof(int64_t), st);   // a failure shows below
  (void)hipMemsetAsync(invalid, 0, sizeof(int64_t), st);
  if (n > 0) {
    int64_t grid = (n + 256 * 8 - 1) / (256 * 8);     // a workgroup counts at most n: no int32 cell overflows
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)grid), dim3(256), 0, st, pred, target, n, n_true, n_pred,
                       (unsigned long long*)counts, (unsigned long long*)invalid);
  }
  ES_CHECK_LAUNCH();
  return ES_OK;
}
