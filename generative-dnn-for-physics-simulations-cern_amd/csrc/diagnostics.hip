// Expert diagnostics on the device: the numbers behind the reference's specialisation plots.
// include/expertsim_hip.h has the definitions; this file has the kernels.
//
// Shared.  x [rows][ld] fp32 / fp64, segment s = the rows idx[seg[2s] .. seg[2s+1]) (clamped).
//   diag_range_kernel     min / max of every column over all rows.  A thread keeps one column (thread t reads
//                         element t of a pass of 256 / cols whole rows: contiguous across the wave when
//                         ld == cols) and holds its min / max in registers; one 64-bit integer min / max
//                         atomic per thread on LDS, then one per (workgroup, column) on global memory, on
//                         the order-preserving key of the double.  Exact, order-independent.
//   diag_linspace_kernel  np.linspace's arithmetic on the decoded range: the histogram's edges, the KDE's grid.
//
// es_segment_histogram: diag_hist_kernel, one workgroup per (tile of rows, segment).  The tile's rows come in
// with all their columns (element i of the tile = row i / cols, column i % cols: coalesced when ld == cols)
// and are parked in LDS as doubles with an odd row pitch; then a wave takes 64 rows of ONE column, so the
// column's edges and histogram are wave-uniform.  The bin is a binary search over the column's edges in LDS
// (the definition itself, no estimate to correct).  Contention: the categorical columns (mass, charge: at
// most three values) put whole waves on one bin, so a wave first peels off up to DIAG_PEEL distinct bins --
// the first pending lane's bin is broadcast, the lanes that share it are counted with a ballot and ONE lane
// adds the count -- and only the lanes still pending after that (continuous columns: spread over many bins)
// add 1 each.  LDS integer atomics (ds_add_u32); the tile's non-zero counts then go to global memory with
// global_atomic_add (vector atomics, integers: order-free, rerun bit-equal).
// LDS banks (computed from the bank rule, not measured): the parked tile is read with a lane stride of
// pitch doubles, pitch odd, so the 32 lanes of each ds_read_b64 group cover 32 distinct even banks and their
// odd neighbours: no conflict.  The binary search reads are lane-divergent addresses inside one column's
// edges; the first steps are broadcasts (all lanes read the same middle edges), the last ones spread.
//
// es_segment_kde: diag_moments_kernel (one workgroup per segment; thread (chunk k, column c) walks its
// members sequentially, es_group_diversity's order; the ES_PREP_CHUNKS partials are added in chunk order
// through LDS), diag_kde_kernel (one workgroup per (member chunk, column, segment): the chunk's
// ES_DIAG_KDE_CHUNK members are parked in LDS and read as broadcasts -- every lane reads the same address, one
// LDS cycle, no conflict by the bank rule -- while a lane owns grid points and sums its chunk sequentially
// from +0.0; the chunk sums go to the workspace) and diag_kde_close_kernel (per grid point the chunk sums in
// chunk order from +0.0, then the normalisation; NaN rows for invalid (segment, column) pairs).  No float
// atomics anywhere.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "segment.h"

namespace {

constexpr int DIAG_THREADS = 256;
constexpr int DIAG_MAX_ROWS = 1 << 20;
constexpr int DIAG_MAX_SEG = 65535;
constexpr int DIAG_STAGE = 2048;          // doubles of a parked tile: 16 KiB
constexpr int DIAG_PEEL = 3;              // distinct bins a wave aggregates before the per-lane adds
constexpr int DIAG_RANGE_BLOCKS = 256;
constexpr double DIAG_SQRT_2PI = 2.5066282746310002;

// rng[c] = min key, rng[ES_DIAG_MAX_COLS + c] = max key (initialised to all ones / zero on the stream)
template <typename T>
__global__ void __launch_bounds__(DIAG_THREADS) diag_range_kernel(const T* __restrict__ x, int64_t ld, int rows,
                                                                  int cols, unsigned long long* __restrict__ rng) {
  __shared__ unsigned long long sh[2 * ES_DIAG_MAX_COLS];
  const int tid = threadIdx.x;
  if (tid < ES_DIAG_MAX_COLS) {
    sh[tid] = ~0ull;
    sh[ES_DIAG_MAX_COLS + tid] = 0ull;
  }
  __syncthreads();
  const int rpp = DIAG_THREADS / cols;                // whole rows of one pass
  const int r0 = tid / cols, c = tid - r0 * cols;
  if (r0 < rpp) {
    unsigned long long lo = ~0ull, hi = 0ull;
    for (int64_t r = (int64_t)blockIdx.x * rpp + r0; r < rows; r += (int64_t)gridDim.x * rpp) {
      const unsigned long long k = f64_key((double)x[r * ld + c]);
      lo = k < lo ? k : lo;
      hi = k > hi ? k : hi;
    }
    if (hi != 0ull) {                                 // the thread has seen a row (no key is 0)
      atomicMin(&sh[c], lo);
      atomicMax(&sh[ES_DIAG_MAX_COLS + c], hi);
    }
  }
  __syncthreads();
  if (tid < cols && sh[ES_DIAG_MAX_COLS + tid] != 0ull) {
    atomicMin(&rng[tid], sh[tid]);
    atomicMax(&rng[ES_DIAG_MAX_COLS + tid], sh[ES_DIAG_MAX_COLS + tid]);
  }
}

// out[c][k] = np.linspace(lo_c, hi_c, num)[k]; widen != 0: lo == hi becomes lo - 1e-6, hi + 1e-6 first
__global__ void __launch_bounds__(DIAG_THREADS) diag_linspace_kernel(const unsigned long long* __restrict__ rng,
                                                                     int cols, int num, int widen,
                                                                     double* __restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * DIAG_THREADS + threadIdx.x;
  if (i >= cols * num) return;
  const int c = i / num, k = i - c * num;
  double lo = f64_unkey(rng[c]), hi = f64_unkey(rng[ES_DIAG_MAX_COLS + c]);
  if (widen && lo == hi) {
    lo = lo - 1e-6;
    hi = hi + 1e-6;
  }
  const int div = num - 1;
  double v = lo;
  if (div > 0) {
    const double delta = hi - lo, step = delta / (double)div;
    if (k == div) {
      v = hi;
    } else if (step != 0.0) {
      const double p = (double)k * step;
      v = p + lo;
    } else {
      const double q = (double)k / (double)div, p = q * delta;
      v = p + lo;
    }
  }
  out[i] = v;
}

template <typename T>
__global__ void __launch_bounds__(DIAG_THREADS) diag_hist_kernel(const T* __restrict__ x, int64_t ld, int rows,
                                                                 int cols, const int32_t* __restrict__ idx,
                                                                 const int32_t* __restrict__ seg, int seg_cap,
                                                                 int bins, int right,
                                                                 const double* __restrict__ edges, int tile_rows,
                                                                 int pitch, int32_t* __restrict__ counts,
                                                                 int32_t* __restrict__ outside) {
  extern __shared__ double diag_sh[];
  double* sh_e = diag_sh;                                       // [cols][bins + 1]
  double* sh_x = sh_e + cols * (bins + 1);                      // [tile_rows][pitch]
  int* sh_h = reinterpret_cast<int*>(sh_x + tile_rows * pitch); // [cols][bins]
  int* sh_o = sh_h + cols * bins;                               // [cols]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int s = blockIdx.y;
  const SegSpan sg = seg_span(seg, s, rows, seg_cap);
  const int p0 = blockIdx.x * tile_rows;
  if (p0 >= sg.n) return;                                       // block-uniform, before any barrier
  const int live = sg.n - p0 < tile_rows ? sg.n - p0 : tile_rows;
  for (int i = tid; i < cols * (bins + 1); i += DIAG_THREADS) sh_e[i] = edges[i];
  for (int i = tid; i < cols * bins + cols; i += DIAG_THREADS) sh_h[i] = 0;      // the histograms and sh_o
  for (int i = tid; i < live * cols; i += DIAG_THREADS) {
    const int r = i / cols, c = i - r * cols;
    const int row = seg_row(idx, sg.b + p0 + r, rows);
    sh_x[r * pitch + c] = (double)x[(int64_t)row * ld + c];
  }
  __syncthreads();
  const int nblk = (live + 63) >> 6;
  for (int u = wid; u < cols * nblk; u += DIAG_THREADS / 64) {  // wave-uniform
    const int c = u / nblk, r = (u - c * nblk) * 64 + lane;
    const bool ok = r < live;
    const double v = ok ? sh_x[r * pitch + c] : 0.0;
    const double* e = sh_e + c * (bins + 1);
    int lo = 0, hi = bins + 1;                                  // the edges <= v (right = 0) or < v (right = 1)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const double ev = e[mid];
      if (right ? ev < v : ev <= v) lo = mid + 1;
      else hi = mid;
    }
    int b = lo - 1;
    if (!right && b == bins && v == e[bins]) b = bins - 1;
    if (right && b < 0 && v == e[0]) b = 0;
    const bool out = b < 0 || b >= bins;
    const unsigned long long om = __ballot(ok && out);
    if (om != 0ull && lane == 0) atomicAdd(&sh_o[c], (int)__popcll(om));
    bool pending = ok && !out;
    int* h = sh_h + c * bins;
    for (int round = 0; round < DIAG_PEEL; ++round) {
      const unsigned long long act = __ballot(pending);
      if (act == 0ull) break;
      const int leader = __builtin_amdgcn_readfirstlane((int)__ffsll((long long)act) - 1);
      const int kb = __builtin_amdgcn_readlane(b, leader);
      const bool mine = pending && b == kb;
      const unsigned long long m = __ballot(mine);
      if (lane == leader) atomicAdd(&h[kb], (int)__popcll(m));
      pending = pending && !mine;
    }
    if (pending) atomicAdd(&h[b], 1);
  }
  __syncthreads();
  int32_t* gc = counts + (int64_t)s * cols * bins;
  for (int i = tid; i < cols * bins; i += DIAG_THREADS) {
    const int v = sh_h[i];
    if (v != 0) atomicAdd(&gc[i], v);
  }
  for (int i = tid; i < cols; i += DIAG_THREADS) {
    const int v = sh_o[i];
    if (v != 0) atomicAdd(&outside[(int64_t)s * cols + i], v);
  }
}

// per (segment, column): S, m, Q in es_group_diversity's order, then sd, bw, valid
template <typename T>
__global__ void __launch_bounds__(DIAG_THREADS) diag_moments_kernel(const T* __restrict__ x, int64_t ld, int rows,
                                                                    int cols, const int32_t* __restrict__ idx,
                                                                    const int32_t* __restrict__ seg, int seg_cap,
                                                                    int min_samples, double std_eps,
                                                                    double* __restrict__ bw,
                                                                    int32_t* __restrict__ valid,
                                                                    double* __restrict__ sd_out) {
#pragma clang fp contract(off)
  __shared__ double part[ES_PREP_CHUNKS][ES_DIAG_MAX_COLS];
  __shared__ double mean[ES_DIAG_MAX_COLS];
  const int tid = threadIdx.x, s = blockIdx.x;
  const SegSpan sg = seg_span(seg, s, rows, seg_cap);
  const int n = sg.n;
  const int L = n <= ES_PREP_SPLIT_MIN ? n : (n + ES_PREP_CHUNKS - 1) / ES_PREP_CHUNKS;
  const double dn = (double)n;
  for (int pass = 0; pass < 2; ++pass) {
    for (int w = tid; w < ES_PREP_CHUNKS * cols; w += DIAG_THREADS) {
      const int k = w / cols, c = w - k * cols;
      const int64_t a = (int64_t)k * L, z = a + L;
      const int lo = a < n ? (int)a : n, hi = z < n ? (int)z : n;
      const double m = pass ? mean[c] : 0.0;
      double acc = 0.0;
      for (int p = lo; p < hi; ++p) {
        const double v = (double)x[(int64_t)seg_row(idx, sg.b + p, rows) * ld + c];
        if (pass) {
          const double d = v - m;
          const double q = d * d;
          acc += q;
        } else {
          acc += v;
        }
      }
      part[k][c] = acc;
    }
    __syncthreads();
    if (tid < cols) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < ES_PREP_CHUNKS; ++k) t += part[k][tid];
      if (pass == 0) {
        mean[tid] = n > 0 ? t / dn : 0.0;
      } else {
        const int need = min_samples > 2 ? min_samples : 2;
        bool ok = n >= need;
        double sd = 0.0, h = 0.0;
        if (ok) {
          ok = t > 0.0 && !(sqrt(t / dn) < std_eps);
          if (ok) {
            sd = sqrt(t / (dn - 1.0));
            h = sd * pow(dn, -0.2);
          }
        }
        bw[(int64_t)s * cols + tid] = h;
        valid[(int64_t)s * cols + tid] = ok ? 1 : 0;
        if (sd_out) sd_out[(int64_t)s * cols + tid] = sd;
      }
    }
    __syncthreads();
  }
}

// partial[s][c][ch][j] = sum over the members of chunk ch, in member order from +0.0, of exp(-z^2 / 2)
template <typename T>
__global__ void __launch_bounds__(DIAG_THREADS) diag_kde_kernel(const T* __restrict__ x, int64_t ld, int rows,
                                                                int cols, const int32_t* __restrict__ idx,
                                                                const int32_t* __restrict__ seg, int seg_cap,
                                                                int points, const double* __restrict__ grid,
                                                                const double* __restrict__ bw,
                                                                const int32_t* __restrict__ valid, int nchunks,
                                                                double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double mem[ES_DIAG_KDE_CHUNK];
  const int tid = threadIdx.x, ch = blockIdx.x, c = blockIdx.y, s = blockIdx.z;
  const SegSpan sg = seg_span(seg, s, rows, seg_cap);
  const int first = ch * ES_DIAG_KDE_CHUNK;
  if (first >= sg.n || valid[(int64_t)s * cols + c] == 0) return;   // block-uniform, before the barrier
  const int cnt = sg.n - first < ES_DIAG_KDE_CHUNK ? sg.n - first : ES_DIAG_KDE_CHUNK;
  for (int i = tid; i < cnt; i += blockDim.x)
    mem[i] = (double)x[(int64_t)seg_row(idx, sg.b + first + i, rows) * ld + c];
  __syncthreads();
  const double r = 1.0 / bw[(int64_t)s * cols + c];
  double* out = partial + (((int64_t)s * cols + c) * nchunks + ch) * points;
  for (int j = tid; j < points; j += blockDim.x) {
    const double g = grid[(int64_t)c * points + j];
    double acc = 0.0;
    for (int i = 0; i < cnt; ++i) {
      const double z = (g - mem[i]) * r;
      const double a = z * z;
      acc += exp(-0.5 * a);
    }
    out[j] = acc;
  }
}

__global__ void __launch_bounds__(DIAG_THREADS) diag_kde_close_kernel(const int32_t* __restrict__ seg, int rows,
                                                                      int seg_cap, int cols, int points,
                                                                      const double* __restrict__ bw,
                                                                      const int32_t* __restrict__ valid,
                                                                      int nchunks,
                                                                      const double* __restrict__ partial,
                                                                      double* __restrict__ density) {
#pragma clang fp contract(off)
  const int c = blockIdx.x, s = blockIdx.y;
  const SegSpan sg = seg_span(seg, s, rows, seg_cap);
  const int64_t sc = (int64_t)s * cols + c;
  const bool ok = valid[sc] != 0;
  const int used = (sg.n + ES_DIAG_KDE_CHUNK - 1) / ES_DIAG_KDE_CHUNK;
  const double norm = ((double)sg.n * bw[sc]) * DIAG_SQRT_2PI;
  for (int j = threadIdx.x; j < points; j += DIAG_THREADS) {
    double v = __longlong_as_double(0x7ff8000000000000ll);
    if (ok) {
      double t = 0.0;
      for (int ch = 0; ch < used; ++ch) t += partial[(sc * nchunks + ch) * points + j];
      v = t / norm;
    }
    density[sc * points + j] = v;
  }
}

bool diag_common_ok(int cols, int64_t ld, int rows, int n_seg, int seg_cap) {
  return cols >= 1 && cols <= ES_DIAG_MAX_COLS && ld >= cols && rows >= 0 && rows <= DIAG_MAX_ROWS && n_seg >= 0 &&
         n_seg <= DIAG_MAX_SEG && seg_cap >= 1;
}
bool diag_hist_ok(int cols, int bins) {
  return cols >= 1 && cols <= ES_DIAG_MAX_COLS && bins >= 1 &&
         (int64_t)cols * (2 * (int64_t)bins + 1) <= ES_DIAG_HIST_MAX_CELLS;
}
int diag_chunks(int seg_cap) { return (seg_cap + ES_DIAG_KDE_CHUNK - 1) / ES_DIAG_KDE_CHUNK; }

// Both workspaces start with the range keys [2][ES_DIAG_MAX_COLS] (ES_DIAG_RANGE_BYTES); the KDE's chunk sums
// [n_seg][cols][chunks][points] follow.  points == 0: the histogram's.
struct DiagWork {
  unsigned long long* rng;
  double* partial;
  size_t bytes;
};
static_assert(ES_DIAG_RANGE_BYTES == 2 * ES_DIAG_MAX_COLS * sizeof(unsigned long long), "the range keys");
DiagWork diag_work(void* base, int n_seg, int cols, int chunks, int points) {
  Carver c(base, sizeof(double));
  DiagWork w;
  w.rng = c.take<unsigned long long>(2 * ES_DIAG_MAX_COLS);
  w.partial = c.take<double>((size_t)n_seg * cols * chunks * points);
  w.bytes = c.bytes();
  return w;
}

// the range of every column into rng, then linspace(lo, hi, num) into out
void diag_range_linspace(const void* x, int x_f64, int64_t ld, int rows, int cols, int num, int widen,
                         unsigned long long* rng, double* out, hipStream_t st) {
  (void)hipMemsetAsync(rng, 0xff, ES_DIAG_MAX_COLS * sizeof(unsigned long long), st);
  (void)hipMemsetAsync(rng + ES_DIAG_MAX_COLS, 0, ES_DIAG_MAX_COLS * sizeof(unsigned long long), st);
  const int rpp = DIAG_THREADS / cols;
  const int want = (rows + rpp - 1) / rpp;
  const dim3 grid(want < DIAG_RANGE_BLOCKS ? want : DIAG_RANGE_BLOCKS), block(DIAG_THREADS);
  if (x_f64) hipLaunchKernelGGL(diag_range_kernel<double>, grid, block, 0, st, (const double*)x, ld, rows, cols, rng);
  else hipLaunchKernelGGL(diag_range_kernel<float>, grid, block, 0, st, (const float*)x, ld, rows, cols, rng);
  hipLaunchKernelGGL(diag_linspace_kernel, dim3((cols * num + DIAG_THREADS - 1) / DIAG_THREADS), block, 0, st, rng,
                     cols, num, widen, out);
}

}  // namespace

extern "C" size_t es_segment_histogram_workspace(int cols, int bins) {
  return diag_hist_ok(cols, bins) ? diag_work(nullptr, 0, 0, 0, 0).bytes : 0;
}

extern "C" int es_segment_histogram(const void* x, int x_f64, int64_t ld, int rows, int cols, const int32_t* idx,
                                    const int32_t* seg, int n_seg, int seg_cap, int bins, int right,
                                    const double* edges, double* edges_out, int32_t* counts, int32_t* outside,
                                    void* work, size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(x && seg && edges_out && counts && outside, "segment_histogram: null argument");
  ES_CHECK_ARG(x_f64 == 0 || x_f64 == 1, "segment_histogram: x_f64 = %d, not 0 or 1", x_f64);
  ES_CHECK_ARG(right == 0 || right == 1, "segment_histogram: right = %d, not 0 or 1", right);
  ES_CHECK_ARG(diag_common_ok(cols, ld, rows, n_seg, seg_cap),
               "segment_histogram: rows=%d cols=%d ld=%lld n_seg=%d seg_cap=%d outside the limits", rows, cols,
               (long long)ld, n_seg, seg_cap);
  ES_CHECK_ARG(diag_hist_ok(cols, bins), "segment_histogram: cols=%d bins=%d outside 1 <= bins, cols*(2*bins+1) <= %d",
               cols, bins, ES_DIAG_HIST_MAX_CELLS);
  if (rows == 0 || n_seg == 0) return ES_OK;
  ES_CHECK_ARG(edges || (work && work_bytes >= (size_t)ES_DIAG_RANGE_BYTES),
               "segment_histogram: workspace of %zu bytes, %d needed", work_bytes, ES_DIAG_RANGE_BYTES);
  const hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(counts, 0, (size_t)n_seg * cols * bins * sizeof(int32_t), st);
  (void)hipMemsetAsync(outside, 0, (size_t)n_seg * cols * sizeof(int32_t), st);
  if (edges) {
    if (edges != edges_out)
      (void)hipMemcpyAsync(edges_out, edges, (size_t)cols * (bins + 1) * sizeof(double), hipMemcpyDeviceToDevice, st);
  } else {
    diag_range_linspace(x, x_f64, ld, rows, cols, bins + 1, 0, diag_work(work, 0, 0, 0, 0).rng, edges_out, st);
  }
  const int pitch = cols | 1;
  const int fit = DIAG_STAGE / pitch;
  const int tile_rows = fit < DIAG_THREADS ? fit : DIAG_THREADS;
  const int cap = seg_cap < rows ? seg_cap : rows;
  const size_t lds = ((size_t)cols * (bins + 1) + (size_t)tile_rows * pitch) * sizeof(double) +
                     ((size_t)cols * bins + cols) * sizeof(int);
  const dim3 grid((cap + tile_rows - 1) / tile_rows, n_seg), block(DIAG_THREADS);
  if (x_f64)
    hipLaunchKernelGGL(diag_hist_kernel<double>, grid, block, lds, st, (const double*)x, ld, rows, cols, idx, seg, cap,
                       bins, right, edges_out, tile_rows, pitch, counts, outside);
  else
    hipLaunchKernelGGL(diag_hist_kernel<float>, grid, block, lds, st, (const float*)x, ld, rows, cols, idx, seg, cap,
                       bins, right, edges_out, tile_rows, pitch, counts, outside);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" size_t es_segment_kde_workspace(int n_seg, int cols, int points, int seg_cap) {
  if (n_seg <= 0 || n_seg > DIAG_MAX_SEG || cols < 1 || cols > ES_DIAG_MAX_COLS || points < 1 ||
      points > ES_DIAG_KDE_MAX_POINTS || seg_cap < 1)
    return 0;
  const int cap = seg_cap < DIAG_MAX_ROWS ? seg_cap : DIAG_MAX_ROWS;
  return diag_work(nullptr, n_seg, cols, diag_chunks(cap), points).bytes;
}

extern "C" int es_segment_kde(const void* x, int x_f64, int64_t ld, int rows, int cols, const int32_t* idx,
                              const int32_t* seg, int n_seg, int seg_cap, int points, const double* grid,
                              int min_samples, double std_eps, double* grid_out, double* density, double* bw,
                              int32_t* valid, double* sd, void* work, size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(x && seg && grid_out && density && bw && valid, "segment_kde: null argument");
  ES_CHECK_ARG(x_f64 == 0 || x_f64 == 1, "segment_kde: x_f64 = %d, not 0 or 1", x_f64);
  ES_CHECK_ARG(diag_common_ok(cols, ld, rows, n_seg, seg_cap),
               "segment_kde: rows=%d cols=%d ld=%lld n_seg=%d seg_cap=%d outside the limits", rows, cols, (long long)ld,
               n_seg, seg_cap);
  ES_CHECK_ARG(points >= 1 && points <= ES_DIAG_KDE_MAX_POINTS, "segment_kde: points=%d outside 1 .. %d", points,
               ES_DIAG_KDE_MAX_POINTS);
  ES_CHECK_ARG(min_samples >= 0 && std_eps == std_eps, "segment_kde: min_samples=%d std_eps=%g", min_samples, std_eps);
  if (rows == 0 || n_seg == 0) return ES_OK;
  const int cap = seg_cap < rows ? seg_cap : rows;
  const size_t need = es_segment_kde_workspace(n_seg, cols, points, cap);
  ES_CHECK_ARG(work && work_bytes >= need, "segment_kde: workspace of %zu bytes, %zu needed", work_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  const int nchunks = diag_chunks(cap);
  const DiagWork w = diag_work(work, n_seg, cols, nchunks, points);
  if (grid) {
    if (grid != grid_out)
      (void)hipMemcpyAsync(grid_out, grid, (size_t)cols * points * sizeof(double), hipMemcpyDeviceToDevice, st);
  } else {
    diag_range_linspace(x, x_f64, ld, rows, cols, points, 1, w.rng, grid_out, st);
  }
  const int lanes = points < DIAG_THREADS ? ((points + 63) / 64) * 64 : DIAG_THREADS;
  const dim3 gm(n_seg), gk(nchunks, cols, n_seg), gc(cols, n_seg), block(DIAG_THREADS), bk(lanes);
  if (x_f64) {
    hipLaunchKernelGGL(diag_moments_kernel<double>, gm, block, 0, st, (const double*)x, ld, rows, cols, idx, seg, cap,
                       min_samples, std_eps, bw, valid, sd);
    hipLaunchKernelGGL(diag_kde_kernel<double>, gk, bk, 0, st, (const double*)x, ld, rows, cols, idx, seg, cap, points,
                       grid_out, bw, valid, nchunks, w.partial);
  } else {
    hipLaunchKernelGGL(diag_moments_kernel<float>, gm, block, 0, st, (const float*)x, ld, rows, cols, idx, seg, cap,
                       min_samples, std_eps, bw, valid, sd);
    hipLaunchKernelGGL(diag_kde_kernel<float>, gk, bk, 0, st, (const float*)x, ld, rows, cols, idx, seg, cap, points,
                       grid_out, bw, valid, nchunks, w.partial);
  }
  hipLaunchKernelGGL(diag_kde_close_kernel, gc, block, 0, st, seg, rows, cap, cols, points, bw, valid, nchunks, w.partial,
                     density);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
