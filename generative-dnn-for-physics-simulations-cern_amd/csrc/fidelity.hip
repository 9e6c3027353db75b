// Sample-level fidelity and diversity on the device: the k-nearest-neighbour radii and the counts behind
// precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020, the `prdc` package).
// include/expertsim_hip.h defines every entry to the letter; this header says how the work is laid out.
//
// Both entries walk all pairs (row p of side A, row q of side B) of a segment and never store a distance.  A
// 256-thread workgroup owns FD_TILE = 128 rows of A and a run of 128-row tiles of B (the B tiles of a segment
// are cut into `split` runs so that a small problem still fills the chip).  Thread (ty, tx) of the 16 x 16
// holds an 8 x 8 micro-tile of pairs in 64 fp64 accumulators: A rows ty * 4 + (i & 3) + 64 * (i >> 2), B rows
// tx * 4 + (j & 3) + 64 * (j >> 2).  The columns come in chunks of FD_KC = 16: fp32, staged column-major in LDS
// (two buffers, the next chunk's global loads issued before the current chunk's arithmetic, one barrier per
// chunk) and widened on load.  Per column a thread reads four 16-byte LDS words and issues 64 x (sub, mul, add)
// in fp64, so one pair's sum is walked by one thread in column order; columns past `cols` are staged as 0 on
// both sides and add +0.0.  Contraction is off: there is no FMA.
//
// es_knn_radius (A = B): per A row a sorted list of the k + 1 smallest distances lives in LDS, owned by the
// lane with tx == 0 of the 16 lanes that share the row.  After a tile the candidates below the row's current
// (k+1)-th value (a ballot says whether the wave has any) are handed to the owner by shuffles and inserted.
// With split > 1 every run writes its list to the workspace and a second launch merges the lists the same way.
//
// es_prdc_count (A = real, B = generated): per tile the row minima and hits are reduced over the 16 lanes of a
// row by shuffles into the owner's LDS slot and the column counts over the four row groups of a wave; they reach
// the workspace by integer atomics (add, or, and an unsigned min on the bit pattern of the non-negative
// distance), so no order matters.  A last launch per segment copies the per-row results out and adds the totals
// in integers.
#include <math.h>

#include "common.h"
#include "segment.h"

namespace {

constexpr int FD_TILE = 128;                // rows of either side in a workgroup's tile
constexpr int FD_THREADS = 256;             // 16 x 16 threads of 8 x 8 pairs
constexpr int FD_KC = 16;                   // columns of a staged chunk
constexpr int FD_LD = FD_TILE + 4;          // floats of a staged column: rows stay 16-byte aligned
constexpr int FD_SIDE = FD_KC * FD_LD;      // floats of one side of one buffer
constexpr int FD_MAX_K = ES_KNN_MAX_K;
constexpr int FD_KK = FD_MAX_K + 1;
constexpr int FD_MAX_ROWS = ES_KNN_MAX_ROWS;
constexpr int FD_MAX_COLS = ES_KNN_MAX_COLS;
constexpr int FD_MAX_SEG = ES_KNN_MAX_SEG;
constexpr int FD_MAX_SPLIT = 16;            // runs of B tiles per (segment, A tile)
constexpr int FD_TARGET_WG = 512;           // workgroups per segment the split aims at

struct FdSide {
  const float* x; int64_t ld; int rows; const int32_t* idx; const int32_t* seg; int cap;
};

struct FdArgs {
  FdSide a, b;
  int cols, k, split, per;                  // per: B tiles of one run
  double* radius2;                          // es_knn_radius: [n_seg][cap] (split == 1: written by the pair kernel)
  double* part;                             //   [n_seg][cap][split][k + 1]
  const double* a_rad;                      // es_prdc_count: [n_seg][a.cap], [n_seg][b.cap]
  const double* b_rad;
  int32_t* cnt;                             //   [n_seg][b.cap]
  int32_t* hit;                             //   [n_seg][a.cap]
  unsigned long long* mn;                   //   [n_seg][a.cap], the bits of a non-negative double
};

__device__ __forceinline__ SegSpan fd_seg(const FdSide& sd, int s) { return seg_span(sd.seg, s, sd.rows, sd.cap); }
// element offset of member i of the segment (n >= 1); a member past the end reads the last one's row
__device__ __forceinline__ int64_t fd_off(const FdSide& sd, SegSpan sg, int i) {
  return (int64_t)seg_row(sd.idx, sg.b + (i < sg.n ? i : sg.n - 1), sd.rows) * sd.ld;
}

// sorted insertion of c < col[k] into the k + 1 ascending values col[0], col[FD_TILE], ..
__device__ __forceinline__ void fd_insert(double* col, int k, double c) {
  int s = k;
  while (s > 0 && col[(s - 1) * FD_TILE] > c) {
    col[s * FD_TILE] = col[(s - 1) * FD_TILE];
    --s;
  }
  col[s * FD_TILE] = c;
}

__device__ __forceinline__ double fd_min(double a, double b) { return b < a ? b : a; }

// ------------------------------------------------------------------------------------------ the pair walk
template <bool COUNT>
__global__ void __launch_bounds__(FD_THREADS, 2) fd_pair_kernel(FdArgs g) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float st[2 * 2 * FD_SIDE];   // [buffer][side][column][row]
  __shared__ int64_t offA[FD_TILE];
  __shared__ int64_t offB[FD_TILE];
  // radius: the lists [slot][row].  count: [0] the A radii (-inf past the end), [1] the running minima,
  // [2] the B radii of the current tile (-inf past the end)
  __shared__ double rowv[FD_KK * FD_TILE];
  __shared__ int rowh[FD_TILE];             // count: the running hits

  const int t = threadIdx.x, lane = t & 63, tx = t & 15, ty = t >> 4, grp = lane & 48;
  const int s = blockIdx.z, chunk = blockIdx.y, p0 = blockIdx.x * FD_TILE;
  const SegSpan sa = fd_seg(g.a, s), sb = fd_seg(g.b, s);
  if (p0 >= sa.n) return;                   // block-uniform: a tile past the live length
  const int k = g.k;

  if (t < FD_TILE) {
    offA[t] = fd_off(g.a, sa, p0 + t);
    if (COUNT) {
      rowv[t] = p0 + t < sa.n ? g.a_rad[(int64_t)s * g.a.cap + p0 + t] : -INFINITY;
      rowv[FD_TILE + t] = INFINITY;
      rowh[t] = 0;
    } else {
      for (int slot = 0; slot <= k; ++slot) rowv[slot * FD_TILE + t] = INFINITY;
    }
  }

  const int nq = (sb.n + FD_TILE - 1) / FD_TILE;
  const int t_lo = chunk * g.per, t_hi = t_lo + g.per < nq ? t_lo + g.per : nq;
  const int sc = t & 15, sr = t >> 4;       // staging: column of the chunk, first row (then every 16th)
  const int nch = (g.cols + FD_KC - 1) / FD_KC;

  for (int qt = t_lo; qt < t_hi; ++qt) {
    const int q0 = qt * FD_TILE;
    if (t < FD_TILE) {
      offB[t] = fd_off(g.b, sb, q0 + t);
      if (COUNT) rowv[2 * FD_TILE + t] = q0 + t < sb.n ? g.b_rad[(int64_t)s * g.b.cap + q0 + t] : -INFINITY;
    }
    __syncthreads();                        // offA / offB / rowv are in place; the last tile's reads are done

    double acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = 0.0;

    float pa[8], pb[8];
    {                                       // chunk 0 into buffer 0
      const bool ok = sc < g.cols;
      const int c = ok ? sc : g.cols - 1;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const float va = g.a.x[offA[sr + 16 * m] + c], vb = g.b.x[offB[sr + 16 * m] + c];
        st[sc * FD_LD + sr + 16 * m] = ok ? va : 0.f;
        st[FD_SIDE + sc * FD_LD + sr + 16 * m] = ok ? vb : 0.f;
      }
    }
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
      const bool more = ch + 1 < nch;       // block-uniform
      if (more) {
        const int cn = (ch + 1) * FD_KC + sc;
        const bool ok = cn < g.cols;
        const int c = ok ? cn : g.cols - 1;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const float va = g.a.x[offA[sr + 16 * m] + c], vb = g.b.x[offB[sr + 16 * m] + c];
          pa[m] = ok ? va : 0.f;
          pb[m] = ok ? vb : 0.f;
        }
      }
      const float* sA = st + (ch & 1) * 2 * FD_SIDE;
      const float* sB = sA + FD_SIDE;
#pragma unroll 2
      for (int cc = 0; cc < FD_KC; ++cc) {
        const f32x4 a0 = *(const f32x4*)(sA + cc * FD_LD + ty * 4);
        const f32x4 a1 = *(const f32x4*)(sA + cc * FD_LD + 64 + ty * 4);
        const f32x4 b0 = *(const f32x4*)(sB + cc * FD_LD + tx * 4);
        const f32x4 b1 = *(const f32x4*)(sB + cc * FD_LD + 64 + tx * 4);
        const double a[8] = {(double)a0[0], (double)a0[1], (double)a0[2], (double)a0[3],
                             (double)a1[0], (double)a1[1], (double)a1[2], (double)a1[3]};
        const double b[8] = {(double)b0[0], (double)b0[1], (double)b0[2], (double)b0[3],
                             (double)b1[0], (double)b1[1], (double)b1[2], (double)b1[3]};
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const double d = a[i] - b[j];
            const double q = d * d;
            acc[i][j] = acc[i][j] + q;
          }
      }
      if (more) {
        float* dA = st + ((ch + 1) & 1) * 2 * FD_SIDE;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          dA[sc * FD_LD + sr + 16 * m] = pa[m];
          dA[FD_SIDE + sc * FD_LD + sr + 16 * m] = pb[m];
        }
      }
      __syncthreads();
    }

    // ---- the tile's 8 x 8 distances of this thread are complete
    if (COUNT) {
      int fc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) fc[j] = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int pr = ty * 4 + (i & 3) + 64 * (i >> 2);
        const double ra = rowv[pr];         // -inf for a row past the end: nothing is below it
        double m = INFINITY;
        int h = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int qc = tx * 4 + (j & 3) + 64 * (j >> 2);
          const double d = acc[i][j];
          if (q0 + qc < sb.n) m = fd_min(m, d);
          h |= d < rowv[2 * FD_TILE + qc] ? 1 : 0;
          fc[j] += d < ra ? 1 : 0;
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          m = fd_min(m, __shfl_xor(m, o, 64));
          h |= __shfl_xor(h, o, 64);
        }
        if (tx == 0) {                      // the row's owner: nobody else touches these slots
          rowv[FD_TILE + pr] = fd_min(rowv[FD_TILE + pr], m);
          rowh[pr] |= h;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int c = fc[j];
        c += __shfl_xor(c, 16, 64);
        c += __shfl_xor(c, 32, 64);
        const int qc = tx * 4 + (j & 3) + 64 * (j >> 2);
        if (lane < 16 && c != 0 && q0 + qc < sb.n) atomicAdd(g.cnt + (int64_t)s * g.b.cap + q0 + qc, c);
      }
      __syncthreads();                      // the next tile replaces the B radii
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int pr = ty * 4 + (i & 3) + 64 * (i >> 2);
        const bool p_live = p0 + pr < sa.n;
        double* col = rowv + pr;
        double thr = col[k * FD_TILE];      // the owner's copy is the one that counts
        thr = __shfl(thr, grp, 64);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int qc = tx * 4 + (j & 3) + 64 * (j >> 2);
          const bool pass = p_live && q0 + qc < sb.n && acc[i][j] < thr;
          if (__ballot(pass) != 0ull) {     // wave-uniform
            const double v = pass ? acc[i][j] : INFINITY;
            for (int l = 0; l < 16; ++l) {
              const double c = __shfl(v, grp + l, 64);
              if (tx == 0 && c < thr) {
                fd_insert(col, k, c);
                thr = col[k * FD_TILE];
              }
            }
            thr = __shfl(thr, grp, 64);
          }
        }
      }
    }
  }

  __syncthreads();                          // the owners' slots are final
  if (t < FD_TILE && p0 + t < sa.n) {
    const int64_t row = (int64_t)s * g.a.cap + p0 + t;
    if (COUNT) {
      const unsigned long long bits = (unsigned long long)__double_as_longlong(rowv[FD_TILE + t]);
      atomicMin(g.mn + row, bits);          // non-negative doubles order as their bit patterns
      if (rowh[t]) atomicOr(g.hit + row, 1);
    } else if (g.split == 1) {
      g.radius2[row] = rowv[k * FD_TILE + t];
    } else {
      double* out = g.part + (row * g.split + chunk) * (k + 1);
      for (int slot = 0; slot <= k; ++slot) out[slot] = rowv[slot * FD_TILE + t];
    }
  }
}

// radius2[s][p] = the (k+1)-th smallest of the row's `split` lists
__global__ void __launch_bounds__(FD_TILE) fd_merge_kernel(FdArgs g) {
  __shared__ double lst[FD_KK * FD_TILE];
  const int t = threadIdx.x, s = blockIdx.y, p = blockIdx.x * FD_TILE + t, k = g.k;
  const SegSpan sa = fd_seg(g.a, s);
  if (p >= sa.n) return;
  double* col = lst + t;                    // a thread owns its column: no barrier
  for (int slot = 0; slot <= k; ++slot) col[slot * FD_TILE] = INFINITY;
  const int64_t row = (int64_t)s * g.a.cap + p;
  const double* in = g.part + row * g.split * (k + 1);
  for (int i = 0; i < g.split * (k + 1); ++i) {
    const double c = in[i];
    if (c < col[k * FD_TILE]) fd_insert(col, k, c);
  }
  g.radius2[row] = col[k * FD_TILE];
}

__global__ void __launch_bounds__(256) fd_fill_kernel(unsigned long long* p, int64_t n, unsigned long long v) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = v;
}

// per segment: the per-row results leave the workspace (live entries only) and the totals are added
__global__ void __launch_bounds__(1024) fd_totals_kernel(FdArgs g, int32_t* __restrict__ f_count,
                                                        int32_t* __restrict__ r_hit, double* __restrict__ r_min2,
                                                        int64_t* __restrict__ totals) {
  __shared__ unsigned long long sum[4];
  const int s = blockIdx.x, t = threadIdx.x;
  const SegSpan sa = fd_seg(g.a, s), sb = fd_seg(g.b, s);
  if (t < 4) sum[t] = 0ull;
  __syncthreads();
  unsigned long long prec = 0, rec = 0, dens = 0, cov = 0;
  for (int q = t; q < sb.n; q += 1024) {
    const int64_t e = (int64_t)s * g.b.cap + q;
    const int c = g.cnt[e];
    if (f_count) f_count[e] = c;
    prec += c > 0 ? 1 : 0;
    dens += (unsigned long long)c;
  }
  for (int p = t; p < sa.n; p += 1024) {
    const int64_t e = (int64_t)s * g.a.cap + p;
    const int h = g.hit[e];
    const double m = __longlong_as_double((long long)g.mn[e]);
    if (r_hit) r_hit[e] = h;
    if (r_min2) r_min2[e] = m;
    rec += h ? 1 : 0;
    cov += m < g.a_rad[e] ? 1 : 0;
  }
  if (prec) atomicAdd(&sum[0], prec);       // integers: the order does not matter
  if (rec) atomicAdd(&sum[1], rec);
  if (dens) atomicAdd(&sum[2], dens);
  if (cov) atomicAdd(&sum[3], cov);
  __syncthreads();
  if (t == 0) {
    const bool valid = sa.n > g.k && sb.n > g.k;
    int64_t* o = totals + (int64_t)s * 8;
    o[0] = sa.n;
    o[1] = sb.n;
    o[2] = valid ? 1 : 0;
    o[3] = valid ? (int64_t)sum[0] : 0;
    o[4] = valid ? (int64_t)sum[1] : 0;
    o[5] = valid ? (int64_t)sum[2] : 0;
    o[6] = valid ? (int64_t)sum[3] : 0;
    o[7] = 0;
  }
}

// ------------------------------------------------------------------------------------------ host side
int fd_tiles(int cap) { return (cap + FD_TILE - 1) / FD_TILE; }
// runs of B tiles: enough workgroups per segment to fill the chip, at most one run per tile
int fd_split(int a_cap, int b_cap) {
  int sp = FD_TARGET_WG / fd_tiles(a_cap);
  const int tb = fd_tiles(b_cap);
  sp = sp < FD_MAX_SPLIT ? sp : FD_MAX_SPLIT;
  sp = sp < tb ? sp : tb;
  return sp > 1 ? sp : 1;
}
constexpr size_t FD_ALIGN = 16;
bool fd_side_ok(int rows, int cap, int n_seg) {
  return rows >= 1 && rows <= FD_MAX_ROWS && cap >= 1 && cap <= FD_MAX_ROWS && n_seg >= 1 && n_seg <= FD_MAX_SEG;
}

// es_knn_radius: the runs' lists [n_seg][cap][split][k + 1]; with one run there is nothing to merge and one
// double stands in, so the size is never 0 inside the limits
double* knn_lists(Carver& c, int n_seg, int cap, int k) {
  const int split = fd_split(cap, cap);
  return c.take<double>(split == 1 ? 1 : (size_t)n_seg * cap * split * (k + 1));
}

struct PrdcWork {
  unsigned long long* mn;  // [n_seg][r_cap]
  int32_t* hit;            // [n_seg][r_cap]
  int32_t* cnt;            // [n_seg][f_cap]
  size_t bytes;
};
PrdcWork prdc_work(void* base, int n_seg, int r_cap, int f_cap) {
  Carver c(base, FD_ALIGN);
  PrdcWork w;
  w.mn = c.take<unsigned long long>((size_t)n_seg * r_cap);
  w.hit = c.take<int32_t>((size_t)n_seg * r_cap);
  w.cnt = c.take<int32_t>((size_t)n_seg * f_cap);
  w.bytes = c.bytes();
  return w;
}

}  // namespace

extern "C" size_t es_knn_radius_workspace(int n_seg, int cap, int k) {
  if (!fd_side_ok(1, cap, n_seg) || k < 1 || k > FD_MAX_K) return 0;
  Carver c(nullptr, FD_ALIGN);
  knn_lists(c, n_seg, cap, k);
  return c.bytes();
}

extern "C" size_t es_prdc_workspace(int n_seg, int r_cap, int f_cap) {
  if (!fd_side_ok(1, r_cap, n_seg) || !fd_side_ok(1, f_cap, n_seg)) return 0;
  return prdc_work(nullptr, n_seg, r_cap, f_cap).bytes;
}

extern "C" int es_knn_radius(const float* x, int64_t ld, int rows, int cols, const int32_t* idx, const int32_t* seg,
                             int n_seg, int cap, int k, double* radius2, void* work, size_t work_bytes,
                             es_stream_t stream) {
  ES_CHECK_ARG(x && seg && radius2, "knn_radius: null argument");
  ES_CHECK_ARG(cols >= 1 && cols <= FD_MAX_COLS && ld >= cols, "knn_radius: cols=%d ld=%lld outside 1 <= cols <= %d, "
               "cols <= ld", cols, (long long)ld, FD_MAX_COLS);
  ES_CHECK_ARG(fd_side_ok(rows, cap, n_seg), "knn_radius: rows=%d cap=%d n_seg=%d outside 1 <= rows, cap <= %d, "
               "1 <= n_seg <= %d", rows, cap, n_seg, FD_MAX_ROWS, FD_MAX_SEG);
  ES_CHECK_ARG(k >= 1 && k <= FD_MAX_K, "knn_radius: k = %d outside 1 .. %d", k, FD_MAX_K);
  const size_t need = es_knn_radius_workspace(n_seg, cap, k);
  ES_CHECK_ARG(work && work_bytes >= need, "knn_radius: workspace of %zu bytes, %zu needed", work_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  FdArgs g = {};
  g.a = {x, ld, rows, idx, seg, cap};
  g.b = g.a;
  g.cols = cols;
  g.k = k;
  g.split = fd_split(cap, cap);
  g.per = (fd_tiles(cap) + g.split - 1) / g.split;
  g.radius2 = radius2;
  Carver c(work, FD_ALIGN);
  g.part = knn_lists(c, n_seg, cap, k);
  hipLaunchKernelGGL(fd_pair_kernel<false>, dim3(fd_tiles(cap), g.split, n_seg), dim3(FD_THREADS), 0, st, g);
  if (g.split > 1) hipLaunchKernelGGL(fd_merge_kernel, dim3(fd_tiles(cap), n_seg), dim3(FD_TILE), 0, st, g);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_prdc_count(const float* real, int64_t r_ld, int r_rows, const int32_t* r_idx, const int32_t* r_seg,
                             int r_cap, const float* fake, int64_t f_ld, int f_rows, const int32_t* f_idx,
                             const int32_t* f_seg, int f_cap, int cols, int n_seg, int k, const double* r_radius2,
                             const double* f_radius2, int32_t* f_count, int32_t* r_hit, double* r_min2,
                             int64_t* totals, void* work, size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(real && fake && r_seg && f_seg && r_radius2 && f_radius2 && totals, "prdc_count: null argument");
  ES_CHECK_ARG(cols >= 1 && cols <= FD_MAX_COLS && r_ld >= cols && f_ld >= cols,
               "prdc_count: cols=%d r_ld=%lld f_ld=%lld outside 1 <= cols <= %d, cols <= ld", cols, (long long)r_ld,
               (long long)f_ld, FD_MAX_COLS);
  ES_CHECK_ARG(fd_side_ok(r_rows, r_cap, n_seg) && fd_side_ok(f_rows, f_cap, n_seg),
               "prdc_count: r_rows=%d r_cap=%d f_rows=%d f_cap=%d n_seg=%d outside 1 <= rows, cap <= %d, "
               "1 <= n_seg <= %d", r_rows, r_cap, f_rows, f_cap, n_seg, FD_MAX_ROWS, FD_MAX_SEG);
  ES_CHECK_ARG(k >= 1 && k <= FD_MAX_K, "prdc_count: k = %d outside 1 .. %d", k, FD_MAX_K);
  const size_t need = es_prdc_workspace(n_seg, r_cap, f_cap);
  ES_CHECK_ARG(work && work_bytes >= need, "prdc_count: workspace of %zu bytes, %zu needed", work_bytes, need);
  const PrdcWork w = prdc_work(work, n_seg, r_cap, f_cap);
  const hipStream_t st = (hipStream_t)stream;
  FdArgs g = {};
  g.a = {real, r_ld, r_rows, r_idx, r_seg, r_cap};
  g.b = {fake, f_ld, f_rows, f_idx, f_seg, f_cap};
  g.cols = cols;
  g.k = k;
  g.split = fd_split(r_cap, f_cap);
  g.per = (fd_tiles(f_cap) + g.split - 1) / g.split;
  g.a_rad = r_radius2;
  g.b_rad = f_radius2;
  g.cnt = w.cnt;
  g.hit = w.hit;
  g.mn = w.mn;
  // hit and cnt are adjacent in the workspace: one memset zeroes both (a failure shows below)
  (void)hipMemsetAsync(w.hit, 0, (size_t)((char*)work + w.bytes - (char*)w.hit), st);
  const int64_t n_min = (int64_t)n_seg * r_cap;
  const int64_t fill_grid = (n_min + 256 * 8 - 1) / (256 * 8);
  hipLaunchKernelGGL(fd_fill_kernel, dim3((unsigned)(fill_grid < 1024 ? fill_grid : 1024)), dim3(256), 0, st, w.mn,
                     n_min, 0x7FF0000000000000ull);
  hipLaunchKernelGGL(fd_pair_kernel<true>, dim3(fd_tiles(r_cap), g.split, n_seg), dim3(FD_THREADS), 0, st, g);
  hipLaunchKernelGGL(fd_totals_kernel, dim3(n_seg), dim3(1024), 0, st, g, f_count, r_hit, r_min2, totals);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
