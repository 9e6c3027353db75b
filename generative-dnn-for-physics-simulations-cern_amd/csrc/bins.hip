// Rows to condition bins on the device, and the rows grouped by class (include/expertsim_hip.h, es_bin_dispatch):
// bin(x) = the number of edges strictly below x (quantile_rule.h's bin_of, np.searchsorted side="left"), class = bin
// or expert * n_bins + bin, perm / offs in es_router_dispatch's layout.  The answer is np.argsort(class,
// kind="stable") and the cumulative counts: it is unique, and nothing here depends on the order in which anything
// lands -- there is no atomic at all.
//
// Three launches over chunks of BD_CHUNK = 1024 consecutive rows:
//   1. bd_rank_kernel, one workgroup per chunk: every row's class, then a bitonic sort in LDS of the 1024 keys
//      (class << 10 | local row); the keys are distinct, so the sorted order IS the stable grouping of the chunk.  A
//      run of equal classes starts at the first position of its class: a row's rank inside its class in its chunk is
//      its sorted position minus that start.  Out go the chunk's class counts, counts[class][chunk], and per sorted
//      position the packed (class, rank, local row).
//   2. bd_scan_kernel, one workgroup: the exclusive prefix sum of counts in (class, chunk) order, in place; offs.
//   3. bd_scatter_kernel: perm[base[class][chunk] + rank] = row.
#include "common.h"
#include "quantile_rule.h"
#include "segment.h"

namespace {

constexpr int BD_CHUNK = 1024, BD_THREADS = 1024;
constexpr int BD_MAX_CLASSES = 1024, BD_MAX_ROWS = 1 << 20;
constexpr uint32_t BD_PAD = 0xFFFFFFFFu;                 // above every key (class < 2^10, local row < 2^10)

struct BdArgs {
  const void* x; int x_f64; int64_t ld; int rows;
  const double* edges; int n_bins;
  const int32_t* expert; int n_experts;
  int n_classes, n_chunks;
};

__global__ void __launch_bounds__(BD_THREADS) bd_rank_kernel(BdArgs a, int32_t* __restrict__ bin,
                                                             int32_t* __restrict__ counts,
                                                             uint32_t* __restrict__ packed) {
  __shared__ double sedge[ES_BINS_MAX];
  __shared__ uint32_t sk[BD_CHUNK];
  __shared__ int sstart[BD_MAX_CLASSES], scnt[BD_MAX_CLASSES];
  const int t = threadIdx.x, chunk = blockIdx.x, row = chunk * BD_CHUNK + t;
  if (t < a.n_bins - 1) sedge[t] = a.edges[t];
  scnt[t] = 0;
  __syncthreads();
  uint32_t key = BD_PAD;
  if (row < a.rows) {
    const double x = a.x_f64 ? ((const double*)a.x)[(int64_t)row * a.ld] : (double)((const float*)a.x)[(int64_t)row * a.ld];
    const int b = bin_of(sedge, a.n_bins - 1, x);
    if (bin) bin[row] = b;
    const int cls = a.expert ? bin_class(b, a.n_bins, a.expert[row], a.n_experts) : b;
    key = ((uint32_t)cls << 10) | (uint32_t)t;
  }
  sk[t] = key;
  __syncthreads();
  for (int k = 2; k <= BD_CHUNK; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (t < BD_CHUNK / 2) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const uint32_t x = sk[i], y = sk[p];
        if ((x > y) == ((i & k) == 0)) { sk[i] = y; sk[p] = x; }      // distinct keys, except the padding
      }
      __syncthreads();
    }
  }
  key = sk[t];
  const bool live = key != BD_PAD;
  const int cls = (int)(key >> 10);
  if (live && (t == 0 || (int)(sk[t - 1] >> 10) != cls)) sstart[cls] = t;
  __syncthreads();
  uint32_t pk = BD_PAD;
  if (live) {
    const int rank = t - sstart[cls];
    pk = ((uint32_t)cls << 20) | ((uint32_t)rank << 10) | (key & 1023u);
    if (t == BD_CHUNK - 1 || sk[t + 1] == BD_PAD || (int)(sk[t + 1] >> 10) != cls) scnt[cls] = rank + 1;
  }
  packed[(int64_t)chunk * BD_CHUNK + t] = pk;
  __syncthreads();
  if (t < a.n_classes) counts[(int64_t)t * a.n_chunks + chunk] = scnt[t];
}

// exclusive prefix sum of counts [n_classes][n_chunks] in place; offs[c] = the base of (c, chunk 0), offs[n_classes]
// = the total.  Thread t owns the `per` consecutive entries from t * per.
__global__ void __launch_bounds__(BD_THREADS) bd_scan_kernel(int32_t* __restrict__ counts, int n_classes, int n_chunks,
                                                             int32_t* __restrict__ offs) {
  __shared__ int swave[BD_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int total = n_classes * n_chunks, per = (total + BD_THREADS - 1) / BD_THREADS;
  const int b = t * per < total ? t * per : total, e = b + per < total ? b + per : total;
  int sum = 0;
  for (int i = b; i < e; ++i) sum += counts[i];
  int inc = sum;                                           // inclusive scan over the lanes of the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) swave[wid] = inc;
  __syncthreads();
  int run = inc - sum, all = 0;
#pragma unroll
  for (int w = 0; w < BD_THREADS / 64; ++w) {
    const int cw = swave[w];
    run += w < wid ? cw : 0;
    all += cw;
  }
  for (int i = b; i < e; ++i) {
    const int c = counts[i];
    counts[i] = run;
    if (i % n_chunks == 0) offs[i / n_chunks] = run;
    run += c;
  }
  if (t == 0) offs[n_classes] = all;
}

__global__ void __launch_bounds__(BD_THREADS) bd_scatter_kernel(int rows, int n_chunks,
                                                                const int32_t* __restrict__ base,
                                                                const uint32_t* __restrict__ packed,
                                                                int32_t* __restrict__ perm) {
  const int chunk = blockIdx.x;
  const uint32_t pk = packed[(int64_t)chunk * BD_CHUNK + threadIdx.x];
  if (pk == BD_PAD) return;
  const int cls = (int)(pk >> 20), rank = (int)((pk >> 10) & 1023u), row = chunk * BD_CHUNK + (int)(pk & 1023u);
  const int dst = base[(int64_t)cls * n_chunks + chunk] + rank;
  if (dst >= 0 && dst < rows) perm[dst] = row;             // always true; a guard, not a rule
}

struct BdWork { int32_t* counts; uint32_t* packed; size_t bytes; };

inline BdWork bd_carve(void* work, int rows, int n_classes) {
  const int n_chunks = (rows + BD_CHUNK - 1) / BD_CHUNK;
  Carver c(work, 256);
  BdWork w;
  w.counts = c.take<int32_t>((size_t)n_classes * n_chunks);
  w.packed = c.take<uint32_t>((size_t)n_chunks * BD_CHUNK);
  w.bytes = c.bytes();
  return w;
}

inline bool bd_limits(int rows, int n_classes) {
  return rows >= 1 && rows <= BD_MAX_ROWS && n_classes >= 1 && n_classes <= BD_MAX_CLASSES;
}

}  // namespace

extern "C" size_t es_bin_dispatch_workspace(int rows, int n_classes) {
  return bd_limits(rows, n_classes) ? bd_carve(nullptr, rows, n_classes).bytes : 0;   // 0: outside the limits
}

extern "C" int es_bin_dispatch(const void* x, int x_f64, int64_t ld, int rows, const double* edges, int n_bins,
                               const int32_t* expert, int n_experts, int32_t* bin, int32_t* perm, int32_t* offs,
                               void* work, size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(x && perm && offs, "bin_dispatch: null argument");
  ES_CHECK_ARG(n_bins >= 1 && n_bins <= ES_BINS_MAX, "bin_dispatch: n_bins=%d outside 1 .. %d", n_bins, ES_BINS_MAX);
  ES_CHECK_ARG(edges || n_bins == 1, "bin_dispatch: %d bins without edges", n_bins);
  ES_CHECK_ARG(n_experts >= 1 && n_experts <= BD_MAX_CLASSES, "bin_dispatch: n_experts=%d", n_experts);
  ES_CHECK_ARG(expert || n_experts == 1, "bin_dispatch: n_experts=%d without an expert vector", n_experts);
  const int n_classes = n_bins * (expert ? n_experts : 1);
  ES_CHECK_ARG(n_classes <= BD_MAX_CLASSES, "bin_dispatch: %d classes above %d", n_classes, BD_MAX_CLASSES);
  ES_CHECK_ARG(rows >= 1 && rows <= BD_MAX_ROWS, "bin_dispatch: rows=%d outside 1 .. %d", rows, BD_MAX_ROWS);
  ES_CHECK_ARG(ld >= 1, "bin_dispatch: ld=%lld", (long long)ld);
  const size_t need = es_bin_dispatch_workspace(rows, n_classes);
  ES_CHECK_ARG(work && work_bytes >= need, "bin_dispatch: workspace of %zu bytes, %zu needed", work_bytes, need);
  const BdWork w = bd_carve(work, rows, n_classes);
  const int n_chunks = (rows + BD_CHUNK - 1) / BD_CHUNK;
  const BdArgs a = {x, x_f64, ld, rows, edges, n_bins, expert, n_experts, n_classes, n_chunks};
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bd_rank_kernel, dim3(n_chunks), dim3(BD_THREADS), 0, st, a, bin, w.counts, w.packed);
  hipLaunchKernelGGL(bd_scan_kernel, dim3(1), dim3(BD_THREADS), 0, st, w.counts, n_classes, n_chunks, offs);
  hipLaunchKernelGGL(bd_scatter_kernel, dim3(n_chunks), dim3(BD_THREADS), 0, st, rows, n_chunks, w.counts, w.packed,
                     perm);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
