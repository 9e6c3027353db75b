// 1-D Wasserstein-1 distances on the device: the scipy.stats.wasserstein_distance
// calls of calculate_joint_ws_across_experts (train/utils.py:117-176), one per (segment, channel).
//
// Arithmetic: scipy's _cdf_distance with p = 1, term for term.  The nu + nv values of a problem are sorted
// together, each carrying a one-byte tag (1: from u); with a[k] the sorted values and cu[k] / cv[k] the
// counts of u / v values among a[0..k],
//     d = sum_{k=0}^{nu+nv-2} |cu[k] / nu - cv[k] / nv| * (a[k+1] - a[k])        (fp64 throughout).
// Inside a run of equal values the difference is exactly 0 and at its end the counts are complete, so
// ties need no stable sort.
//
// Sort: a bitonic network over order-preserving 64-bit keys (sign-flipped IEEE bits), padded with
// all-ones keys to the next power of two of the LIVE nu + nv (read on the device).  The padding keys sort
// to the end and the sum stops at nu + nv - 2, so none enters it.
//   nu_cap + nv_cap <= ES_WS_LDS_MAX: one launch, one 1024-thread workgroup per problem, keys and tags in
//     LDS (8192 x (8 + 1) B = 72 KiB of the CU's 160 KiB: two workgroups per CU).
//   larger: keys / tags in the workspace; every 8192-element tile is sorted in LDS, then per merge
//     size k the strides >= 8192 run as global compare-exchange passes and the strides below are
//     finished in LDS (one launch per k); a last launch takes the sums, one workgroup per problem.
// Reductions: per thread in index order, then block_sum_d: a fixed order, no atomics, bitwise
// reproducible.
#include "common.h"
#include "segment.h"

namespace {

constexpr int WS_TILE = ES_WS_LDS_MAX;     // elements of one LDS tile
constexpr int WS_THREADS = 1024;
constexpr int WS_MAX = 1 << 20;            // largest nu_cap + nv_cap of one problem
constexpr uint64_t WS_PAD = ~0ull;         // above every finite value's key

struct WsArgs {
  const double* u; int64_t u_ld; int u_rows; const int32_t* u_idx; const int32_t* u_seg; int u_cap;
  const double* v; int64_t v_ld; int v_rows; const int32_t* v_idx; const int32_t* v_seg; int v_cap;
  int channels;
};

__device__ __forceinline__ int ws_pow2(int m) {       // next power of two, >= 2
  int p = 2;
  while (p < m) p <<= 1;
  return p;
}

// element i of problem (s, c): i < nu from u, i < nu + nv from v, else padding
__device__ __forceinline__ void ws_fetch(const WsArgs& a, int c, SegSpan su, SegSpan sv, int i, uint64_t& key,
                                         uint8_t& tag) {
  if (i < su.n) {
    key = f64_key(a.u[(int64_t)seg_row(a.u_idx, su.b + i, a.u_rows) * a.u_ld + c]);
    tag = 1;
  } else if (i < su.n + sv.n) {
    key = f64_key(a.v[(int64_t)seg_row(a.v_idx, sv.b + i - su.n, a.v_rows) * a.v_ld + c]);
    tag = 0;
  } else {
    key = WS_PAD;
    tag = 0;
  }
}

// Bitonic stages on the n (a power of two <= WS_TILE) elements of one LDS tile whose first element has
// global index `base`: merge sizes k_lo .. k_hi, per size the strides min(k / 2, n / 2) .. 1.
__device__ __forceinline__ void ws_lds_stages(uint64_t* sk, uint8_t* st, int n, int base, int k_lo, int k_hi) {
  for (int k = k_lo; k <= k_hi; k <<= 1) {
    for (int j = (k >> 1) < (n >> 1) ? (k >> 1) : (n >> 1); j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n >> 1); t += WS_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const uint64_t a = sk[i], b = sk[p];
        const bool up = ((base + i) & k) == 0;
        if ((a > b) == up && a != b) {
          sk[i] = b; sk[p] = a;
          const uint8_t ta = st[i];
          st[i] = st[p]; st[p] = ta;
        }
      }
      __syncthreads();
    }
  }
}

// The sum over the sorted keys / tags (LDS or global), every thread gets it.  shi: 16 ints, shd: 16 doubles.
__device__ __forceinline__ double ws_sum(const uint64_t* keys, const uint8_t* tags, int m, int nu, int nv, int* shi,
                                         double* shd) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t le = ((1ull << lane) << 1) - 1ull;        // lanes <= mine
  const double dnu = (double)nu, dnv = (double)nv;
  double acc = 0.0;
  int base = 0;
  for (int t0 = 0; t0 < m - 1; t0 += WS_THREADS) {
    const int k = t0 + (int)threadIdx.x;
    const bool live = k < m - 1;
    const int tag = live ? (int)tags[k] : 0;
    const uint64_t bal = __ballot(tag != 0);
    if (lane == 0) shi[wid] = __popcll(bal);
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WS_THREADS / 64; ++w) {
      const int cw = shi[w];
      pre += w < wid ? cw : 0;
      tot += cw;
    }
    if (live) {
      const int cu = base + pre + __popcll(bal & le), cv = k + 1 - cu;
      const double d = f64_unkey(keys[k + 1]) - f64_unkey(keys[k]);
      acc += fabs((double)cu / dnu - (double)cv / dnv) * d;
    }
    base += tot;
    __syncthreads();
  }
  return block_sum_d(acc, shd);
}

// ------------------------------------------------------------------------------------------ LDS path
__global__ void __launch_bounds__(WS_THREADS) ws_lds_kernel(WsArgs a, double* __restrict__ out) {
  __shared__ uint64_t sk[WS_TILE];
  __shared__ uint8_t st[WS_TILE];
  __shared__ int shi[WS_THREADS / 64];
  __shared__ double shd[WS_THREADS / 64];
  const int prob = blockIdx.x, s = prob / a.channels, c = prob - s * a.channels;
  const SegSpan su = seg_span(a.u_seg, s, a.u_rows, a.u_cap), sv = seg_span(a.v_seg, s, a.v_rows, a.v_cap);
  if (su.n == 0 || sv.n == 0) {                      // block-uniform
    if (threadIdx.x == 0) out[prob] = 0.0;
    return;
  }
  const int m = su.n + sv.n;                         // <= u_cap + v_cap <= WS_TILE
  const int pm = ws_pow2(m);
  for (int i = threadIdx.x; i < pm; i += WS_THREADS) ws_fetch(a, c, su, sv, i, sk[i], st[i]);
  __syncthreads();
  ws_lds_stages(sk, st, pm, 0, 2, pm);
  const double d = ws_sum(sk, st, m, su.n, sv.n, shi, shd);
  if (threadIdx.x == 0) out[prob] = d;
}

// --------------------------------------------------------------------------------------- global path
// Workspace: keys [nprob][P] uint64, then tags [nprob][P] uint8, P = the padded host bound.
// mode 0: fetch the tile's elements and sort it (merge sizes 2 .. min(pm, WS_TILE));
// mode 1: the strides below WS_TILE of merge size k.
__global__ void __launch_bounds__(WS_THREADS) ws_tile_kernel(WsArgs a, int P, int mode, int k, uint64_t* wk,
                                                             uint8_t* wt) {
  __shared__ uint64_t sk[WS_TILE];
  __shared__ uint8_t st[WS_TILE];
  const int prob = blockIdx.y, s = prob / a.channels, c = prob - s * a.channels;
  const SegSpan su = seg_span(a.u_seg, s, a.u_rows, a.u_cap), sv = seg_span(a.v_seg, s, a.v_rows, a.v_cap);
  if (su.n == 0 || sv.n == 0) return;
  const int pm = ws_pow2(su.n + sv.n);               // <= P
  const int base = blockIdx.x * WS_TILE;
  if (base >= pm || (mode == 1 && k > pm)) return;   // block-uniform
  const int n = pm < WS_TILE ? pm : WS_TILE;
  uint64_t* gk = wk + (int64_t)prob * P + base;
  uint8_t* gt = wt + (int64_t)prob * P + base;
  if (mode == 0) {
    for (int i = threadIdx.x; i < n; i += WS_THREADS) ws_fetch(a, c, su, sv, base + i, sk[i], st[i]);
  } else {
    for (int i = threadIdx.x; i < n; i += WS_THREADS) { sk[i] = gk[i]; st[i] = gt[i]; }
  }
  __syncthreads();
  if (mode == 0) ws_lds_stages(sk, st, n, base, 2, n);
  else ws_lds_stages(sk, st, n, base, k, k);
  for (int i = threadIdx.x; i < n; i += WS_THREADS) { gk[i] = sk[i]; gt[i] = st[i]; }
}

// one compare-exchange pass of merge size k at stride j >= WS_TILE
__global__ void __launch_bounds__(WS_THREADS) ws_global_stage_kernel(WsArgs a, int P, int k, int j, uint64_t* wk,
                                                                     uint8_t* wt) {
  const int prob = blockIdx.y, s = prob / a.channels;
  const SegSpan su = seg_span(a.u_seg, s, a.u_rows, a.u_cap), sv = seg_span(a.v_seg, s, a.v_rows, a.v_cap);
  if (su.n == 0 || sv.n == 0) return;
  const int pm = ws_pow2(su.n + sv.n);
  const int t = blockIdx.x * WS_THREADS + threadIdx.x;
  if (k > pm || t >= (pm >> 1)) return;
  uint64_t* gk = wk + (int64_t)prob * P;
  uint8_t* gt = wt + (int64_t)prob * P;
  const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
  const uint64_t x = gk[i], y = gk[p];
  const bool up = (i & k) == 0;
  if ((x > y) == up && x != y) {
    gk[i] = y; gk[p] = x;
    const uint8_t tx = gt[i];
    gt[i] = gt[p]; gt[p] = tx;
  }
}

__global__ void __launch_bounds__(WS_THREADS) ws_sum_kernel(WsArgs a, int P, const uint64_t* wk, const uint8_t* wt,
                                                            double* __restrict__ out) {
  __shared__ int shi[WS_THREADS / 64];
  __shared__ double shd[WS_THREADS / 64];
  const int prob = blockIdx.x, s = prob / a.channels;
  const SegSpan su = seg_span(a.u_seg, s, a.u_rows, a.u_cap), sv = seg_span(a.v_seg, s, a.v_rows, a.v_cap);
  if (su.n == 0 || sv.n == 0) {
    if (threadIdx.x == 0) out[prob] = 0.0;
    return;
  }
  const double d = ws_sum(wk + (int64_t)prob * P, wt + (int64_t)prob * P, su.n + sv.n, su.n, sv.n, shi, shd);
  if (threadIdx.x == 0) out[prob] = d;
}

int64_t ws_padded(int64_t cap) {
  int64_t p = 2;
  while (p < cap) p <<= 1;
  return p;
}

}  // namespace

extern "C" int es_wasserstein_lds_max(void) { return ES_WS_LDS_MAX; }

extern "C" size_t es_wasserstein_1d_workspace(int n_seg, int channels, int u_cap, int v_cap) {
  if (n_seg <= 0 || channels <= 0 || u_cap < 0 || v_cap < 0) return 0;
  const int64_t cap = (int64_t)u_cap + v_cap;
  if (cap <= WS_TILE || cap > WS_MAX) return 0;       // LDS path (or an argument error of the call)
  return (size_t)n_seg * (size_t)channels * (size_t)ws_padded(cap) * (sizeof(uint64_t) + sizeof(uint8_t));
}

extern "C" int es_wasserstein_1d(const double* u, int64_t u_ld, int u_rows, const int32_t* u_idx, const int32_t* u_seg,
                                 const double* v, int64_t v_ld, int v_rows, const int32_t* v_idx, const int32_t* v_seg,
                                 int n_seg, int channels, int u_cap, int v_cap, double* out, void* work,
                                 size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(u && v && u_seg && v_seg && out, "wasserstein_1d: null argument");
  ES_CHECK_ARG(n_seg > 0 && channels > 0, "wasserstein_1d: n_seg=%d channels=%d", n_seg, channels);
  ES_CHECK_ARG(u_rows > 0 && v_rows > 0, "wasserstein_1d: u_rows=%d v_rows=%d", u_rows, v_rows);
  ES_CHECK_ARG(u_ld >= channels && v_ld >= channels, "wasserstein_1d: row stride below %d channels", channels);
  ES_CHECK_ARG(u_cap >= 0 && v_cap >= 0, "wasserstein_1d: u_cap=%d v_cap=%d", u_cap, v_cap);
  const int64_t cap = (int64_t)u_cap + v_cap;
  ES_CHECK_ARG(cap <= WS_MAX, "wasserstein_1d: u_cap + v_cap = %lld above %d", (long long)cap, WS_MAX);
  const int64_t nprob = (int64_t)n_seg * channels;
  ES_CHECK_ARG(nprob <= 65535, "wasserstein_1d: %lld problems above 65535", (long long)nprob);
  const WsArgs a = {u, u_ld, u_rows, u_idx, u_seg, u_cap, v, v_ld, v_rows, v_idx, v_seg, v_cap, channels};
  const hipStream_t st = (hipStream_t)stream;
  if (cap <= WS_TILE) {
    hipLaunchKernelGGL(ws_lds_kernel, dim3((unsigned)nprob), dim3(WS_THREADS), 0, st, a, out);
    ES_CHECK_LAUNCH();
    return ES_OK;
  }
  const size_t need = es_wasserstein_1d_workspace(n_seg, channels, u_cap, v_cap);
  ES_CHECK_ARG(work && work_bytes >= need, "wasserstein_1d: workspace of %zu bytes, %zu needed", work_bytes, need);
  const int P = (int)ws_padded(cap);
  uint64_t* wk = (uint64_t*)work;
  uint8_t* wt = (uint8_t*)(wk + (size_t)nprob * P);
  const dim3 tiles(P / WS_TILE, (unsigned)nprob), pairs(P / 2 / WS_THREADS, (unsigned)nprob);
  hipLaunchKernelGGL(ws_tile_kernel, tiles, dim3(WS_THREADS), 0, st, a, P, 0, 0, wk, wt);
  for (int k = 2 * WS_TILE; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= WS_TILE; j >>= 1)
      hipLaunchKernelGGL(ws_global_stage_kernel, pairs, dim3(WS_THREADS), 0, st, a, P, k, j, wk, wt);
    hipLaunchKernelGGL(ws_tile_kernel, tiles, dim3(WS_THREADS), 0, st, a, P, 1, k, wk, wt);
  }
  hipLaunchKernelGGL(ws_sum_kernel, dim3((unsigned)nprob), dim3(WS_THREADS), 0, st, a, P, wk, wt, out);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
