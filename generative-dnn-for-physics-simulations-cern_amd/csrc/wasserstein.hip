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
// Sort: tagged_sort.h's bitonic network over order-preserving 64-bit keys (shared with rank.hip), padded with
// all-ones keys to the next power of two of the LIVE nu + nv (read on the device).  The padding keys sort
// to the end and the sum stops at nu + nv - 2, so none enters it.
//   nu_cap + nv_cap <= ES_WS_LDS_MAX: one launch, one 1024-thread workgroup per problem, keys and tags in
//     LDS (8192 x (8 + 1) B = 72 KiB of the CU's 160 KiB: two workgroups per CU).
//   larger: keys / tags in the workspace; every 8192-element tile is sorted in LDS, then per merge
//     size k the strides >= 8192 run as global compare-exchange passes and the strides below are
//     finished in LDS (one launch per k); a last launch takes the sums, one workgroup per problem.
// Reductions: per thread in index order, then block_sum_d: a fixed order, no atomics, bitwise
// reproducible.
#include "tagged_sort.h"

namespace {

constexpr int WS_TILE = TS_TILE, WS_THREADS = TS_THREADS, WS_MAX = TS_MAX;
typedef TsArgs WsArgs;

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
  const int pm = ts_pow2(m);
  for (int i = threadIdx.x; i < pm; i += WS_THREADS) ts_fetch<false>(a, c, su, sv, i, sk[i], st[i]);
  __syncthreads();
  ts_lds_stages(sk, st, pm, 0, 2, pm);
  const double d = ws_sum(sk, st, m, su.n, sv.n, shi, shd);
  if (threadIdx.x == 0) out[prob] = d;
}

// --------------------------------------------------------------------------------------- global path
// tagged_sort.h sorts into the workspace; this launch takes the sums, one workgroup per problem.
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

}  // namespace

extern "C" int es_wasserstein_lds_max(void) { return ES_WS_LDS_MAX; }

extern "C" size_t es_wasserstein_1d_workspace(int n_seg, int channels, int u_cap, int v_cap) {
  return ts_workspace(n_seg, channels, u_cap, v_cap);   // 0: the LDS path (or an argument error of the call)
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
  const int P = (int)ts_padded(cap);
  uint64_t* wk = (uint64_t*)work;
  uint8_t* wt = (uint8_t*)(wk + (size_t)nprob * P);
  ts_sort_global<false>(a, nprob, P, wk, wt, st);
  hipLaunchKernelGGL(ws_sum_kernel, dim3((unsigned)nprob), dim3(WS_THREADS), 0, st, a, P, wk, wt, out);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
