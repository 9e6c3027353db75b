// Order statistics on the device: the quantiles at n_q probabilities of column c of the u rows and of the v rows of
// segment s (include/expertsim_hip.h, es_segment_quantiles), by numpy's default rule (quantile_rule.h).  Arguments,
// segments, caps and the two paths are es_wasserstein_1d's; the sort is tagged_sort.h's, ONE sort of both sides,
// fetched with -0.0 as +0.0 so that equal values have equal keys, and with ONE_SIDED so that a side can be alone.
//
// With t[k] the tags of the sorted positions (1: from u) and cu[k] the count of tags 1 among t[0..k], the element at
// position k is the (cu[k] - 1)-th order statistic of u when t[k] = 1 and the (k - cu[k])-th of v otherwise: its
// exclusive prefix count of its own tag.  The counts cross the positions as in rank.hip: a ballot per wave, the 16
// wave totals in LDS, a carry from chunk to chunk.  Every (side, probability) needs the two order statistics lo and
// hi; exactly one position holds each, so each slot of the small LDS table has one writer.  Equal keys are equal
// values, so the order the network leaves inside a run cannot matter.
#include "quantile_rule.h"
#include "tagged_sort.h"

namespace {

struct QtProbs { double p[ES_QUANTILE_MAX_Q]; int n; };

constexpr int QT_SLOTS = 2 * ES_QUANTILE_MAX_Q;          // (side, probability)

struct QtShared {
  int cnt[TS_THREADS / 64];
  int lo[QT_SLOTS], hi[QT_SLOTS];
  double g[QT_SLOTS], a[QT_SLOTS], b[QT_SLOTS];
};

// The quantiles of both sides from the sorted keys / tags (LDS or global) of one problem, m = nu + nv > 0.
// out: the problem's [2][n_q] results.
__device__ __forceinline__ void qt_extract(const uint64_t* keys, const uint8_t* tags, int m, int nu, int nv,
                                           const QtProbs& pr, QtShared& sh, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  constexpr int NW = TS_THREADS / 64;
  const uint64_t le = ((1ull << lane) << 1) - 1ull;        // lanes <= mine
  const int nq = pr.n;
  if ((int)threadIdx.x < 2 * nq) {
    const int side = threadIdx.x / nq, q = threadIdx.x - side * nq, n = side ? nv : nu;
    QuantPos pos = {-1, -1, 0.0};                          // an empty side matches no position
    if (n > 0) pos = quantile_pos(pr.p[q], n);
    sh.lo[threadIdx.x] = pos.lo;
    sh.hi[threadIdx.x] = pos.hi;
    sh.g[threadIdx.x] = pos.g;
  }
  __syncthreads();
  int base = 0;                                            // u's before this chunk
  for (int t0 = 0; t0 < m; t0 += TS_THREADS) {
    const int k = t0 + (int)threadIdx.x;
    const bool live = k < m;
    const int tag = live ? (int)tags[k] : 0;
    const uint64_t bal = __ballot(tag != 0);
    if (lane == 0) sh.cnt[wid] = __popcll(bal);
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int cw = sh.cnt[w];
      pre += w < wid ? cw : 0;
      tot += cw;
    }
    if (live) {
      const int cu = base + pre + __popcll(bal & le);      // inclusive count of u's
      const int r = tag ? cu - 1 : k - cu;                 // my rank inside my own side
      const int s0 = tag ? 0 : nq;
      const double x = f64_unkey(keys[k]);
      for (int q = 0; q < nq; ++q) {
        if (sh.lo[s0 + q] == r) sh.a[s0 + q] = x;
        if (sh.hi[s0 + q] == r) sh.b[s0 + q] = x;
      }
    }
    base += tot;
    __syncthreads();
  }
  if ((int)threadIdx.x < 2 * nq) {
    const int side = threadIdx.x / nq, n = side ? nv : nu;
    out[threadIdx.x] = n > 0 ? quantile_lerp(sh.a[threadIdx.x], sh.b[threadIdx.x], sh.g[threadIdx.x])
                             : __builtin_nan("");
  }
}

__device__ __forceinline__ void qt_counts(int s, int c, int nu, int nv, int32_t* __restrict__ count) {
  if (c == 0 && threadIdx.x == 0) { count[2 * s] = nu; count[2 * s + 1] = nv; }
}

__device__ __forceinline__ void qt_empty(const QtProbs& pr, double* __restrict__ out) {
  if ((int)threadIdx.x < 2 * pr.n) out[threadIdx.x] = __builtin_nan("");
}

// ------------------------------------------------------------------------------------------ LDS path
__global__ void __launch_bounds__(TS_THREADS) qt_lds_kernel(TsArgs a, QtProbs pr, double* __restrict__ out,
                                                            int32_t* __restrict__ count) {
  __shared__ uint64_t sk[TS_TILE];
  __shared__ uint8_t st[TS_TILE];
  __shared__ QtShared sh;
  const int prob = blockIdx.x, s = prob / a.channels, c = prob - s * a.channels;
  const SegSpan su = seg_span(a.u_seg, s, a.u_rows, a.u_cap), sv = seg_span(a.v_seg, s, a.v_rows, a.v_cap);
  double* o = out + (int64_t)prob * 2 * pr.n;
  qt_counts(s, c, su.n, sv.n, count);
  if (ts_skip<true>(su, sv)) {                       // block-uniform
    qt_empty(pr, o);
    return;
  }
  const int m = su.n + sv.n;                         // <= u_cap + v_cap <= TS_TILE
  const int pm = ts_pow2(m);
  for (int i = threadIdx.x; i < pm; i += TS_THREADS) ts_fetch<true>(a, c, su, sv, i, sk[i], st[i]);
  __syncthreads();
  ts_lds_stages(sk, st, pm, 0, 2, pm);
  qt_extract(sk, st, m, su.n, sv.n, pr, sh, o);
}

// --------------------------------------------------------------------------------------- global path
// tagged_sort.h sorts into the workspace; this launch extracts, one workgroup per problem.
__global__ void __launch_bounds__(TS_THREADS) qt_extract_kernel(TsArgs a, QtProbs pr, int P, const uint64_t* wk,
                                                                const uint8_t* wt, double* __restrict__ out,
                                                                int32_t* __restrict__ count) {
  __shared__ QtShared sh;
  const int prob = blockIdx.x, s = prob / a.channels, c = prob - s * a.channels;
  const SegSpan su = seg_span(a.u_seg, s, a.u_rows, a.u_cap), sv = seg_span(a.v_seg, s, a.v_rows, a.v_cap);
  double* o = out + (int64_t)prob * 2 * pr.n;
  qt_counts(s, c, su.n, sv.n, count);
  if (ts_skip<true>(su, sv)) {
    qt_empty(pr, o);
    return;
  }
  qt_extract(wk + (int64_t)prob * P, wt + (int64_t)prob * P, su.n + sv.n, su.n, sv.n, pr, sh, o);
}

}  // namespace

extern "C" size_t es_segment_quantiles_workspace(int n_seg, int channels, int u_cap, int v_cap) {
  return ts_workspace(n_seg, channels, u_cap, v_cap);   // 0: the LDS path (or an argument error of the call)
}

extern "C" int es_segment_quantiles(const double* u, int64_t u_ld, int u_rows, const int32_t* u_idx,
                                    const int32_t* u_seg, const double* v, int64_t v_ld, int v_rows,
                                    const int32_t* v_idx, const int32_t* v_seg, int n_seg, int channels, int u_cap,
                                    int v_cap, const double* probs, int n_q, double* out, int32_t* count, void* work,
                                    size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(u && u_seg && out && count && probs, "segment_quantiles: null argument");
  const bool one = v == nullptr;                        // the one-sample form
  ES_CHECK_ARG(one ? (v_rows == 0 && v_cap == 0) : (v_seg != nullptr && v_rows > 0),
               "segment_quantiles: v=%p v_seg=%p v_rows=%d v_cap=%d (one sample: v NULL, v_rows = v_cap = 0)",
               (const void*)v, (const void*)v_seg, v_rows, v_cap);
  ES_CHECK_ARG(n_seg > 0 && channels > 0, "segment_quantiles: n_seg=%d channels=%d", n_seg, channels);
  ES_CHECK_ARG(u_rows > 0, "segment_quantiles: u_rows=%d", u_rows);
  ES_CHECK_ARG(u_ld >= channels && (one || v_ld >= channels), "segment_quantiles: row stride below %d channels",
               channels);
  ES_CHECK_ARG(u_cap >= 0 && v_cap >= 0, "segment_quantiles: u_cap=%d v_cap=%d", u_cap, v_cap);
  ES_CHECK_ARG(n_q >= 1 && n_q <= ES_QUANTILE_MAX_Q, "segment_quantiles: n_q=%d outside 1 .. %d", n_q,
               ES_QUANTILE_MAX_Q);
  QtProbs pr;
  pr.n = n_q;
  for (int k = 0; k < ES_QUANTILE_MAX_Q; ++k) {
    pr.p[k] = k < n_q ? probs[k] : 0.0;
    ES_CHECK_ARG(quantile_prob_ok(pr.p[k]), "segment_quantiles: probs[%d]=%g outside [0, 1]", k, pr.p[k]);
  }
  const int64_t cap = (int64_t)u_cap + v_cap;
  ES_CHECK_ARG(cap <= TS_MAX, "segment_quantiles: u_cap + v_cap = %lld above %d", (long long)cap, TS_MAX);
  const int64_t nprob = (int64_t)n_seg * channels;
  ES_CHECK_ARG(nprob <= 65535, "segment_quantiles: %lld problems above 65535", (long long)nprob);
  // one sample: the v side is the empty span of every segment (rows = 0 clamps it), and v is never read
  const TsArgs a = {u, u_ld, u_rows, u_idx, u_seg, u_cap, v, one ? u_ld : v_ld, one ? 0 : v_rows,
                    one ? nullptr : v_idx, one ? u_seg : v_seg, one ? 0 : v_cap, channels};
  const hipStream_t st = (hipStream_t)stream;
  if (cap <= TS_TILE) {
    hipLaunchKernelGGL(qt_lds_kernel, dim3((unsigned)nprob), dim3(TS_THREADS), 0, st, a, pr, out, count);
    ES_CHECK_LAUNCH();
    return ES_OK;
  }
  const size_t need = es_segment_quantiles_workspace(n_seg, channels, u_cap, v_cap);
  ES_CHECK_ARG(work && work_bytes >= need, "segment_quantiles: workspace of %zu bytes, %zu needed", work_bytes, need);
  const int P = (int)ts_padded(cap);
  uint64_t* wk = (uint64_t*)work;
  uint8_t* wt = (uint8_t*)(wk + (size_t)nprob * P);
  ts_sort_global<true, true>(a, nprob, P, wk, wt, st);
  hipLaunchKernelGGL(qt_extract_kernel, dim3((unsigned)nprob), dim3(TS_THREADS), 0, st, a, pr, P, wk, wt, out, count);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
