// Exact two-sample rank statistics on the device: the Mann-Whitney rank sum (ROC AUC) and the Kolmogorov-Smirnov
// statistic of column c of the u rows against the v rows of segment s, as integers (include/expertsim_hip.h,
// es_rank_stats).  Arguments, segments, caps and the two paths are es_wasserstein_1d's; the sort is
// tagged_sort.h's, fetched with -0.0 as +0.0 so that equal values have equal keys.
//
// With a[k] the sorted values, cu[k] / cv[k] the counts of u / v values among a[0..k] and a RUN a maximal stretch
// of equal values:
//   KS = max over the run ENDS k of |cu[k] nv - cv[k] nu|;
//   U2 = sum_pairs 2 [u > v] + [u == v] = nu nv + sum_pairs [v < u] - sum_pairs [u < v], and
//        sum_pairs [v < u] = sum over the u elements of cv before their run's START (likewise [u < v]).
// Counts are looked at only at run starts and run ends, so the order inside a run (the bitonic network is not
// stable) cannot matter.  "The counts before my run's start" reach every element by a prefix MAXIMUM over the
// positions (the counts are monotone, so the latest start's are the largest).  Everything is integer arithmetic
// (nu nv <= 2^38): sums and maxima in any order give the same bits, no atomics.
#include "tagged_sort.h"

namespace {

__device__ __forceinline__ int rk_shfl_up(int v, int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ long long rk_shfl_xor_ll(long long v, int m) {
  const int lo = __shfl_xor((int)(v & 0xFFFFFFFFll), m, 64), hi = __shfl_xor((int)(v >> 32), m, 64);
  return ((long long)hi << 32) | (unsigned int)lo;
}

// out4 = (nu, nv, U2, KS) from the sorted keys / tags (LDS or global) of one problem; thread 0 writes.
// shi: 3 x 16 ints, shl: 2 x 16 long longs.
__device__ __forceinline__ void rk_stats(const uint64_t* keys, const uint8_t* tags, int m, int nu, int nv, int* shi,
                                         long long* shl, long long* out4) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  constexpr int NW = TS_THREADS / 64;
  const uint64_t le = ((1ull << lane) << 1) - 1ull;        // lanes <= mine
  long long acc = 0, ks = 0;                               // sum [v < u] - sum [u < v]; the running maximum
  int base = 0, car_u = 0, car_v = 0;                      // u's before this chunk; the latest start's counts
  for (int t0 = 0; t0 < m; t0 += TS_THREADS) {
    const int k = t0 + (int)threadIdx.x;
    const bool live = k < m;
    const uint64_t key = live ? keys[k] : 0;
    const int tag = live ? (int)tags[k] : 0;
    const bool start = live && (k == 0 || keys[k - 1] != key);
    const bool end = live && (k == m - 1 || keys[k + 1] != key);
    const uint64_t bal = __ballot(tag != 0);
    if (lane == 0) shi[wid] = __popcll(bal);
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int cw = shi[w];
      pre += w < wid ? cw : 0;
      tot += cw;
    }
    const int cu = base + pre + __popcll(bal & le), cv = k + 1 - cu;      // inclusive counts
    // the counts before the latest run start at or before k: an inclusive prefix maximum
    int su = start ? cu - tag : 0, sv = start ? cv - (1 - tag) : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int ou = rk_shfl_up(su, d), ov = rk_shfl_up(sv, d);
      if (lane >= d) { su = su > ou ? su : ou; sv = sv > ov ? sv : ov; }
    }
    if (lane == 63) { shi[NW + wid] = su; shi[2 * NW + wid] = sv; }
    __syncthreads();
    int pu = car_u, pv = car_v, lu = car_u, lv = car_v;     // maxima of the waves before mine; of all waves
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int wu = shi[NW + w], wv = shi[2 * NW + w];
      if (w < wid) { pu = pu > wu ? pu : wu; pv = pv > wv ? pv : wv; }
      lu = lu > wu ? lu : wu; lv = lv > wv ? lv : wv;
    }
    su = su > pu ? su : pu;
    sv = sv > pv ? sv : pv;
    if (live) {
      acc += tag ? (long long)sv : -(long long)su;
      if (end) {
        long long d = (long long)cu * nv - (long long)cv * nu;
        d = d < 0 ? -d : d;
        ks = ks > d ? ks : d;
      }
    }
    base += tot;
    car_u = lu;
    car_v = lv;
    __syncthreads();
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += rk_shfl_xor_ll(acc, o);
    const long long other = rk_shfl_xor_ll(ks, o);
    ks = ks > other ? ks : other;
  }
  if (lane == 0) { shl[wid] = acc; shl[NW + wid] = ks; }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long a = 0, kmax = 0;
    for (int w = 0; w < NW; ++w) {
      a += shl[w];
      kmax = kmax > shl[NW + w] ? kmax : shl[NW + w];
    }
    out4[0] = nu;
    out4[1] = nv;
    out4[2] = (long long)nu * nv + a;
    out4[3] = kmax;
  }
}

__device__ __forceinline__ void rk_empty(int nu, int nv, long long* out4) {
  if (threadIdx.x == 0) { out4[0] = nu; out4[1] = nv; out4[2] = 0; out4[3] = 0; }
}

__global__ void __launch_bounds__(TS_THREADS) rk_lds_kernel(TsArgs a, long long* __restrict__ out) {
  __shared__ uint64_t sk[TS_TILE];
  __shared__ uint8_t st[TS_TILE];
  __shared__ int shi[3 * TS_THREADS / 64];
  __shared__ long long shl[2 * TS_THREADS / 64];
  const int prob = blockIdx.x, s = prob / a.channels, c = prob - s * a.channels;
  const SegSpan su = seg_span(a.u_seg, s, a.u_rows, a.u_cap), sv = seg_span(a.v_seg, s, a.v_rows, a.v_cap);
  if (su.n == 0 || sv.n == 0) {                      // block-uniform
    rk_empty(su.n, sv.n, out + 4 * (int64_t)prob);
    return;
  }
  const int m = su.n + sv.n;                         // <= u_cap + v_cap <= TS_TILE
  const int pm = ts_pow2(m);
  for (int i = threadIdx.x; i < pm; i += TS_THREADS) ts_fetch<true>(a, c, su, sv, i, sk[i], st[i]);
  __syncthreads();
  ts_lds_stages(sk, st, pm, 0, 2, pm);
  rk_stats(sk, st, m, su.n, sv.n, shi, shl, out + 4 * (int64_t)prob);
}

__global__ void __launch_bounds__(TS_THREADS) rk_stat_kernel(TsArgs a, int P, const uint64_t* wk, const uint8_t* wt,
                                                             long long* __restrict__ out) {
  __shared__ int shi[3 * TS_THREADS / 64];
  __shared__ long long shl[2 * TS_THREADS / 64];
  const int prob = blockIdx.x, s = prob / a.channels;
  const SegSpan su = seg_span(a.u_seg, s, a.u_rows, a.u_cap), sv = seg_span(a.v_seg, s, a.v_rows, a.v_cap);
  if (su.n == 0 || sv.n == 0) {
    rk_empty(su.n, sv.n, out + 4 * (int64_t)prob);
    return;
  }
  rk_stats(wk + (int64_t)prob * P, wt + (int64_t)prob * P, su.n + sv.n, su.n, sv.n, shi, shl,
           out + 4 * (int64_t)prob);
}

}  // namespace

extern "C" size_t es_rank_stats_workspace(int n_seg, int channels, int u_cap, int v_cap) {
  return ts_workspace(n_seg, channels, u_cap, v_cap);   // 0: the LDS path (or an argument error of the call)
}

extern "C" int es_rank_stats(const double* u, int64_t u_ld, int u_rows, const int32_t* u_idx, const int32_t* u_seg,
                             const double* v, int64_t v_ld, int v_rows, const int32_t* v_idx, const int32_t* v_seg,
                             int n_seg, int channels, int u_cap, int v_cap, int64_t* out, void* work,
                             size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(u && v && u_seg && v_seg && out, "rank_stats: null argument");
  ES_CHECK_ARG(n_seg > 0 && channels > 0, "rank_stats: n_seg=%d channels=%d", n_seg, channels);
  ES_CHECK_ARG(u_rows > 0 && v_rows > 0, "rank_stats: u_rows=%d v_rows=%d", u_rows, v_rows);
  ES_CHECK_ARG(u_ld >= channels && v_ld >= channels, "rank_stats: row stride below %d channels", channels);
  ES_CHECK_ARG(u_cap >= 0 && v_cap >= 0, "rank_stats: u_cap=%d v_cap=%d", u_cap, v_cap);
  const int64_t cap = (int64_t)u_cap + v_cap;
  ES_CHECK_ARG(cap <= TS_MAX, "rank_stats: u_cap + v_cap = %lld above %d", (long long)cap, TS_MAX);
  const int64_t nprob = (int64_t)n_seg * channels;
  ES_CHECK_ARG(nprob <= 65535, "rank_stats: %lld problems above 65535", (long long)nprob);
  const TsArgs a = {u, u_ld, u_rows, u_idx, u_seg, u_cap, v, v_ld, v_rows, v_idx, v_seg, v_cap, channels};
  const hipStream_t st = (hipStream_t)stream;
  long long* o = (long long*)out;
  if (cap <= TS_TILE) {
    hipLaunchKernelGGL(rk_lds_kernel, dim3((unsigned)nprob), dim3(TS_THREADS), 0, st, a, o);
    ES_CHECK_LAUNCH();
    return ES_OK;
  }
  const size_t need = es_rank_stats_workspace(n_seg, channels, u_cap, v_cap);
  ES_CHECK_ARG(work && work_bytes >= need, "rank_stats: workspace of %zu bytes, %zu needed", work_bytes, need);
  const int P = (int)ts_padded(cap);
  uint64_t* wk = (uint64_t*)work;
  uint8_t* wt = (uint8_t*)(wk + (size_t)nprob * P);
  ts_sort_global<true>(a, nprob, P, wk, wt, st);
  hipLaunchKernelGGL(rk_stat_kernel, dim3((unsigned)nprob), dim3(TS_THREADS), 0, st, a, P, wk, wt, o);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
