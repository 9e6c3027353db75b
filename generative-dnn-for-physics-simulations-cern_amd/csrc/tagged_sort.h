// The tagged sort that es_wasserstein_1d (wasserstein.hip) and es_rank_stats (rank.hip) share: the nu + nv
// values of a problem (segment s, column c) are sorted together, each carrying a one-byte tag (1: from u).
//
// A bitonic network over order-preserving 64-bit keys (segment.h's f64_key), padded with all-ones keys to the
// next power of two of the LIVE nu + nv (read on the device); the padding keys sort to the end.
//   nu_cap + nv_cap <= TS_TILE: the caller's kernel fetches into LDS and runs ts_lds_stages over all merge sizes
//     (8192 x (8 + 1) B = 72 KiB of the CU's 160 KiB).
//   larger: keys / tags in the workspace, [nprob][P] uint64 then [nprob][P] uint8, P = ts_padded(cap); ts_sort_global
//     sorts every TS_TILE-element tile in LDS, then per merge size k runs the strides >= TS_TILE as global
//     compare-exchange passes and finishes the strides below in LDS (one launch per k).
// The network is not stable: equal keys end in an order that depends on the network alone, so a caller's result
// must not depend on the order inside a run of equal keys.  CANON: -0.0 is fetched as +0.0, so that equal values
// have equal keys (es_rank_stats; es_wasserstein_1d keeps the bits it always sorted).
// ONE_SIDED (defaulted false; es_segment_quantiles sets it): a problem is skipped only when BOTH sides are empty, not
// when either is, so that one side can be sorted alone.
// Every kernel is a template in an anonymous namespace: each including file gets its own instantiations.
#pragma once
#include "common.h"
#include "segment.h"

namespace {

constexpr int TS_TILE = ES_WS_LDS_MAX;     // elements of one LDS tile
constexpr int TS_THREADS = 1024;
constexpr int TS_MAX = 1 << 20;            // largest nu_cap + nv_cap of one problem
constexpr uint64_t TS_PAD = ~0ull;         // above every finite value's key

struct TsArgs {
  const double* u; int64_t u_ld; int u_rows; const int32_t* u_idx; const int32_t* u_seg; int u_cap;
  const double* v; int64_t v_ld; int v_rows; const int32_t* v_idx; const int32_t* v_seg; int v_cap;
  int channels;
};

__device__ __forceinline__ int ts_pow2(int m) {       // next power of two, >= 2
  int p = 2;
  while (p < m) p <<= 1;
  return p;
}

// a problem the sort leaves alone
template <bool ONE_SIDED> __device__ __forceinline__ bool ts_skip(SegSpan su, SegSpan sv) {
  return ONE_SIDED ? su.n + sv.n == 0 : (su.n == 0 || sv.n == 0);
}

template <bool CANON> __device__ __forceinline__ uint64_t ts_key(double x) {
  if (CANON) x = x == 0.0 ? 0.0 : x;
  return f64_key(x);
}

// element i of problem (s, c): i < nu from u, i < nu + nv from v, else padding
template <bool CANON>
__device__ __forceinline__ void ts_fetch(const TsArgs& a, int c, SegSpan su, SegSpan sv, int i, uint64_t& key,
                                         uint8_t& tag) {
  if (i < su.n) {
    key = ts_key<CANON>(a.u[(int64_t)seg_row(a.u_idx, su.b + i, a.u_rows) * a.u_ld + c]);
    tag = 1;
  } else if (i < su.n + sv.n) {
    key = ts_key<CANON>(a.v[(int64_t)seg_row(a.v_idx, sv.b + i - su.n, a.v_rows) * a.v_ld + c]);
    tag = 0;
  } else {
    key = TS_PAD;
    tag = 0;
  }
}

// Bitonic stages on the n (a power of two <= TS_TILE) elements of one LDS tile whose first element has
// global index `base`: merge sizes k_lo .. k_hi, per size the strides min(k / 2, n / 2) .. 1.
__device__ __forceinline__ void ts_lds_stages(uint64_t* sk, uint8_t* st, int n, int base, int k_lo, int k_hi) {
  for (int k = k_lo; k <= k_hi; k <<= 1) {
    for (int j = (k >> 1) < (n >> 1) ? (k >> 1) : (n >> 1); j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n >> 1); t += TS_THREADS) {
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

// --------------------------------------------------------------------------------------- global path
// mode 0: fetch the tile's elements and sort it (merge sizes 2 .. min(pm, TS_TILE));
// mode 1: the strides below TS_TILE of merge size k.
template <bool CANON, bool ONE_SIDED = false>
__global__ void __launch_bounds__(TS_THREADS) ts_tile_kernel(TsArgs a, int P, int mode, int k, uint64_t* wk,
                                                             uint8_t* wt) {
  __shared__ uint64_t sk[TS_TILE];
  __shared__ uint8_t st[TS_TILE];
  const int prob = blockIdx.y, s = prob / a.channels, c = prob - s * a.channels;
  const SegSpan su = seg_span(a.u_seg, s, a.u_rows, a.u_cap), sv = seg_span(a.v_seg, s, a.v_rows, a.v_cap);
  if (ts_skip<ONE_SIDED>(su, sv)) return;
  const int pm = ts_pow2(su.n + sv.n);               // <= P
  const int base = blockIdx.x * TS_TILE;
  if (base >= pm || (mode == 1 && k > pm)) return;   // block-uniform
  const int n = pm < TS_TILE ? pm : TS_TILE;
  uint64_t* gk = wk + (int64_t)prob * P + base;
  uint8_t* gt = wt + (int64_t)prob * P + base;
  if (mode == 0) {
    for (int i = threadIdx.x; i < n; i += TS_THREADS) ts_fetch<CANON>(a, c, su, sv, base + i, sk[i], st[i]);
  } else {
    for (int i = threadIdx.x; i < n; i += TS_THREADS) { sk[i] = gk[i]; st[i] = gt[i]; }
  }
  __syncthreads();
  if (mode == 0) ts_lds_stages(sk, st, n, base, 2, n);
  else ts_lds_stages(sk, st, n, base, k, k);
  for (int i = threadIdx.x; i < n; i += TS_THREADS) { gk[i] = sk[i]; gt[i] = st[i]; }
}

// one compare-exchange pass of merge size k at stride j >= TS_TILE
template <bool ONE_SIDED = false>
__global__ void __launch_bounds__(TS_THREADS) ts_global_stage_kernel(TsArgs a, int P, int k, int j, uint64_t* wk,
                                                                     uint8_t* wt) {
  const int prob = blockIdx.y, s = prob / a.channels;
  const SegSpan su = seg_span(a.u_seg, s, a.u_rows, a.u_cap), sv = seg_span(a.v_seg, s, a.v_rows, a.v_cap);
  if (ts_skip<ONE_SIDED>(su, sv)) return;
  const int pm = ts_pow2(su.n + sv.n);
  const int t = blockIdx.x * TS_THREADS + threadIdx.x;
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

inline int64_t ts_padded(int64_t cap) {
  int64_t p = 2;
  while (p < cap) p <<= 1;
  return p;
}

// bytes of the global path's workspace (0 on the LDS path or outside the limits)
inline size_t ts_workspace(int n_seg, int channels, int u_cap, int v_cap) {
  if (n_seg <= 0 || channels <= 0 || u_cap < 0 || v_cap < 0) return 0;
  const int64_t cap = (int64_t)u_cap + v_cap;
  if (cap <= TS_TILE || cap > TS_MAX) return 0;
  return (size_t)n_seg * (size_t)channels * (size_t)ts_padded(cap) * (sizeof(uint64_t) + sizeof(uint8_t));
}

// The global path's launches: after them wk / wt [nprob][P] hold every live problem's sorted keys and tags.
template <bool CANON, bool ONE_SIDED = false>
inline void ts_sort_global(const TsArgs& a, int64_t nprob, int P, uint64_t* wk, uint8_t* wt, hipStream_t st) {
  const dim3 tiles(P / TS_TILE, (unsigned)nprob), pairs(P / 2 / TS_THREADS, (unsigned)nprob);
  hipLaunchKernelGGL((ts_tile_kernel<CANON, ONE_SIDED>), tiles, dim3(TS_THREADS), 0, st, a, P, 0, 0, wk, wt);
  for (int k = 2 * TS_TILE; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= TS_TILE; j >>= 1)
      hipLaunchKernelGGL(ts_global_stage_kernel<ONE_SIDED>, pairs, dim3(TS_THREADS), 0, st, a, P, k, j, wk, wt);
    hipLaunchKernelGGL((ts_tile_kernel<CANON, ONE_SIDED>), tiles, dim3(TS_THREADS), 0, st, a, P, 1, k, wk, wt);
  }
}

}  // namespace
