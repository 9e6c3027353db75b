// The two rules of the conditional-fidelity kernels (include/expertsim_hip.h: es_segment_quantiles, es_bin_dispatch),
// as host and device functions: quantile.hip, bins.hip and the host-only tests/quantile_main.hip compile this text.
// Nothing here launches, allocates or reads memory other than the edges handed to bin_of.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// ---------------------------------------------------------------- quantiles
// numpy's default ("linear") rule for the quantile at p of n >= 1 sorted values x_(0) <= .. <= x_(n-1):
//   h = p (n - 1); lo = floor(h); g = h - lo; hi = min(lo + 1, n - 1);
//   a = x_(lo), b = x_(hi), d = b - a; the result is g >= 0.5 ? b - d (1 - g) : a + d g.
// Every operation is rounded on its own: no contraction into a fused multiply-add.
struct QuantPos { int lo, hi; double g; };

__host__ __device__ inline bool quantile_prob_ok(double p) { return p >= 0.0 && p <= 1.0; }   // false for NaN

// 0 <= p <= 1, n >= 1
__host__ __device__ inline QuantPos quantile_pos(double p, int n) {
#pragma clang fp contract(off)
  const double h = p * (double)(n - 1);
  const double fl = floor(h);
  int lo = (int)fl;
  lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
  const int hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
  return {lo, hi, h - fl};
}

__host__ __device__ inline double quantile_lerp(double a, double b, double g) {
#pragma clang fp contract(off)
  const double d = b - a;
  const double up = d * (1.0 - g), down = d * g;
  return g >= 0.5 ? b - up : a + down;
}

// ---------------------------------------------------------------- bins
// The number of edges strictly below x, edges[0 .. n_edges) ascending (equal neighbours allowed):
// np.searchsorted(edges, x, side="left"), pandas' (a, b] intervals.  A NaN x gives 0.
__host__ __device__ inline int bin_of(const double* edges, int n_edges, double x) {
  int lo = 0, hi = n_edges;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (edges[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// class of a row: its bin, or clamp(expert, 0, n_experts - 1) * n_bins + bin
__host__ __device__ inline int bin_class(int bin, int n_bins, int expert, int n_experts) {
  const int e = expert < 0 ? 0 : (expert >= n_experts ? n_experts - 1 : expert);
  return e * n_bins + bin;
}
