// What the analysis files (wasserstein, prepare, diagnostics, embedding, cluster, fidelity) share: the segment
// rule of include/expertsim_hip.h ("Segments follow es_wasserstein_1d"), the order-preserving key of a double
// and the carving of a workspace.  Host and device code; nothing here launches or allocates.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

// ---------------------------------------------------------------- segments
// The positions [b, b + n) of a segment with the bounds (b, e) over `rows` positions: b clamped to [0, rows],
// e to [b, rows], the length to cap.
struct SegSpan { int b, n; };
__host__ __device__ __forceinline__ SegSpan seg_span(int b, int e, int rows, int cap = INT_MAX) {
  b = b < 0 ? 0 : (b > rows ? rows : b);
  e = e < b ? b : (e > rows ? rows : e);
  const int n = e - b;
  return {b, n < cap ? n : cap};
}
// segment s of seg [n_seg][2]
__host__ __device__ __forceinline__ SegSpan seg_span(const int32_t* seg, int s, int rows, int cap = INT_MAX) {
  return seg_span(seg[2 * s], seg[2 * s + 1], rows, cap);
}
// the row of position p (0 <= p < rows): p itself without an index, else idx[p] clamped to [0, rows)
__host__ __device__ __forceinline__ int seg_row(const int32_t* idx, int p, int rows) {
  if (idx == nullptr) return p;
  const int r = idx[p];
  return r < 0 ? 0 : (r >= rows ? rows - 1 : r);
}

// ---------------------------------------------------------------- ordered keys
// a < b  <=>  f64_key(a) < f64_key(b) as unsigned integers (sign-flipped IEEE bits); no key of a number is 0
// or all ones
__host__ __device__ __forceinline__ uint64_t f64_key(double x) {
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double f64_unkey(uint64_t k) {
  return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k);
}

// ---------------------------------------------------------------- workspaces (host)
// Arrays taken one after the other from a workspace, each padded to `align` bytes (a power of two).  With a
// null base it only measures: bytes() after the same takes is the size the workspace needs.
class Carver {
 public:
  Carver(void* base, size_t align) : base_((char*)base), align_(align) {}
  template <class T> T* take(size_t count) {
    T* p = base_ ? (T*)(base_ + off_) : nullptr;
    off_ += (count * sizeof(T) + align_ - 1) & ~(align_ - 1);
    return p;
  }
  size_t bytes() const { return off_; }

 private:
  char* base_;
  size_t align_, off_ = 0;
};
