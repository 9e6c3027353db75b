// Host-only driver of csrc/segment.h for tests/test_segments_cpu.py: prints seg_span and seg_row over a small
// exhaustive grid, and the carver's offsets.  No kernel, no HIP call.
//   S rows b e cap B N    seg_span(b, e, rows, cap) = {B, N}; cap 0 stands for the call without a cap.  Both
//                         overloads are evaluated and must agree (exit 1 otherwise).
//   R rows p v r          seg_row(idx, p, rows) = r with idx[p] = v; v = x: a NULL idx
//   K x k                 f64_key(x) as hex; f64_unkey of it must give x back bit for bit (exit 1 otherwise)
//   C align off...        the offsets after taking 3 doubles, 5 int32, 0 floats and 1 byte
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "segment.h"

int main() {
  for (int rows = 0; rows <= 4; ++rows) {
    for (int b = -3; b <= rows + 3; ++b)
      for (int e = -3; e <= rows + 3; ++e)
        for (int cap = 0; cap <= 5; ++cap) {
          const int32_t seg[4] = {7, 7, b, e};
          const SegSpan x = cap ? seg_span(b, e, rows, cap) : seg_span(b, e, rows);
          const SegSpan y = cap ? seg_span(seg, 1, rows, cap) : seg_span(seg, 1, rows);
          if (x.b != y.b || x.n != y.n) return 1;
          printf("S %d %d %d %d %d %d\n", rows, b, e, cap, x.b, x.n);
        }
    int32_t idx[4];
    for (int p = 0; p < rows; ++p) {
      printf("R %d %d x %d\n", rows, p, seg_row(nullptr, p, rows));
      for (int v = -2; v <= rows + 2; ++v) {
        for (int q = 0; q < rows; ++q) idx[q] = q == p ? v : 1000;
        printf("R %d %d %d %d\n", rows, p, v, seg_row(idx, p, rows));
      }
    }
  }
  const double xs[] = {-1e300, -2.5, -1e-300, -0.0, 0.0, 1e-300, 2.5, 1e300};
  for (double x : xs) {
    const uint64_t k = f64_key(x);
    const double back = f64_unkey(k);
    if (memcmp(&back, &x, sizeof x) != 0) return 1;
    printf("K %a %016" PRIx64 "\n", x, k);
  }
  for (size_t align : {8, 16, 256}) {
    for (int pass = 0; pass < 2; ++pass) {
      static char buf[2048];
      Carver c(pass ? buf : nullptr, align);
      char* p0 = (char*)c.take<double>(3);
      const size_t o1 = c.bytes();
      char* p1 = (char*)c.take<int32_t>(5);
      const size_t o2 = c.bytes();
      c.take<float>(0);
      const size_t o3 = c.bytes();
      c.take<char>(1);
      if (pass ? (p0 != buf || p1 != buf + o1) : (p0 != nullptr || p1 != nullptr)) return 1;
      if (pass) printf("C %zu %zu %zu %zu %zu\n", align, o1, o2, o3, c.bytes());
    }
  }
  return 0;
}
