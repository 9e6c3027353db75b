// Host-only driver of csrc/quantile_rule.h for tests/test_conditional_cpu.py: applies the quantile rule and the bin
// rule to the cases on standard input and prints the results as hexadecimal doubles / integers.  No kernel, no HIP
// call.  Numbers are read with %la, so the test passes the exact bits (float.hex()).
//   Q p n x_0 .. x_(n-1)          the sorted values; prints "Q <quantile at p>"
//   B x m e_0 .. e_(m-1)          the ascending edges; prints "B <bin_of(edges, m, x)>"
//   C bin n_bins expert n_experts prints "C <bin_class(..)>"
//   P p                           prints "P <quantile_prob_ok(p)>"
#include <stdio.h>

#include <vector>

#include "quantile_rule.h"

int main() {
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'Q' || kind == 'B') {
      double first;
      int n;
      if (scanf("%la %d", &first, &n) != 2 || n < 0) return 1;
      std::vector<double> x(n);
      for (int i = 0; i < n; ++i)
        if (scanf("%la", &x[i]) != 1) return 1;
      if (kind == 'Q') {
        if (n < 1 || !quantile_prob_ok(first)) return 1;
        const QuantPos pos = quantile_pos(first, n);
        if (pos.lo < 0 || pos.hi >= n || pos.lo > pos.hi) return 1;
        printf("Q %a\n", quantile_lerp(x[pos.lo], x[pos.hi], pos.g));
      } else {
        printf("B %d\n", bin_of(x.data(), n, first));
      }
    } else if (kind == 'C') {
      int b, nb, e, ne;
      if (scanf("%d %d %d %d", &b, &nb, &e, &ne) != 4) return 1;
      printf("C %d\n", bin_class(b, nb, e, ne));
    } else if (kind == 'P') {
      double p;
      if (scanf("%la", &p) != 1) return 1;
      printf("P %d\n", quantile_prob_ok(p) ? 1 : 0);
    } else {
      return 1;
    }
  }
  return 0;
}
