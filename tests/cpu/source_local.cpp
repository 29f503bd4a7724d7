// CPU harness for rtd_source_local (pythonic-disort_amd/csrc/rtd_dd.h), the routine rtd_prepare_columns_kernel runs per layer on
// the device and rtd_source_polynomials_local on the host: reads "n top sc omega a0 ... a(n-1)" lines from stdin, prints the
// coefficients about the layer's top in the scaled depth with 17 significant digits.  Used by tests/test_thermal_deep_cpu.py.
#include <cstdio>
#include <vector>

#include "../../pythonic-disort_amd/csrc/rtd_dd.h"

int main() {
  int n;
  double top, sc, om;
  while (std::scanf("%d %lf %lf %lf", &n, &top, &sc, &om) == 4) {
    std::vector<double> a(n), o(n);
    for (int i = 0; i < n; ++i)
      if (std::scanf("%lf", &a[i]) != 1) return 1;
    rtd_source_local(a.data(), o.data(), n, top, sc, om);
    for (int i = 0; i < n; ++i) std::printf("%.17g%c", o[i], i + 1 < n ? ' ' : '\n');
  }
  return 0;
}
