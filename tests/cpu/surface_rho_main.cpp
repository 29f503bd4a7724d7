// TEST PROGRAM (tests/test_surface_cpu.py): the surface models of csrc/rtd_surface.h as the host compiles them, stand-alone under the
// address / undefined-behaviour sanitizers.  Reads rows "model p0 p1 p2 p3 mu mup nphi" (doubles as hex floats) from stdin and writes,
// per row, rho(mu, mup, 2 pi p / nphi) for p < nphi as hex floats on one line -- through rtd_surface_cs and rtd_surface_rho, the two
// calls rtd_surface_samples_kernel makes per sample.  A row that rtd_surface_bad refuses is answered with "bad".
#include <cstdio>
#include <vector>

#include "../../pythonic-disort_amd/csrc/rtd_surface.h"

int main() {
  int model, nphi;
  double par[4], mu, mup;
  while (std::scanf("%d %la %la %la %la %la %la %d", &model, &par[0], &par[1], &par[2], &par[3], &mu, &mup, &nphi) == 8) {
    if (rtd_surface_bad(model, par) || nphi < 1) {
      std::printf("bad\n");
      continue;
    }
    std::vector<double> rho((size_t)nphi);
    for (int p = 0; p < nphi; ++p) {
      double c, s;
      rtd_surface_cs(2.0 * (double)p / (double)nphi, &c, &s);
      rho[(size_t)p] = rtd_surface_rho(model, par, mu, mup, c, s);
    }
    for (int p = 0; p < nphi; ++p) std::printf("%a%c", rho[(size_t)p], p + 1 < nphi ? ' ' : '\n');
  }
  return 0;
}
