// TEST PROGRAM (tests/test_thermal_host_sanitized_cpu.py): the host side of rtd_plan_set_columns_thermal and rtd_planck_band
// (csrc/rtd_api.hip: the carve of the staging block, the copies, the launches) over the stand-in runtime of fake_hip/ and the
// shadow launchers of host_asan_shadow.cpp, as a stand-alone program under the address / undefined-behaviour sanitizers.  The
// thermal kernels belong to rtd_api.hip itself, so they RUN here, thread by thread, on heap memory: every index they form is
// bounds-checked.  All caller arrays are heap blocks of exactly the documented extent.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/rtd.h"
#include "../../pythonic-disort_amd/csrc/rtd_planck.h"

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rtd_last_error()); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static int scenario(int C, int L, int nquad, int M, int nbdrf) {
  const int N = nquad / 2;
  rtd_dims dims = {C, L, nquad, nquad, M, 2, nbdrf, 0};
  rtd_plan* p = nullptr;
  CHECK(rtd_plan_create(&dims, 0, &p) == 0);
  std::vector<double> mu(N), w(N, 1.0 / N);
  for (int i = 0; i < N; ++i) mu[i] = (i + 0.5) / N;
  std::vector<double> tau(C * L), om(C * L, 0.5), leg(C * L * nquad, 0.0), f(C * L, 0.0), mu0(C, 0.5), I0(C, 0.0), phi0(C, 0.0);
  for (int c = 0; c < C; ++c)
    for (int l = 0; l < L; ++l) {
      tau[c * L + l] = 0.5 * (l + 1) + 0.01 * c;
      leg[(c * L + l) * nquad] = 1.0;
    }
  std::vector<double> bp(C * M * N, 0.25), bn(C * M * N, 0.125), q(C * nbdrf * N * N + 1, 0.3), q0(C * nbdrf * N + 1, 0.3);
  std::vector<double> temper(C * (L + 1)), lo(C), hi(C), bt(C, 300.0), tt(C, 90.0), te(C, 0.7), em(C * N, 0.9);
  for (int c = 0; c < C; ++c) {
    lo[c] = 100.0 * c;
    hi[c] = lo[c] + 500.0;
    for (int l = 0; l <= L; ++l) temper[c * (L + 1) + l] = 200.0 + 10.0 * l + c;
  }
  q.pop_back();  // (exact extents; the + 1 above only keeps data() valid when nbdrf = 0)
  q0.pop_back();
  const double* Q = nbdrf ? q.data() : nullptr;
  const double* Q0 = nbdrf ? q0.data() : nullptr;
  rtd_thermal th = {temper.data(), lo.data(), hi.data(), bt.data(), tt.data(), te.data(), em.data()};
  // emissivity by Kirchhoff's law needs the quadrature: refused before it is set (only when there is a BDRF table to read)
  rtd_thermal kirch = th;
  kirch.emissivity = nullptr;
  if (nbdrf)
    CHECK(rtd_plan_set_columns_thermal(p, tau.data(), om.data(), leg.data(), nquad, f.data(), mu0.data(), I0.data(), phi0.data(),
                                       bp.data(), bn.data(), Q, Q0, &kirch) == RTD_ERR_STATE);
  CHECK(rtd_plan_set_quadrature(p, mu.data(), w.data()) == 0);
  for (int v = 0; v < 6; ++v) {
    rtd_thermal t = th;
    const double *b_pos = bp.data(), *b_neg = bn.data();
    if (v == 1) t.btemp = nullptr;
    if (v == 2) { t.ttemp = nullptr; b_pos = nullptr; }
    if (v == 3) { t.emissivity = nullptr; b_neg = nullptr; }
    if (v == 4) { t.temis = nullptr; b_pos = nullptr; b_neg = nullptr; }
    if (v == 5) { t.btemp = nullptr; t.ttemp = nullptr; t.temis = nullptr; t.emissivity = nullptr; b_pos = nullptr; b_neg = nullptr; }
    CHECK(rtd_plan_set_columns_thermal(p, tau.data(), om.data(), leg.data(), nquad, f.data(), mu0.data(), I0.data(), phi0.data(), b_pos,
                                       b_neg, Q, Q0, &t) == 0);
    CHECK(rtd_plan_solve(p) == 0 && rtd_plan_synchronize(p) == 0);
  }
  // the raw entry point on the same plan: its own s_poly, as before
  std::vector<double> sp(C * L * 2, 0.1);
  CHECK(rtd_plan_set_columns_raw(p, tau.data(), om.data(), leg.data(), nquad, f.data(), mu0.data(), I0.data(), phi0.data(), bp.data(),
                                 nullptr, sp.data(), Q, Q0) == 0);
  CHECK(rtd_plan_set_columns_raw(p, tau.data(), om.data(), leg.data(), nquad, f.data(), mu0.data(), I0.data(), phi0.data(), bp.data(),
                                 nullptr, nullptr, Q, Q0) == RTD_ERR_ARG);
  CHECK(rtd_plan_set_columns_thermal(p, tau.data(), om.data(), leg.data(), nquad, f.data(), mu0.data(), I0.data(), phi0.data(), nullptr,
                                     nullptr, Q, Q0, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_destroy(p) == 0);
  return 0;
}

int main() {
  if (scenario(5, 3, 6, 2, 1)) return 1;    // N = 3 padded to NP = 4, two modes, a BDRF table
  if (scenario(70, 1, 8, 1, 0)) return 1;   // N = NP, more than one block of columns, black surface
  if (scenario(1, 20, 32, 3, 2)) return 1;  // one column, many layers
  {                                          // a plan without a thermal source refuses the thermal entry point
    rtd_dims dims = {1, 1, 4, 4, 1, 0, 0, 0};
    rtd_plan* p = nullptr;
    CHECK(rtd_plan_create(&dims, 0, &p) == 0);
    const double one[2] = {1.0, 1.0}, zero[4] = {0.0, 0.0, 0.0, 0.0}, legc[4] = {1.0, 0.0, 0.0, 0.0};
    rtd_thermal th = {one, zero, one, nullptr, nullptr, nullptr, nullptr};
    CHECK(rtd_plan_set_columns_thermal(p, one, zero, legc, 4, zero, one, zero, zero, nullptr, nullptr, nullptr, nullptr, &th) == RTD_ERR_ARG);
    CHECK(rtd_plan_destroy(p) == 0);
  }
  // the plan-free form: a length that is no multiple of the block, every element the header's own value
  const int64_t n = 1003;
  std::vector<double> T(n), lo(n), hi(n), out(n, -1.0);
  for (int64_t i = 0; i < n; ++i) {
    T[i] = i % 17 == 0 ? 0.0 : 50.0 + 3.0 * i;
    lo[i] = 10.0 * (i % 50);
    hi[i] = lo[i] + (i % 13 == 0 ? 0.0 : 1.0 + 40.0 * (i % 29));
  }
  CHECK(rtd_planck_band(0, n, T.data(), lo.data(), hi.data(), out.data()) == 0);
  for (int64_t i = 0; i < n; ++i) CHECK(out[i] == rtd_planck_band(T[i], lo[i], hi[i]) && out[i] >= 0.0);
  CHECK(rtd_planck_band(0, 0, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(rtd_planck_band(0, 4, T.data(), nullptr, hi.data(), out.data()) == RTD_ERR_ARG);
  CHECK(rtd_planck_band(0, -1, T.data(), lo.data(), hi.data(), out.data()) == RTD_ERR_ARG);
  std::printf("THERMAL HOST OK\n");
  return 0;
}
