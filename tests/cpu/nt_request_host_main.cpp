// TEST PROGRAM (tests/test_nt_request_host_sanitized_cpu.py): rtd_plan_request_nt / rtd_plan_get_nt and what they change in
// rtd_plan_set_columns_raw, _thermal, _band and in the windows of an evaluation (csrc/rtd_api.hip), over the stand-in runtime of
// fake_hip/ and the shadow launchers of host_asan_shadow.cpp, as a stand-alone program under the address / undefined-behaviour
// sanitizers.  The preparation kernels of the corrections' inputs belong to rtd_api.hip itself, so they RUN here, thread by thread, on
// heap memory: the carve of a band's unweighted moments at the end of the staging block and the plan's buffers (one row of the
// weighted phase function per PROFILE of a band) are bounds-checked, and rtd_plan_get_nt's copies are checked by value and extent
// (the moments are 0.5, or 1: every product below is exact).  Plans of raw columns are then evaluated through every window.  A band
// plan is not evaluated here: the shadow of the apply kernel reads one row of the weighted phase function per COLUMN of its view,
// which is not what the kernel reads of a band -- the rows (c0 + c) / G of windows that are not aligned to G are held on the GPU,
// bit for bit against the batch entry (tests/test_gpu_nt_device.py).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/rtd.h"

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rtd_last_error()); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

typedef std::vector<double> vec;

// wfull [R][L][nall] = (2k + 1) x (k == 0 ? g0 : 0.5)
static bool weighted(const vec& w, int nall, double g0) {
  for (size_t i = 0; i < w.size(); ++i) {
    const int k = (int)(i % nall);
    if (w[i] != (2.0 * k + 1.0) * (k == 0 ? g0 : 0.5)) return false;
  }
  return true;
}
static bool all_finite(const vec& v) {
  for (double y : v)
    if (!std::isfinite(y)) return false;
  return true;
}

// kind 0: one window; 1: windows of 4 columns; 2: the same, retained.  band: the columns are 3 profiles x 5 spectral points
static int scenario(int kind, bool band, bool thermal) {
  const int P = 3, G = 5, S = 2, L = 3, C = P * G, nquad = 8, N = 4, M = 2, nleg = 8, nall = 12;
  rtd_dims dims = {C, L, nquad, nleg, M, thermal ? 2 : 0, 0, 1};
  rtd_plan* p = nullptr;
  if (kind == 0) CHECK(rtd_plan_create(&dims, 0, &p) == 0);
  else if (kind == 1) CHECK(rtd_plan_create_windowed(&dims, 0, 4, &p) == 0);
  else CHECK(rtd_plan_create_retained_form(&dims, 0, 4, (int64_t)1 << 30, 1, &p) == 0);
  vec mu(N), wq(N, 1.0 / N);
  for (int i = 0; i < N; ++i) mu[i] = (i + 0.5) / N;
  CHECK(rtd_plan_set_quadrature(p, mu.data(), wq.data()) == 0);
  vec abs_(P * G * L, 0.2), dspec(P * L * S, 0.1), ospec(P * L * S, 0.7), lspec(S * nall, 0.5);
  for (int s = 0; s < S; ++s) lspec[s * nall] = 1.0;
  rtd_band bd = {P, G, S, nall, 1, abs_.data(), dspec.data(), ospec.data(), lspec.data()};
  vec tau(C * L), om(C * L, 0.6), f(C * L, 0.1), leg(C * L * nall, 0.5), mu0(C, 0.6), I0(C, 1.0), phi0(C, 0.1), bp(C * M * N, 0.25);
  for (int c = 0; c < C; ++c)
    for (int l = 0; l < L; ++l) tau[c * L + l] = 0.3 * (l + 1) + 0.01 * c;
  vec temper(C * (L + 1), 250.0), lo(C, 300.0), hi(C, 800.0), bt(C, 290.0), sp(C * L * 2, 0.0);
  rtd_thermal th = {temper.data(), lo.data(), hi.data(), bt.data(), nullptr, nullptr, nullptr};
  vec tau_out(C * L, -1.0);
  auto upload = [&](int32_t nleg_all) -> int {
    if (band) return rtd_plan_set_columns_band(p, &bd, mu0.data(), I0.data(), phi0.data(), bp.data(), nullptr, nullptr, nullptr, thermal ? &th : nullptr, tau_out.data());
    if (thermal)
      return rtd_plan_set_columns_thermal(p, tau.data(), om.data(), leg.data(), nleg_all, f.data(), mu0.data(), I0.data(), phi0.data(), bp.data(), nullptr,
                                          nullptr, nullptr, &th);
    return rtd_plan_set_columns_raw(p, tau.data(), om.data(), leg.data(), nleg_all, f.data(), mu0.data(), I0.data(), phi0.data(), bp.data(), nullptr, nullptr,
                                    nullptr, nullptr);
  };
  int32_t rows = -1;
  // no request: nothing is held
  CHECK(upload(nall) == 0);
  CHECK(rtd_plan_get_nt(p, nullptr, nullptr, nullptr, nullptr, &rows) == RTD_ERR_STATE);
  int64_t bytes0 = 0, bytes1 = 0;
  CHECK(rtd_plan_device_bytes(p, &bytes0) == 0);
  // requests that do not fit the columns
  CHECK(rtd_plan_request_nt(p, nall + 1) == 0 && upload(nall) == RTD_ERR_ARG);
  CHECK(rtd_plan_request_nt(p, nleg) == 0 && upload(band ? nall : nleg) == RTD_ERR_ARG);  // not above nleg (a band: not its nleg_all)
  if (band) {
    CHECK(rtd_plan_request_nt(p, nall) == 0);
    bd.delta_m = 0;
    CHECK(upload(nall) == RTD_ERR_ARG);
    bd.delta_m = 1;
  }
  CHECK(rtd_plan_device_bytes(p, &bytes1) == 0 && bytes1 == bytes0);  // refused before anything was allocated
  CHECK(rtd_plan_request_nt(p, nall) == 0);
  {
    vec so(C * L, 0.5), t0(C * (L + 1), 0.0), sc(C * L, 1.0), wl(C * L * nleg, 0.1), resc(C, 1.0);
    for (int c = 0; c < C; ++c)
      for (int l = 0; l < L; ++l) t0[c * (L + 1) + l + 1] = tau[c * L + l];
    CHECK(rtd_plan_set_columns(p, so.data(), tau.data(), t0.data(), sc.data(), wl.data(), mu0.data(), I0.data(), phi0.data(), resc.data(), nullptr, nullptr,
                               thermal ? sp.data() : nullptr, nullptr, nullptr) == RTD_ERR_STATE);
  }
  for (int pass = 0; pass < 2; ++pass) {  // twice: the buffers are reused, not grown again
    CHECK(upload(nall) == 0);
    CHECK(rtd_plan_device_bytes(p, &bytes1) == 0 && bytes1 > bytes0);
    const int R = band ? P : C;
    vec w(R * L * nall, -1.0), ff(C * L, -1.0), ic(C * nall, -1.0), ip(C * 2, -1.0);
    CHECK(rtd_plan_get_nt(p, w.data(), ff.data(), ic.data(), ip.data(), &rows) == 0 && rows == R);
    CHECK(weighted(w, nall, band ? 1.0 : 0.5) && all_finite(ic) && all_finite(ip) && all_finite(ff));
    for (int c = 0; c < C; ++c) CHECK(ip[2 * c] > 0.5 && ip[2 * c + 1] > 0.0);  // (the shadow preparation leaves mu0 = I0 = 0.5)
    for (int c = 0; c < C; ++c)
      for (int k = 0; k < nleg; ++k) CHECK(ic[c * nall + k] == (2.0 * k + 1.0));  // r_k = sum f w / sum f w = 1 below nleg
    if (!band) CHECK(ff == f);
    CHECK(rtd_plan_get_nt(p, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    // evaluation through every window, the three orders, with and without the corrections
    const int nt = L + 1, np = 2;
    vec lev(C * nt, 0.0), phi = {0.0, 1.0}, u(C * nquad * nt * np);
    for (int c = 0; c < C; ++c)
      for (int l = 0; l < L; ++l) lev[c * nt + 1 + l] = band ? tau_out[c * L + l] : tau[c * L + l];
    if (band) continue;
    CHECK(rtd_plan_solve(p) == 0);
    for (int flags : {0, 1, 4, 2})
      CHECK(rtd_plan_evaluate(p, nt, lev.data(), np, phi.data(), flags, u.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(rtd_plan_set_eval_points(p, nt, lev.data(), np, phi.data()) == 0);
    CHECK(rtd_plan_run_fetch(p, u.data(), nullptr, nullptr, nullptr, nullptr) == 0);
  }
  // off until the next columns; the request withdrawn: off for good, and the host-prepared upload is taken again
  CHECK(rtd_plan_set_nt(p, 0, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(rtd_plan_get_nt(p, nullptr, nullptr, nullptr, nullptr, &rows) == RTD_ERR_STATE);
  CHECK(upload(nall) == 0 && rtd_plan_get_nt(p, nullptr, nullptr, nullptr, nullptr, &rows) == 0);
  CHECK(rtd_plan_request_nt(p, 0) == 0 && rtd_plan_set_nt(p, 0, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(upload(nall) == 0 && rtd_plan_get_nt(p, nullptr, nullptr, nullptr, nullptr, &rows) == RTD_ERR_STATE);
  CHECK(rtd_plan_destroy(p) == 0);
  return 0;
}

int main() {
  for (int kind = 0; kind < 3; ++kind)
    for (int band = 0; band < 2; ++band)
      for (int thermal = 0; thermal < 2; ++thermal)
        if (scenario(kind, band != 0, thermal != 0)) return 1;
  {  // a plan without a beam refuses, as rtd_plan_set_nt does
    rtd_dims dims = {2, 1, 4, 4, 1, 0, 0, 0};
    rtd_plan* p = nullptr;
    CHECK(rtd_plan_create(&dims, 0, &p) == 0);
    vec mu = {0.25, 0.75}, w = {0.5, 0.5}, one(2, 0.5), zero(2, 0.0), leg(2 * 6, 0.5);
    CHECK(rtd_plan_set_quadrature(p, mu.data(), w.data()) == 0);
    CHECK(rtd_plan_request_nt(p, 6) == 0);
    CHECK(rtd_plan_set_columns_raw(p, one.data(), one.data(), leg.data(), 6, one.data(), one.data(), zero.data(), zero.data(), nullptr, nullptr, nullptr,
                                   nullptr, nullptr) == RTD_ERR_ARG);
    CHECK(rtd_plan_destroy(p) == 0);
  }
  CHECK(rtd_plan_request_nt(nullptr, 4) == RTD_ERR_ARG);
  CHECK(rtd_plan_get_nt(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  std::printf("NT REQUEST HOST OK\n");
  return 0;
}
