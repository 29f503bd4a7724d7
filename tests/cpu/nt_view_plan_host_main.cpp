// TEST PROGRAM (tests/test_nt_view_plan_host_sanitized_cpu.py): rtd_plan_set_view_nt and what it changes in the windows of an evaluation
// and in the two view fetches (csrc/rtd_api.hip), over the stand-in runtime of fake_hip/ and the shadow launchers of
// host_asan_shadow.cpp, as a stand-alone program under the address / undefined-behaviour sanitizers.  A host compiler takes
// csrc/rtd_nt_view.hip into rtd_api.hip's unit, so rtd_nt_view_tables_kernel and rtd_nt_view_apply_kernel RUN here, thread by thread on
// heap memory, as do the view's basis and apply kernels: the window's slice of the view buffer, the one-window table of the other-layer
// sums, the angles per column or shared and every row the kernels read of the plan's buffers are bounds-checked.  Values are the shadow
// launchers' constants: only finiteness and the identities that do not depend on them are checked by value.
// (A band plan is not evaluated here, for the reason tests/cpu/nt_request_host_main.cpp gives; rows shared by the columns of a profile
// are bounds-checked by tests/cpu/nt_view_host_main.cpp.)
#include <cmath>
#include <cstdio>
#include <cstring>
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

static bool all_finite(const vec& v) {
  for (double y : v)
    if (!std::isfinite(y)) return false;
  return true;
}

// kind 0: one window; 1: windows of 4 columns; 2: the same, retained in full; 3: retained lean
static int scenario(int kind, bool per_column, bool with_nt) {
  const int L = 3, C = 10, nquad = 8, N = 4, M = 2, nleg = 8, nall = 12, nmu = 5;
  rtd_dims dims = {C, L, nquad, nleg, M, 0, 0, 1};
  rtd_plan* p = nullptr;
  if (kind == 0) CHECK(rtd_plan_create(&dims, 0, &p) == 0);
  else if (kind == 1) CHECK(rtd_plan_create_windowed(&dims, 0, 4, &p) == 0);
  else CHECK(rtd_plan_create_retained_form(&dims, 0, 4, (int64_t)1 << 30, kind == 2 ? 1 : 2, &p) == 0);
  vec mu(N), wq(N, 1.0 / N);
  for (int i = 0; i < N; ++i) mu[i] = (i + 0.5) / N;
  CHECK(rtd_plan_set_quadrature(p, mu.data(), wq.data()) == 0);
  vec tau(C * L), om(C * L, 0.6), f(C * L, 0.1), leg(C * L * nall, 0.5), mu0(C, 0.6), I0(C, 1.0), phi0(C, 0.1), bp(C * M * N, 0.25);
  for (int c = 0; c < C; ++c)
    for (int l = 0; l < L; ++l) tau[c * L + l] = 0.3 * (l + 1) + 0.01 * c;
  if (with_nt) CHECK(rtd_plan_request_nt(p, nall) == 0);
  CHECK(rtd_plan_set_columns_raw(p, tau.data(), om.data(), leg.data(), nall, f.data(), mu0.data(), I0.data(), phi0.data(), bp.data(), nullptr, nullptr,
                                 nullptr, nullptr) == 0);
  // angles: general, a node, +-1, the shadow preparation's mu0 = 0.5 exactly (the coincidence) -- shared, or shifted per column
  const double base[nmu] = {0.3, mu[1], -1.0, -0.5, 1.0};
  vec ang((per_column ? C : 1) * nmu);
  for (size_t i = 0; i < ang.size(); ++i) ang[i] = base[i % nmu] * ((i / nmu) % 2 ? 0.999 : 1.0);
  vec zero = ang;
  zero[1] = -0.0;

  // the refusals of the mode, before anything is evaluated
  CHECK(rtd_plan_set_view_nt(nullptr, 1) == RTD_ERR_ARG && rtd_plan_set_view_nt(p, 2) == RTD_ERR_ARG && rtd_plan_set_view_nt(p, -1) == RTD_ERR_ARG);
  CHECK(rtd_plan_set_view_mu(p, nmu, zero.data(), per_column) == 0);  // mode 0 takes mu = 0 ...
  CHECK(rtd_plan_set_view_nt(p, 1) == RTD_ERR_ARG);                   // ... and mode 1 is refused while it is among the angles
  CHECK(rtd_plan_set_view_mu(p, nmu, ang.data(), per_column) == 0 && rtd_plan_set_view_nt(p, 1) == 0);
  CHECK(rtd_plan_set_view_mu(p, nmu, zero.data(), per_column) == RTD_ERR_ARG);  // refused: the earlier angles stand
  CHECK(std::strstr(rtd_last_error(), "mu = 0") != nullptr);
  CHECK(rtd_plan_set_view_nt(p, 0) == 0);

  const int nt = L + 1, np = 2;
  vec lev(C * nt, 0.0), phi = {0.1, 1.0}, u(C * nquad * nt * np), u0(C * nquad * nt);
  for (int c = 0; c < C; ++c)
    for (int l = 0; l < L; ++l) lev[c * nt + 1 + l] = tau[c * L + l];
  vec v0(C * nmu * nt * np), v1(v0.size()), w0(C * nmu * nt), w1(w0.size());
  int64_t bytes0 = 0, bytes1 = 0, bytes2 = 0;
  CHECK(rtd_plan_solve(p) == 0);
  // mode 0: the interpolated view; the plan then holds what it holds without the new symbol
  CHECK(rtd_plan_evaluate(p, nt, lev.data(), np, phi.data(), 0, u.data(), u0.data(), nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(rtd_plan_fetch_view(p, v0.data(), w0.data()) == 0 && all_finite(v0) && all_finite(w0));
  CHECK(rtd_plan_device_bytes(p, &bytes0) == 0);
  // mode 1, set after the evaluation: the view of u waits for the next one, u0_mu is served
  CHECK(rtd_plan_set_view_nt(p, 1) == 0);
  if (with_nt) {
    CHECK(rtd_plan_fetch_view(p, v1.data(), nullptr) == RTD_ERR_STATE && std::strstr(rtd_last_error(), "evaluate again") != nullptr);
    CHECK(rtd_plan_fetch_view(p, nullptr, w1.data()) == 0 && w1 == w0);
  }
  for (int flags : {0, 1, 4, 8, 2}) {  // value, antiderivative, derivative, u kept on the device, corrections skipped
    vec uu(u.size());
    CHECK(rtd_plan_evaluate(p, nt, lev.data(), np, phi.data(), flags, flags == 8 ? nullptr : uu.data(), u0.data(), nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(rtd_plan_fetch_view(p, v1.data(), w1.data()) == 0 && all_finite(v1) && all_finite(w1));
    if (flags == 0) CHECK(uu == u);                   // u itself keeps its bits
    if (flags == 0 || flags == 8) CHECK(w1 == w0);   // and so does the view of u0
    if (!with_nt && flags == 0) CHECK(v1 == v0);     // a plan without corrections ignores the mode
  }
  CHECK(rtd_plan_device_bytes(p, &bytes1) == 0 && (with_nt ? bytes1 > bytes0 : bytes1 == bytes0));  // the table, only when it is used
  // new angles after an evaluation with the corrections: refused until the next one, in every entry
  CHECK(rtd_plan_evaluate(p, nt, lev.data(), np, phi.data(), 0, u.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(rtd_plan_set_view_mu(p, nmu, ang.data(), per_column) == 0);
  CHECK(rtd_plan_fetch_view(p, v1.data(), nullptr) == (with_nt ? RTD_ERR_STATE : 0));
  CHECK(rtd_plan_set_eval_points(p, nt, lev.data(), np, phi.data()) == 0);
  for (int order : {0, -1, 1}) {
    CHECK(rtd_plan_set_eval_order(p, order) == 0);
    CHECK(rtd_plan_run(p) == 0 && rtd_plan_fetch_view(p, v1.data(), w1.data()) == 0 && all_finite(v1));
    CHECK(rtd_plan_run_fetch(p, u.data(), nullptr, nullptr, nullptr, nullptr) == 0 && rtd_plan_fetch_view(p, v1.data(), nullptr) == 0 && all_finite(v1));
  }
  CHECK(rtd_plan_device_bytes(p, &bytes2) == 0 && bytes2 == bytes1);  // nothing grows from run to run
  // the request withdrawn and made again in mode 1
  CHECK(rtd_plan_set_view_mu(p, 0, nullptr, 0) == 0 && rtd_plan_fetch_view(p, v1.data(), nullptr) == RTD_ERR_STATE);
  CHECK(rtd_plan_set_view_mu(p, 2, ang.data(), 0) == 0 && rtd_plan_run(p) == 0);
  vec small(C * 2 * nt * np);
  CHECK(rtd_plan_fetch_view(p, small.data(), nullptr) == 0 && all_finite(small));
  CHECK(rtd_plan_destroy(p) == 0);
  return 0;
}

int main() {
  for (int kind = 0; kind < 4; ++kind)
    for (int per_column = 0; per_column < 2; ++per_column)
      for (int with_nt = 0; with_nt < 2; ++with_nt)
        if (scenario(kind, per_column != 0, with_nt != 0)) return 1;
  std::printf("NT VIEW PLAN HOST OK\n");
  return 0;
}
