// TEST PROGRAM (tests/test_actinic_host_sanitized_cpu.py): the actinic-flux entry points -- rtd_plan_fetch_actinic,
// rtd_plan_fetch_band_actinic (csrc/rtd_api.hip) -- over the stand-in runtime of fake_hip/ and the shadow launchers of
// host_asan_shadow.cpp, as a stand-alone program under the address / undefined-behaviour sanitizers.  rtd_actinic_kernel and
// rtd_band_reduce_kernel belong to rtd_api.hip itself, so they RUN here, thread by thread, on heap memory: every index they form
// is bounds-checked, and every element they write is recomputed in long double from the u0 fetched from the same plan and the
// inputs this program uploaded.  What the VALUES can show here is limited: the shadow evaluation launcher fills u0 with one
// constant, so a wrong stream index, stride or permutation in the kernel's u0 reads gives the same sums and only the sanitizer's
// bounds check sees it (the GPU test holds the sums to exact rational sums of a real u0).  The R / D part is checked by value:
// scale_tau, mu0, I0 and rescale differ from column to column, so a wrong column or layer index there is a wrong number.  All
// caller arrays are heap blocks of exactly the documented extent.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

static const int P = 3, G = 5, C = P * G, L = 3, NQ = 8, N = 4, M = 2, NLEG = 8, K = 2;
static const long double PI_L = 3.14159265358979323846264338327950288L;

struct Cols {
  vec mu, wq, om, tau, ts0, sc, wl, mu0, I0, phi0, resc;
};

static Cols make_cols(bool beam) {
  Cols c{vec(N), vec(N), vec(C * L), vec(C * L), vec(C * (L + 1), 0.0), vec(C * L), vec(C * L * NLEG, 0.1), vec(C), vec(C), vec(C, 0.1), vec(C)};
  for (int i = 0; i < N; ++i) {
    c.mu[i] = (i + 0.5) / N;
    c.wq[i] = 0.1 * (i + 1);
  }
  for (int k = 0; k < C; ++k) {
    c.mu0[k] = 0.3 + 0.04 * k;
    c.resc[k] = 1.0 + 0.25 * (k % 4);
    c.I0[k] = (!beam || k == 7) ? 0.0 : 1.0 / c.resc[k];  // (the prepared I0: the caller's divided by rescale)
    double t = 0.0;
    for (int l = 0; l < L; ++l) {
      const double dt = 0.2 + 0.05 * ((k + 2 * l) % 5);
      t += dt;
      c.om[k * L + l] = 0.03 + 0.06 * k;
      c.tau[k * L + l] = t;
      c.sc[k * L + l] = k == 3 ? 1.0 : 0.75 + 0.01 * (k + l);  // (column 3: no delta-M scaling)
      c.ts0[k * (L + 1) + l + 1] = c.ts0[k * (L + 1) + l] + dt * c.sc[k * L + l];
    }
  }
  return c;
}

// every element of the three arrays against the definitions of include/rtd.h in long double, from the u0 of the same plan
static int check_actinic(const Cols& in, bool beam, int order, int nt, const vec& tau, const vec& u0, const vec* act[3]) {
  const long double u = std::ldexp(1.0L, -53);
  for (int c = 0; c < C; ++c)
    for (int t = 0; t < nt; ++t) {
      long double up = 0.0L, dn = 0.0L, aup = 0.0L, adn = 0.0L;
      for (int i = 0; i < N; ++i) {
        const long double a = (long double)in.wq[i] * u0[(c * NQ + i) * nt + t], b = (long double)in.wq[i] * u0[(c * NQ + N + i) * nt + t];
        up += a; dn += b; aup += std::fabs(a); adn += std::fabs(b);
      }
      up *= 2 * PI_L; dn *= 2 * PI_L; aup *= 2 * PI_L; adn *= 2 * PI_L;
      long double R = 0.0L, D = 0.0L, aR = 0.0L;
      const long double I0 = beam ? (long double)in.resc[c] * in.I0[c] : 0.0L;
      if (I0 != 0.0L) {
        const long double x = tau[c * nt + t], mu0 = in.mu0[c];
        int l = 0;
        while (l < L - 1 && !(x <= in.tau[c * L + l])) ++l;
        const long double sc = in.sc[c * L + l], far = ((long double)in.tau[c * L + l] - x) * sc;
        const long double ts = in.ts0[c * (L + 1) + l + 1] - far, X = (in.ts0[c * (L + 1) + l + 1] + far) / mu0;
        long double es = I0 * std::exp(-ts / mu0), ed = I0 * std::exp(-x / mu0);
        if (order < 0) { es /= (-sc / mu0); ed *= -mu0; }
        else if (order > 0) { es *= (-sc / mu0); ed /= -mu0; }
        R = es - ed;
        D = ed;
        aR = (8 + 4 * X) * (std::fabs(es) + std::fabs(ed));  // (roundings counted in tests/test_gpu_actinic.py)
      }
      const long o = (long)c * nt + t;
      if (act[0]) CHECK(std::fabs((*act[0])[o] - up) <= (N + 2) * u * aup);
      if (act[1]) CHECK(std::fabs((*act[1])[o] - (dn + R)) <= u * ((N + 2) * adn + aR + std::fabs(dn + R)));
      if (act[2]) CHECK(std::fabs((*act[2])[o] - D) <= u * aR);
      if (I0 == 0.0L) {
        if (act[2]) CHECK((*act[2])[o] == 0.0);
      } else if (act[2]) CHECK((*act[2])[o] != 0.0);
    }
  return 0;
}

static int check_reduced(const vec& w, int nt, const vec& full, const vec& red) {
  for (int p = 0; p < P; ++p)
    for (int k = 0; k < K; ++k)
      for (int t = 0; t < nt; ++t) {
        long double want = 0.0L, size = 0.0L;
        for (int g = 0; g < G; ++g) {
          const long double x = (long double)w[k * G + g] * full[(p * G + g) * nt + t];
          want += x;
          size += std::fabs(x);
        }
        CHECK(std::fabs((long double)red[(p * K + k) * nt + t] - want) <= std::ldexp(1.0L, -52) * std::fabs(want) + std::ldexp(1.0L, -60) * size);
      }
  return 0;
}

// fetch the three arrays, every pointer NULL in turn, and hold them; then the reduced ones
static int fetch_and_check(rtd_plan* p, const Cols& in, bool beam, int order, int nt, const vec& tau, const vec& wb) {
  vec u0(C * NQ * nt, -7.0), a0(C * nt, -7.0), a1(C * nt, -7.0), a2(C * nt, -7.0);
  CHECK(rtd_plan_fetch(p, nullptr, u0.data(), nullptr, nullptr, nullptr) == 0);
  CHECK(rtd_plan_fetch_actinic(p, a0.data(), a1.data(), a2.data()) == 0);
  const vec* all[3] = {&a0, &a1, &a2};
  if (check_actinic(in, beam, order, nt, tau, u0, all)) return 1;
  for (int skip = 0; skip < 4; ++skip) {  // every pointer NULL in turn, then all of them
    vec b0(C * nt, -7.0), b1(C * nt, -7.0), b2(C * nt, -7.0);
    CHECK(rtd_plan_fetch_actinic(p, skip == 0 || skip == 3 ? nullptr : b0.data(), skip == 1 || skip == 3 ? nullptr : b1.data(),
                                 skip == 2 || skip == 3 ? nullptr : b2.data()) == 0);
    if (skip != 0 && skip != 3) CHECK(b0 == a0);
    if (skip != 1 && skip != 3) CHECK(b1 == a1);
    if (skip != 2 && skip != 3) CHECK(b2 == a2);
  }
  vec r0(P * K * nt, -7.0), r1(P * K * nt, -7.0), r2(P * K * nt, -7.0);
  CHECK(rtd_plan_fetch_band_actinic(p, r0.data(), r1.data(), r2.data()) == 0);
  if (check_reduced(wb, nt, a0, r0) || check_reduced(wb, nt, a1, r1) || check_reduced(wb, nt, a2, r2)) return 1;
  for (int skip = 0; skip < 4; ++skip) {
    vec s0(P * K * nt, -7.0), s1(P * K * nt, -7.0), s2(P * K * nt, -7.0);
    CHECK(rtd_plan_fetch_band_actinic(p, skip == 0 || skip == 3 ? nullptr : s0.data(), skip == 1 || skip == 3 ? nullptr : s1.data(),
                                      skip == 2 || skip == 3 ? nullptr : s2.data()) == 0);
    if (skip != 0 && skip != 3) CHECK(s0 == r0);
    if (skip != 1 && skip != 3) CHECK(s1 == r1);
    if (skip != 2 && skip != 3) CHECK(s2 == r2);
  }
  return 0;
}

// kind 0: plan of one window; 1: windows of 4 columns (C = 15, G = 5: 4 divides neither); 2: the same, retained
static int plan_scenario(int kind, bool beam) {
  rtd_dims dims = {C, L, NQ, NLEG, M, 0, 0, beam ? 1 : 0};
  rtd_plan* p = nullptr;
  if (kind == 0) CHECK(rtd_plan_create(&dims, 0, &p) == 0);
  else if (kind == 1) CHECK(rtd_plan_create_windowed(&dims, 0, 4, &p) == 0);
  else CHECK(rtd_plan_create_retained_form(&dims, 0, 4, (int64_t)1 << 30, 1, &p) == 0);
  int32_t wc = 0, nw = 0;
  CHECK(rtd_plan_windows(p, &wc, &nw) == 0 && (kind == 0 ? nw == 1 : (wc == 4 && nw == 4)));
  const Cols in = make_cols(beam);
  vec one(C, 0.5), out(C * 2);
  CHECK(rtd_plan_fetch_actinic(p, out.data(), nullptr, nullptr) == RTD_ERR_STATE);  // nothing uploaded, nothing solved
  CHECK(rtd_plan_set_quadrature(p, in.mu.data(), in.wq.data()) == 0);
  CHECK(rtd_plan_set_columns(p, in.om.data(), in.tau.data(), in.ts0.data(), in.sc.data(), in.wl.data(), in.mu0.data(), in.I0.data(),
                             in.phi0.data(), in.resc.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  int64_t bytes0 = 0, bytes1 = 0;
  CHECK(rtd_plan_solve(p) == 0 && rtd_plan_synchronize(p) == 0);
  CHECK(rtd_plan_fetch_actinic(p, out.data(), nullptr, nullptr) == RTD_ERR_STATE);  // solved, nothing evaluated
  const int ntL = L + 1, nphi = 2;
  vec lev(C * ntL, 0.0), phi = {0.0, 1.0};
  for (int c = 0; c < C; ++c)
    for (int l = 0; l < L; ++l) lev[c * ntL + 1 + l] = in.tau[c * L + l];
  CHECK(rtd_plan_set_eval_points(p, ntL, lev.data(), nphi, phi.data()) == 0);
  CHECK(rtd_plan_fetch_actinic(p, out.data(), nullptr, nullptr) == RTD_ERR_STATE);  // points stored, nothing evaluated at them
  CHECK(rtd_plan_run(p) == 0);
  CHECK(rtd_plan_device_bytes(p, &bytes0) == 0);
  CHECK(rtd_plan_fetch_band_actinic(p, out.data(), nullptr, nullptr) == RTD_ERR_STATE);  // no weights
  CHECK(rtd_plan_device_bytes(p, &bytes1) == 0 && bytes1 == bytes0);                      // (and nothing was allocated for it)
  vec wb(K * G);
  for (int i = 0; i < K * G; ++i) wb[i] = (i % 3 == 1 ? -1.0 : 1.0) * std::pow(10.0, -3.0 + 6.0 * std::fabs(std::sin(1.0 + i)));
  CHECK(rtd_plan_set_band_weights(p, G, K, wb.data()) == 0);
  CHECK(rtd_plan_device_bytes(p, &bytes0) == 0);

  // interior points, an interface and the bottom
  const int nt = 4;
  vec sub(C * nt);
  for (int c = 0; c < C; ++c) {
    sub[c * nt] = 0.5 * in.tau[c * L];
    sub[c * nt + 1] = in.tau[c * L + 1];
    sub[c * nt + 2] = in.tau[c * L + 1] + 0.3 * (in.tau[c * L + 2] - in.tau[c * L + 1]);
    sub[c * nt + 3] = in.tau[c * L + 2];
  }
  for (int order : {0, -1, 1}) {
    // run + fetch at the interfaces
    CHECK(rtd_plan_set_eval_order(p, order) == 0);
    CHECK(rtd_plan_set_eval_points(p, ntL, lev.data(), nphi, phi.data()) == 0);
    CHECK(rtd_plan_run(p) == 0);
    if (fetch_and_check(p, in, beam, order, ntL, lev, wb)) return 1;
    // run_fetch
    vec fu(C * ntL);
    CHECK(rtd_plan_run_fetch(p, nullptr, nullptr, fu.data(), nullptr, nullptr) == 0);
    if (fetch_and_check(p, in, beam, order, ntL, lev, wb)) return 1;
    // evaluate and evaluate_band with the flag word, whatever the stored order
    const int flags = order < 0 ? 1 : order > 0 ? 4 : 0;
    CHECK(rtd_plan_set_eval_order(p, -order) == 0);
    vec eu0(C * NQ * nt);
    CHECK(rtd_plan_evaluate(p, nt, sub.data(), 0, nullptr, flags, nullptr, eu0.data(), nullptr, nullptr, nullptr, nullptr) == 0);
    if (fetch_and_check(p, in, beam, order, nt, sub, wb)) return 1;
    CHECK(rtd_plan_evaluate(p, nt, sub.data(), 0, nullptr, flags, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);  // nothing wanted but the actinic fluxes
    if (fetch_and_check(p, in, beam, order, nt, sub, wb)) return 1;
    vec bfu(P * K * nt);
    CHECK(rtd_plan_evaluate_band(p, nt, sub.data(), nphi, phi.data(), flags, nullptr, nullptr, bfu.data(), nullptr, nullptr) == 0);
    if (fetch_and_check(p, in, beam, order, nt, sub, wb)) return 1;
  }
  CHECK(rtd_plan_device_bytes(p, &bytes1) == 0 && bytes1 > bytes0);  // (the actinic buffers came with the first fetch)
  CHECK(rtd_plan_solve(p) == 0);
  CHECK(rtd_plan_fetch_actinic(p, out.data(), nullptr, nullptr) == RTD_ERR_STATE);  // a new solve: the buffers are an earlier one's
  if (kind == 0) {
    // the layer-shard path marks the plan solved without rtd_plan_solve: the buffers of the evaluation before the new columns
    // must not be combined with the new columns' tau, taus0, scale, mu0 and I0
    vec a0(C * nt);
    CHECK(rtd_plan_evaluate(p, nt, sub.data(), 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(rtd_plan_fetch_actinic(p, a0.data(), nullptr, nullptr) == 0);
    CHECK(rtd_plan_set_columns(p, in.om.data(), in.tau.data(), in.ts0.data(), in.sc.data(), in.wl.data(), in.mu0.data(), in.I0.data(),
                               in.phi0.data(), in.resc.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(rtd_plan_fetch_actinic(p, a0.data(), nullptr, nullptr) == RTD_ERR_STATE);
    CHECK(rtd_plan_solve_layers(p, 0, L) == 0 && rtd_plan_solve_bc(p) == 0);
    CHECK(rtd_plan_fetch_actinic(p, a0.data(), nullptr, nullptr) == RTD_ERR_STATE);
    CHECK(rtd_plan_fetch_band_actinic(p, out.data(), nullptr, nullptr) == RTD_ERR_STATE);
  }
  CHECK(rtd_plan_set_band_weights(p, 0, 0, nullptr) == 0);
  CHECK(rtd_plan_fetch_band_actinic(p, out.data(), nullptr, nullptr) == RTD_ERR_STATE);
  CHECK(rtd_plan_destroy(p) == 0);
  return 0;
}

int main() {
  for (int kind = 0; kind < 3; ++kind)
    for (int beam = 1; beam >= 0; --beam)
      if (plan_scenario(kind, beam != 0)) return 1;
  CHECK(rtd_plan_fetch_actinic(nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_fetch_band_actinic(nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  std::printf("ACTINIC HOST OK\n");
  return 0;
}
