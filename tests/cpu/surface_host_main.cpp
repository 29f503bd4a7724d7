// TEST PROGRAM (tests/test_surface_host_sanitized_cpu.py): rtd_plan_request_surface, rtd_surface_samples and rtd_plan_get_bdrf and what
// the request changes in rtd_plan_set_columns_raw, _thermal and _band (csrc/rtd_api.hip), over the stand-in runtime of fake_hip/ and
// the shadow launchers of host_asan_shadow.cpp, as a stand-alone program under the address / undefined-behaviour sanitizers.
// rtd_surface_samples_kernel and rtd_surface_lambert_kernel belong to rtd_api.hip itself, so they RUN here, thread by thread, on heap
// memory: the scratch block, its carve for the parameters, the chunk loop and the shifted descriptors are bounds-checked -- the shadow
// of rtd_bdrf_modes_kernel reads exactly the samples of its view's columns and writes 0.5 into exactly their tables, so a chunk that
// is skipped leaves zeros and a descriptor that is off is a sanitizer report.  Lambert's tables and the plan-free samples are checked
// by value: every sample is recomputed here in long double from the formulas of include/rtd.h.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
typedef long double ld;

// rho in long double, from the chords (the arccos form would lose half of long double's digits at the hot spot too); *unclamped too
static ld rho_ld(int model, const double* par, ld mu, ld mup, int p, int nphi, ld* unclamped) {
  const ld pi = 3.14159265358979323846264338327950288L;
  const ld ang = 2.0L * pi * (ld)p / (ld)nphi, c = cosl(ang), s = sinl(ang);
  const ld sm = sqrtl((1 - mu) * (1 + mu)), sp = sqrtl((1 - mup) * (1 + mup));
  const ld h = 0.5L * ((sm * c + sp) * (sm * c + sp) + sm * s * sm * s + (mu - mup) * (mu - mup));
  const ld cosxi = 1 - h, g = 2 - h;
  ld r;
  if (model == RTD_SURFACE_LAMBERT) {
    r = par[0];
  } else if (model == RTD_SURFACE_HAPKE) {
    const ld B0 = par[0], HH = par[1], W = par[2], B = B0 * HH / (HH + sqrtl(h / g)), gam = sqrtl(1 - W);
    r = W / 4 / (mu + mup) * ((1 + B) * (1 + cosxi / 2) + (1 + 2 * mup) / (1 + 2 * mup * gam) * (1 + 2 * mu) / (1 + 2 * mu * gam) - 1);
  } else {
    const ld ti = sm / mu, tv = sp / mup, sec = 1 / mu + 1 / mup, D2 = (ti - tv) * (ti - tv) + 2 * ti * tv * (1 + c);
    if (model == RTD_SURFACE_ROSSLI) {
      const ld xi = 2 * asinl(sqrtl(h / 2)), Kvol = ((pi / 2 - xi) * cosxi + sqrtl(h * g)) / (mu + mup) - pi / 4;
      ld cost = 2 * sqrtl(D2 + ti * tv * s * ti * tv * s) / sec;
      if (cost > 1) cost = 1;
      const ld t = acosl(cost), O = (t - sinl(t) * cost) * sec / pi, Kgeo = O - sec + (1 + cosxi) / (2 * mu * mup);
      r = par[0] + par[1] * Kvol + par[2] * Kgeo;
    } else {
      const ld rho0 = par[0], k = par[1], Th = par[2], rhoc = par[3];
      r = rho0 * powl(mu * mup * (mu + mup), k - 1) * (1 - Th * Th) / powl(1 + Th * Th + 2 * Th * cosxi, 1.5L) * (1 + (1 - rhoc) / (1 + sqrtl(D2)));
    }
  }
  *unclamped = r;
  return model == RTD_SURFACE_ROSSLI && r < 0 ? 0 : r;
}

static int plan_free() {
  const int nphi = 24;
  const double mus[] = {0.0199, 0.1, 0.3, 0.5, 0.77, 1.0};
  const struct { int model; double par[4]; } cases[] = {{RTD_SURFACE_LAMBERT, {0.25, 0, 0, 0}}, {RTD_SURFACE_HAPKE, {1.0, 0.06, 0.6, 0}},
      {RTD_SURFACE_ROSSLI, {0.3, 0.1, 0.05, 0}}, {RTD_SURFACE_RPV, {0.1, 0.8, -0.1, 0.1}}, {RTD_SURFACE_RPV, {0.3, 1.2, 0.25, 0.6}}};
  for (const char* bytes : {"", "1", "1000"}) {  // the default block; one row per pass; a few rows per pass
    if (*bytes) setenv("RTD_SURFACE_BYTES", bytes, 1);
    else unsetenv("RTD_SURFACE_BYTES");
    for (const auto& cs : cases) {
      vec par, mu, mup;
      for (double a : mus)
        for (double b : mus) { mu.push_back(a); mup.push_back(b); par.insert(par.end(), cs.par, cs.par + 4); }
      const int n = (int)mu.size();
      vec rho((size_t)n * nphi, -7.0);
      CHECK(rtd_surface_samples(0, cs.model, n, par.data(), mu.data(), mup.data(), nphi, rho.data()) == 0);
      double worst = 0.0;
      for (int r = 0; r < n; ++r) {
        ld scale = 0;
        std::vector<ld> want((size_t)nphi);
        for (int p = 0; p < nphi; ++p) {
          ld u;
          want[(size_t)p] = rho_ld(cs.model, cs.par, mu[r], mup[r], p, nphi, &u);
          scale = fmaxl(scale, fabsl(u));
        }
        for (int p = 0; p < nphi; ++p) worst = fmax(worst, (double)(fabsl((ld)rho[(size_t)r * nphi + p] - want[(size_t)p]) / scale));
      }
      std::printf("plan-free model %d bytes '%s': worst %.3e of the row's max |rho|\n", cs.model, bytes, worst);
      CHECK(worst <= 1e-13);
    }
  }
  unsetenv("RTD_SURFACE_BYTES");
  // refusals
  const double ok[4] = {0.3, 0.1, 0.05, 0}, neg[4] = {0.3, -0.1, 0.05, 0}, half = 0.5, zero = 0.0, big = 1.5;
  double out[4];
  CHECK(rtd_surface_samples(0, RTD_SURFACE_ROSSLI, 1, neg, &half, &half, 4, out) == RTD_ERR_ARG && std::strstr(rtd_last_error(), "row 0"));
  CHECK(rtd_surface_samples(0, 4, 1, ok, &half, &half, 4, out) == RTD_ERR_ARG);
  CHECK(rtd_surface_samples(0, -1, 1, ok, &half, &half, 4, out) == RTD_ERR_ARG);
  CHECK(rtd_surface_samples(0, RTD_SURFACE_ROSSLI, 1, ok, &zero, &half, 4, out) == RTD_ERR_ARG);
  CHECK(rtd_surface_samples(0, RTD_SURFACE_ROSSLI, 1, ok, &half, &big, 4, out) == RTD_ERR_ARG);
  CHECK(rtd_surface_samples(0, RTD_SURFACE_ROSSLI, 1, ok, &half, &half, 0, out) == RTD_ERR_ARG);
  CHECK(rtd_surface_samples(0, RTD_SURFACE_ROSSLI, 1, ok, &half, &half, 16385, out) == RTD_ERR_ARG);
  CHECK(rtd_surface_samples(0, RTD_SURFACE_ROSSLI, 1, nullptr, &half, &half, 4, out) == RTD_ERR_ARG);
  CHECK(rtd_surface_samples(0, RTD_SURFACE_ROSSLI, -1, ok, &half, &half, 4, out) == RTD_ERR_ARG);
  CHECK(rtd_surface_samples(0, RTD_SURFACE_ROSSLI, 0, nullptr, nullptr, nullptr, 4, nullptr) == 0);
  return 0;
}

// One plan of P x G columns, `kind` 0 raw, 1 thermal with Kirchhoff emissivity, 2 band (thermal too when nsc = 2); beam or not;
// windows of 4 columns.  `bytes`: RTD_SURFACE_BYTES ("" = default).
static int scenario(int kind, int P, int G, bool beam, const char* bytes) {
  const int S = 2, L = 3, C = P * G, nquad = 8, N = 4, M = 3, NB = 2, nleg = 8, nall = 9, nphi = 16;
  const bool thermal = kind >= 1;
  if (*bytes) setenv("RTD_SURFACE_BYTES", bytes, 1);
  else unsetenv("RTD_SURFACE_BYTES");
  rtd_dims dims = {C, L, nquad, nleg, M, thermal ? 2 : 0, NB, beam ? 1 : 0};
  rtd_plan* p = nullptr;
  CHECK(rtd_plan_create_windowed(&dims, 0, 4, &p) == 0);
  vec mu(N), wq(N, 1.0 / N);
  for (int i = 0; i < N; ++i) mu[i] = (i + 0.5) / N;
  vec abs_(P * G * L, 0.2), dspec(P * L * S, 0.1), ospec(P * L * S, 0.7), lspec(S * nall, 0.5);
  for (int s = 0; s < S; ++s) lspec[s * nall] = 1.0;
  rtd_band bd = {P, G, S, nall, 1, abs_.data(), dspec.data(), ospec.data(), lspec.data()};
  vec tau(C * L), om(C * L, 0.6), f(C * L, 0.1), leg(C * L * nall, 0.5), mu0(C), I0(C, beam ? 1.0 : 0.0), phi0(C, 0.1);
  for (int c = 0; c < C; ++c) {
    mu0[c] = 0.3 + 0.05 * c;
    for (int l = 0; l < L; ++l) tau[c * L + l] = 0.3 * (l + 1) + 0.01 * c;
  }
  vec temper(C * (L + 1), 250.0), lo(C, 300.0), hi(C, 800.0), bt(C, 290.0);
  rtd_thermal th = {temper.data(), lo.data(), hi.data(), bt.data(), nullptr, nullptr, nullptr};  // emissivity NULL: Kirchhoff
  vec tq(C * NB * N * N, 0.125), tq0(C * NB * N, 0.25);
  auto upload = [&](const double* q, const double* q0) -> int {
    if (kind == 2) return rtd_plan_set_columns_band(p, &bd, mu0.data(), I0.data(), phi0.data(), nullptr, nullptr, q, q0, &th, nullptr);
    if (kind == 1)
      return rtd_plan_set_columns_thermal(p, tau.data(), om.data(), leg.data(), nall, f.data(), mu0.data(), I0.data(), phi0.data(), nullptr, nullptr, q, q0,
                                          &th);
    return rtd_plan_set_columns_raw(p, tau.data(), om.data(), leg.data(), nall, f.data(), mu0.data(), I0.data(), phi0.data(), nullptr, nullptr, nullptr, q, q0);
  };
  vec q(C * NB * N * N), q0(C * NB * N);
  auto tables_are = [&](double vq_mode0, double vq_rest, double vq0_mode0, double vq0_rest) {
    if (rtd_plan_get_bdrf(p, q.data(), q0.data()) != 0) return false;
    for (int c = 0; c < C; ++c)
      for (int m = 0; m < NB; ++m) {
        for (int k = 0; k < N * N; ++k)
          if (q[(c * NB + m) * N * N + k] != (m == 0 ? vq_mode0 : vq_rest)) return false;
        for (int k = 0; k < N; ++k)
          if (q0[(c * NB + m) * N + k] != (m == 0 ? vq0_mode0 : vq0_rest)) return false;
      }
    return true;
  };
  // a request before the quadrature: taken, but the columns are refused
  const double hap[4] = {1.0, 0.06, 0.6, 0.0};
  rtd_surface sf = {RTD_SURFACE_HAPKE, nphi, 1, hap};
  CHECK(rtd_plan_get_bdrf(p, q.data(), q0.data()) == RTD_ERR_STATE);
  CHECK(rtd_plan_request_surface(p, &sf) == 0);
  CHECK(upload(nullptr, nullptr) == RTD_ERR_STATE);
  CHECK(rtd_plan_set_quadrature(p, mu.data(), wq.data()) == 0);
  // the requests that are refused leave the standing one in place
  rtd_surface bad = sf;
  bad.nphi = 2 * (NB - 1);
  CHECK(rtd_plan_request_surface(p, &bad) == RTD_ERR_ARG);
  bad.nphi = 16385;
  CHECK(rtd_plan_request_surface(p, &bad) == RTD_ERR_ARG);
  bad = sf; bad.model = 4;
  CHECK(rtd_plan_request_surface(p, &bad) == RTD_ERR_ARG);
  bad = sf; bad.rows = 0;
  CHECK(rtd_plan_request_surface(p, &bad) == RTD_ERR_ARG);
  bad = sf; bad.params = nullptr;
  CHECK(rtd_plan_request_surface(p, &bad) == RTD_ERR_ARG);
  {
    vec rows(4 * 4, 0.0);
    for (int r = 0; r < 4; ++r) { rows[4 * r] = 1.0; rows[4 * r + 1] = 0.06; rows[4 * r + 2] = r == 2 ? 1.5 : 0.6; }  // W > 1 in row 2
    bad = sf; bad.rows = 4; bad.params = rows.data();
    CHECK(rtd_plan_request_surface(p, &bad) == RTD_ERR_ARG && std::strstr(rtd_last_error(), "row 2"));
    rows[4 * 2 + 2] = NAN;
    CHECK(rtd_plan_request_surface(p, &bad) == RTD_ERR_ARG && std::strstr(rtd_last_error(), "row 2"));
  }
  int64_t bytes0 = 0, bytes1 = 0;
  CHECK(rtd_plan_device_bytes(p, &bytes0) == 0);
  // rows = 1: every column's tables are reached by some chunk (the shadow reduction writes 0.5 into the tables of its view), whatever
  // the chunk size; a table next to the request is refused
  CHECK(upload(tq.data(), tq0.data()) == RTD_ERR_ARG);
  CHECK(upload(tq.data(), nullptr) == RTD_ERR_ARG);
  CHECK(upload(nullptr, nullptr) == 0);
  CHECK(tables_are(0.5, 0.5, 0.5, 0.5));
  CHECK(rtd_plan_get_bdrf(p, nullptr, q0.data()) == 0 && rtd_plan_get_bdrf(p, q.data(), nullptr) == 0 && rtd_plan_get_bdrf(p, nullptr, nullptr) == 0);
  CHECK(rtd_plan_device_bytes(p, &bytes1) == 0 && bytes1 == bytes0);  // nothing is held between uploads
  // the host-prepared uploads are refused while the request stands
  {
    vec so(C * L, 0.5), t0(C * (L + 1), 0.0), sc(C * L, 1.0), wl(C * L * nleg, 0.1), resc(C, 1.0), sp(C * L * 2, 0.0);
    for (int c = 0; c < C; ++c)
      for (int l = 0; l < L; ++l) t0[c * (L + 1) + l + 1] = tau[c * L + l];
    CHECK(rtd_plan_set_columns(p, so.data(), tau.data(), t0.data(), sc.data(), wl.data(), mu0.data(), I0.data(), phi0.data(), resc.data(), nullptr, nullptr,
                               thermal ? sp.data() : nullptr, tq.data(), tq0.data()) == RTD_ERR_STATE);
    CHECK(rtd_plan_set_columns_local(p, so.data(), tau.data(), t0.data(), sc.data(), wl.data(), mu0.data(), I0.data(), phi0.data(), resc.data(), nullptr,
                                     nullptr, thermal ? sp.data() : nullptr, nullptr, nullptr) == RTD_ERR_STATE);
  }
  // rows = C, per column; rows that fit nothing; a band's rows = P
  {
    vec rows(C * 4, 0.0);
    for (int c = 0; c < C; ++c) { rows[4 * c] = 0.1 + 0.01 * c; rows[4 * c + 1] = 0.8; rows[4 * c + 2] = -0.1; rows[4 * c + 3] = 0.1; }
    rtd_surface rpv = {RTD_SURFACE_RPV, nphi, C, rows.data()};
    CHECK(rtd_plan_request_surface(p, &rpv) == 0);
    rows.assign(rows.size(), NAN);  // (the parameters were copied)
    CHECK(upload(nullptr, nullptr) == 0 && tables_are(0.5, 0.5, 0.5, 0.5));
    vec three(3 * 4, 0.0);
    for (int r = 0; r < 3; ++r) { three[4 * r] = 0.3; three[4 * r + 1] = 0.1; three[4 * r + 2] = 0.05; }
    rtd_surface rl = {RTD_SURFACE_ROSSLI, nphi, 3, three.data()};
    CHECK(rtd_plan_request_surface(p, &rl) == 0);
    CHECK(upload(nullptr, nullptr) == ((kind == 2 && P == 3) || C == 3 ? 0 : RTD_ERR_ARG));
    rl.rows = P;
    vec perp(P * 4, 0.0);
    for (int r = 0; r < P; ++r) { perp[4 * r] = 0.3; perp[4 * r + 1] = 0.1; perp[4 * r + 2] = 0.05; }
    rl.params = perp.data();
    CHECK(rtd_plan_request_surface(p, &rl) == 0);
    CHECK(upload(nullptr, nullptr) == (kind == 2 || P == C || P == 1 ? 0 : RTD_ERR_ARG));
  }
  // Lambert: the tables are written directly and hold the row's albedo in mode 0 -- shared, per column, per profile of a band
  for (int rows : {1, C, P}) {
    if (rows == P && kind != 2 && P != C && P != 1) continue;
    vec alb(rows * 4, 0.0);
    for (int r = 0; r < rows; ++r) alb[4 * r] = 0.125 * (r % 7 + 1);
    rtd_surface lam = {RTD_SURFACE_LAMBERT, nphi, rows, alb.data()};
    CHECK(rtd_plan_request_surface(p, &lam) == 0);
    CHECK(upload(nullptr, nullptr) == 0);
    CHECK(rtd_plan_get_bdrf(p, q.data(), q0.data()) == 0);
    for (int c = 0; c < C; ++c) {
      const double a = alb[4 * (rows == 1 ? 0 : rows == C ? c : c / G)];
      for (int m = 0; m < NB; ++m) {
        for (int k = 0; k < N * N; ++k) CHECK(q[(c * NB + m) * N * N + k] == (m == 0 ? a : 0.0));
        for (int k = 0; k < N; ++k) CHECK(q0[(c * NB + m) * N + k] == (m == 0 && beam ? a : 0.0));  // no beam: the mu0 column is skipped
      }
    }
  }
  // a mu0 that no model takes, in a plan with a beam
  if (beam) {
    const double keep = mu0[C - 1];
    mu0[C - 1] = 0.0;
    CHECK(upload(nullptr, nullptr) == RTD_ERR_ARG);
    mu0[C - 1] = keep;
  }
  // solve and evaluate through every window with device-formed tables; rtd_plan_set_bdrf_samples still overwrites them
  CHECK(upload(nullptr, nullptr) == 0);
  {
    vec rqq((size_t)C * N * N * 8, 0.2), rq0((size_t)C * N * 8, 0.2);
    CHECK(rtd_plan_set_bdrf_samples(p, 8, rqq.data(), beam ? rq0.data() : nullptr) == 0);
    CHECK(tables_are(0.5, 0.5, 0.5, 0.5));
    const int nt = L + 1, np = 2;
    vec lev(C * nt, 0.0), phi = {0.0, 1.0}, u(C * nquad * nt * np);
    if (kind != 2) {
      for (int c = 0; c < C; ++c)
        for (int l = 0; l < L; ++l) lev[c * nt + 1 + l] = tau[c * L + l];
      CHECK(rtd_plan_set_eval_points(p, nt, lev.data(), np, phi.data()) == 0);
      CHECK(rtd_plan_run_fetch(p, u.data(), nullptr, nullptr, nullptr, nullptr) == 0);
    } else {
      CHECK(rtd_plan_solve(p) == 0 && rtd_plan_synchronize(p) == 0);
    }
  }
  // withdrawn (NULL, then model < 0): tables are required again, and the host-prepared upload is taken again
  CHECK(rtd_plan_request_surface(p, nullptr) == 0);
  CHECK(upload(nullptr, nullptr) == RTD_ERR_ARG);
  CHECK(upload(tq.data(), tq0.data()) == 0 && tables_are(0.125, 0.125, 0.25, 0.25));
  CHECK(rtd_plan_request_surface(p, &sf) == 0);
  rtd_surface off = {-1, 0, 0, nullptr};
  CHECK(rtd_plan_request_surface(p, &off) == 0);
  CHECK(upload(nullptr, nullptr) == RTD_ERR_ARG && upload(tq.data(), tq0.data()) == 0);
  CHECK(rtd_plan_destroy(p) == 0);
  return 0;
}

int main() {
  if (plan_free()) return 1;
  // per column: (16 + 4) x 16 samples = 2560 bytes with a beam, 16 x 16 x 8 = 2048 without
  for (int kind = 0; kind < 3; ++kind)
    for (int beam = 1; beam >= 0; --beam) {
      const char* one = beam ? "2560" : "2048";
      const char* three = beam ? "7680" : "6144";
      for (const char* bytes : {"", one, three, "8"})  // all columns in one chunk; chunks of 1; of 3 (3 + 3 + 1); less than one column: 1
        if (scenario(kind, 7, 1, beam != 0, bytes)) return 1;
    }
  for (const char* bytes : {"", "2560", "7680"}) {  // a band whose profiles share a parameter row: 2 x 3 and 3 x 2 columns
    if (scenario(2, 2, 3, true, bytes)) return 1;
    if (scenario(2, 3, 2, false, bytes)) return 1;
  }
  {  // a plan without BDRF modes takes no request
    rtd_dims dims = {2, 1, 4, 4, 1, 0, 0, 1};
    rtd_plan* p = nullptr;
    CHECK(rtd_plan_create(&dims, 0, &p) == 0);
    const double alb[4] = {0.3, 0, 0, 0};
    rtd_surface lam = {RTD_SURFACE_LAMBERT, 16, 1, alb};
    CHECK(rtd_plan_request_surface(p, &lam) == RTD_ERR_ARG);
    CHECK(rtd_plan_request_surface(p, nullptr) == 0);
    CHECK(rtd_plan_destroy(p) == 0);
  }
  CHECK(rtd_plan_request_surface(nullptr, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_get_bdrf(nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  std::printf("SURFACE HOST OK\n");
  return 0;
}
