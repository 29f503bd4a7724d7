// TEST PROGRAM (tests/test_lambert_host_sanitized_cpu.py): Lambertian albedo sweeps -- rtd_plan_couple_lambert,
// rtd_plan_couple_lambert_band, rtd_lambert_kappa (csrc/rtd_api.hip) -- over the stand-in runtime of fake_hip/ and the shadow
// launchers of host_asan_shadow.cpp, as a stand-alone program under the address / undefined-behaviour sanitizers.  A host compiler
// takes csrc/rtd_lambert.hip into rtd_api.hip's unit, so rtd_lambert_kappa_kernel and rtd_lambert_couple_kernel RUN here, thread by
// thread on heap memory, and so do rtd_band_reduce_kernel and the view kernels behind them: every index they form is bounds-checked,
// and every element they write is recomputed in long double from the arrays fetched from the same two plans.  The shadow evaluation
// launcher fills u and the fluxes with values that carry the column's identity and the position in its block, so a wrong column,
// stride or chunk offset is a wrong number; u0 is one constant, there only the bounds check sees it (the GPU test holds real fields).
// All caller arrays are heap blocks of exactly the documented extent.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
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

static const int P = 3, G = 5, C = P * G, L = 3, NQ = 8, N = 4, M = 2, NLEG = 8, K = 2, NMU = 3, NA = 4;
static const long double PI_L = 3.14159265358979323846264338327950288L;

struct Cols {
  vec mu, wq, om, tau, ts0, sc, wl, mu0, I0, phi0, resc, bpos;
};

// below: the companion's columns (no beam, b_pos = 1, another omega so that its shadow results differ from the primary's)
static Cols make_cols(bool below) {
  Cols c{vec(N), vec(N), vec(C * L), vec(C * L), vec(C * (L + 1), 0.0), vec(C * L), vec(C * L * NLEG, 0.1), vec(C), vec(C), vec(C, 0.1), vec(C),
         vec(C * N, 1.0)};
  for (int i = 0; i < N; ++i) {
    c.mu[i] = (i + 0.5) / N;
    c.wq[i] = 0.1 * (i + 1);
  }
  for (int k = 0; k < C; ++k) {
    c.mu0[k] = 0.3 + 0.04 * k;
    c.resc[k] = 1.0;
    c.I0[k] = below ? 0.0 : 1.0;
    double t = 0.0;
    for (int l = 0; l < L; ++l) {
      const double dt = 0.2 + 0.05 * ((k + 2 * l) % 5);
      t += dt;
      c.om[k * L + l] = (below ? 0.011 : 0.03) + 0.06 * k;
      c.tau[k * L + l] = t;
      c.sc[k * L + l] = 0.75 + 0.01 * (k + l);
      c.ts0[k * (L + 1) + l + 1] = c.ts0[k * (L + 1) + l] + dt * c.sc[k * L + l];
    }
  }
  return c;
}

struct Terms {
  vec shared, percol, perprof, F, s, E;
};
static Terms make_terms() {
  Terms t{{0.0, 0.3, 0.95, 1.0}, vec(C * NA), vec(P * NA), vec(C), vec(C), vec(C)};
  for (int c = 0; c < C; ++c) {
    t.F[c] = 1.0 + 0.1 * c;
    t.s[c] = 0.05 + 0.06 * c;  // up to 0.89: 1 / (1 - s) = 9
    t.E[c] = c % 3 == 0 ? 0.0 : 0.2 * c;
    for (int a = 0; a < NA; ++a) t.percol[c * NA + a] = a == 0 ? 0.0 : std::fmin(1.0, t.shared[a] * (0.5 + 0.05 * c));
  }
  for (int p = 0; p < P; ++p)
    for (int a = 0; a < NA; ++a) t.perprof[p * NA + a] = t.shared[a] * (1.0 - 0.2 * p);
  return t;
}

// the albedo of (column, index) for rows = 1, P or C
static double albedo_of(const vec& alb, int rows, int c, int a) { return alb[(rows == 1 ? 0 : rows == C ? c : c / G) * NA + a]; }

// out [C][NA][E] against X [C][E] + kappa Y [C][E / nrep] in long double, within the bound of csrc/rtd_lambert.h (8 u (|a| + |kappa b|))
static int check_coupled(const Terms& t, const vec& alb, int rows, bool emit, long E, int nrep, const vec& X, const vec& Y, const double* out) {
  const long double u = std::ldexp(1.0L, -53);
  for (int c = 0; c < C; ++c)
    for (int a = 0; a < NA; ++a) {
      const long double A = albedo_of(alb, rows, c, a), Ee = emit ? t.E[c] : 0.0;
      const long double kappa = (A * t.F[c] / PI_L + (1.0L - A) * Ee) / (1.0L - A * t.s[c]);
      for (long e = 0; e < E; ++e) {
        const long double x = X[c * E + e], y = Y[c * (E / nrep) + e / nrep], want = x + kappa * y;
        const double got = out[((long)c * NA + a) * E + e];
        CHECK(std::fabs((long double)got - want) <= 8.0L * u * (std::fabs(x) + std::fabs(kappa * y)));
        if (kappa == 0.0L) CHECK(got == X[c * E + e]);  // A = 0 without emission: the primary's element, bit for bit
      }
    }
  return 0;
}

static int check_reduced(const vec& w, long E, const vec& full, const vec& red) {
  for (int p = 0; p < P; ++p)
    for (int k = 0; k < K; ++k)
      for (long e = 0; e < E; ++e) {
        long double want = 0.0L, size = 0.0L;
        for (int g = 0; g < G; ++g) {
          const long double x = (long double)w[k * G + g] * full[(long)(p * G + g) * E + e];
          want += x;
          size += std::fabs(x);
        }
        CHECK(std::fabs((long double)red[(long)(p * K + k) * E + e] - want) <= std::ldexp(1.0L, -52) * std::fabs(want) + std::ldexp(1.0L, -60) * size);
      }
  return 0;
}

struct Coupled {
  vec u, u0, fup, fdn, vu, vu0;
};

// Couple the latest evaluations of (a, b) with `alb`, every output at once, and hold each element to the arrays fetched from the two
// plans; then each output alone, the others NULL (the same bits); then the band entry against weighted sums of the unreduced arrays.
// has_u: the primary's latest evaluation formed u; view: angles are set on both plans.
static int couple_and_check(rtd_plan* a, rtd_plan* b, const Terms& t, const vec& alb, int rows, bool emit, int nt, int np, bool has_u, bool view,
                            const vec& wb, Coupled* keep = nullptr) {
  const long Eu = (long)NQ * nt * np, Eu0 = (long)NQ * nt, Evu = (long)NMU * nt * np, Evu0 = (long)NMU * nt;
  vec xu(has_u ? C * Eu : 0), xu0(C * Eu0), xfup(C * nt), xfdn(C * nt), yu0(C * Eu0), yfup(C * nt), yfdn(C * nt);
  vec xvu(has_u && view ? C * Evu : 0), xvu0(view ? C * Evu0 : 0), yvu0(view ? C * Evu0 : 0);
  CHECK(rtd_plan_fetch(a, has_u ? xu.data() : nullptr, xu0.data(), xfup.data(), xfdn.data(), nullptr) == 0);
  CHECK(rtd_plan_fetch(b, nullptr, yu0.data(), yfup.data(), yfdn.data(), nullptr) == 0);
  if (view) {
    CHECK(rtd_plan_fetch_view(a, has_u ? xvu.data() : nullptr, xvu0.data()) == 0);
    CHECK(rtd_plan_fetch_view(b, nullptr, yvu0.data()) == 0);
  }
  const double* em = emit ? t.E.data() : nullptr;
  Coupled o{vec(has_u ? C * NA * Eu : 0, -7.0), vec(C * NA * Eu0, -7.0), vec(C * NA * nt, -7.0), vec(C * NA * nt, -7.0),
            vec(has_u && view ? C * NA * Evu : 0, -7.0), vec(view ? C * NA * Evu0 : 0, -7.0)};
  double *pu = has_u ? o.u.data() : nullptr, *pvu = has_u && view ? o.vu.data() : nullptr, *pvu0 = view ? o.vu0.data() : nullptr;
  if (!has_u) {
    vec dummy(C * NA * std::max<long>(Eu, 1) + 1);
    CHECK(rtd_plan_couple_lambert(a, b, NA, t.shared.data(), 1, t.F.data(), t.s.data(), em, dummy.data(), nullptr, nullptr, nullptr, nullptr, nullptr) ==
          RTD_ERR_STATE);
    CHECK(rtd_plan_couple_lambert_band(a, b, NA, alb.data(), rows, t.F.data(), t.s.data(), em, dummy.data(), nullptr, nullptr, nullptr, nullptr, nullptr) ==
          RTD_ERR_STATE);
  }
  if (rows != P) {
    CHECK(rtd_plan_couple_lambert(a, b, NA, alb.data(), rows, t.F.data(), t.s.data(), em, pu, o.u0.data(), o.fup.data(), o.fdn.data(), pvu, pvu0) == 0);
    if (has_u && check_coupled(t, alb, rows, emit, Eu, np, xu, yu0, o.u.data())) return 1;
    if (check_coupled(t, alb, rows, emit, Eu0, 1, xu0, yu0, o.u0.data())) return 1;
    if (check_coupled(t, alb, rows, emit, nt, 1, xfup, yfup, o.fup.data())) return 1;
    if (check_coupled(t, alb, rows, emit, nt, 1, xfdn, yfdn, o.fdn.data())) return 1;
    if (has_u && view && check_coupled(t, alb, rows, emit, Evu, np, xvu, yvu0, o.vu.data())) return 1;
    if (view && check_coupled(t, alb, rows, emit, Evu0, 1, xvu0, yvu0, o.vu0.data())) return 1;
    // each output alone
    double* all[6] = {pu, o.u0.data(), o.fup.data(), o.fdn.data(), pvu, pvu0};
    const vec* ref[6] = {&o.u, &o.u0, &o.fup, &o.fdn, &o.vu, &o.vu0};
    for (int i = 0; i < 6; ++i) {
      if (!all[i]) continue;
      vec one(ref[i]->size(), -7.0);
      double* q[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
      q[i] = one.data();
      CHECK(rtd_plan_couple_lambert(a, b, NA, alb.data(), rows, t.F.data(), t.s.data(), em, q[0], q[1], q[2], q[3], q[4], q[5]) == 0);
      CHECK(one == *ref[i]);
    }
    CHECK(rtd_plan_couple_lambert(a, b, NA, alb.data(), rows, t.F.data(), t.s.data(), em, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  } else {  // a list per profile is the band entry's alone: the unreduced arrays through the same list repeated per column
    vec rep(C * NA);
    for (int c = 0; c < C; ++c)
      for (int i = 0; i < NA; ++i) rep[c * NA + i] = alb[(c / G) * NA + i];
    CHECK(rtd_plan_couple_lambert(a, b, NA, alb.data(), rows, t.F.data(), t.s.data(), em, nullptr, o.u0.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
    CHECK(rtd_plan_couple_lambert(a, b, NA, rep.data(), C, t.F.data(), t.s.data(), em, pu, o.u0.data(), o.fup.data(), o.fdn.data(), pvu, pvu0) == 0);
  }
  // the band entry: reduced arrays against weighted sums of the unreduced coupled ones
  Coupled r{vec(has_u ? P * K * NA * Eu : 0, -7.0), vec(P * K * NA * Eu0, -7.0), vec(P * K * NA * nt, -7.0), vec(P * K * NA * nt, -7.0),
            vec(has_u && view ? P * K * NA * Evu : 0, -7.0), vec(view ? P * K * NA * Evu0 : 0, -7.0)};
  CHECK(rtd_plan_couple_lambert_band(a, b, NA, alb.data(), rows, t.F.data(), t.s.data(), em, has_u ? r.u.data() : nullptr, r.u0.data(), r.fup.data(),
                                     r.fdn.data(), has_u && view ? r.vu.data() : nullptr, view ? r.vu0.data() : nullptr) == 0);
  if (has_u && check_reduced(wb, NA * Eu, o.u, r.u)) return 1;
  if (check_reduced(wb, NA * Eu0, o.u0, r.u0)) return 1;
  if (check_reduced(wb, (long)NA * nt, o.fup, r.fup)) return 1;
  if (check_reduced(wb, (long)NA * nt, o.fdn, r.fdn)) return 1;
  if (has_u && view && check_reduced(wb, NA * Evu, o.vu, r.vu)) return 1;
  if (view && check_reduced(wb, NA * Evu0, o.vu0, r.vu0)) return 1;
  {
    vec one(r.fdn.size(), -7.0);
    CHECK(rtd_plan_couple_lambert_band(a, b, NA, alb.data(), rows, t.F.data(), t.s.data(), em, nullptr, nullptr, nullptr, one.data(), nullptr, nullptr) == 0);
    CHECK(one == r.fdn);
    CHECK(rtd_plan_couple_lambert_band(a, b, NA, alb.data(), rows, t.F.data(), t.s.data(), em, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  }
  if (keep) {
    *keep = o;
    keep->fup.insert(keep->fup.end(), r.u0.begin(), r.u0.end());  // (the reduced u0 rides along: the chunked run must reproduce it too)
  }
  return 0;
}

static int create(int kind, const rtd_dims& dims, rtd_plan** p) {
  if (kind == 0) CHECK(rtd_plan_create(&dims, 0, p) == 0);
  else if (kind == 1) CHECK(rtd_plan_create_windowed(&dims, 0, 4, p) == 0);
  else CHECK(rtd_plan_create_retained_form(&dims, 0, 4, (int64_t)1 << 30, 1, p) == 0);
  int32_t wc = 0, nw = 0;
  CHECK(rtd_plan_windows(*p, &wc, &nw) == 0 && (kind == 0 ? nw == 1 : (wc == 4 && nw == 4)));
  return 0;
}

static int set_cols(rtd_plan* p, const Cols& in, bool below) {
  CHECK(rtd_plan_set_quadrature(p, in.mu.data(), in.wq.data()) == 0);
  CHECK(rtd_plan_set_columns(p, in.om.data(), in.tau.data(), in.ts0.data(), in.sc.data(), in.wl.data(), in.mu0.data(), in.I0.data(), in.phi0.data(),
                             in.resc.data(), below ? in.bpos.data() : nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  return 0;
}

// kind 0: plans of one window; 1: windows of 4 columns (C = 15, G = 5: 4 divides neither); 2: the same, retained
static int plan_scenario(int kind) {
  const rtd_dims da = {C, L, NQ, NLEG, M, 0, 0, 1}, db = {C, L, NQ, NLEG, 1, 0, 0, 0};
  rtd_plan *a = nullptr, *b = nullptr;
  if (create(kind, da, &a) || create(kind, db, &b)) return 1;
  const Cols ina = make_cols(false), inb = make_cols(true);
  const Terms t = make_terms();
  if (set_cols(a, ina, false) || set_cols(b, inb, true)) return 1;
  vec sink(C * NA * NQ * (L + 1) * 2 + 8);
  auto couple_u0 = [&](rtd_plan* x, rtd_plan* y) {
    return rtd_plan_couple_lambert(x, y, NA, t.shared.data(), 1, t.F.data(), t.s.data(), nullptr, nullptr, sink.data(), nullptr, nullptr, nullptr, nullptr);
  };
  CHECK(couple_u0(a, b) == RTD_ERR_STATE);  // nothing solved
  CHECK(rtd_plan_solve(a) == 0 && rtd_plan_solve(b) == 0);
  CHECK(couple_u0(a, b) == RTD_ERR_STATE);  // solved, nothing evaluated
  const int ntL = L + 1, nphi = 2, nt = 4;
  vec lev(C * ntL, 0.0), phi = {0.0, 1.0}, sub(C * nt);
  for (int c = 0; c < C; ++c) {
    for (int l = 0; l < L; ++l) lev[c * ntL + 1 + l] = ina.tau[c * L + l];
    sub[c * nt] = 0.0;
    sub[c * nt + 1] = ina.tau[c * L + 1];
    sub[c * nt + 2] = ina.tau[c * L + 1] + 0.3 * (ina.tau[c * L + 2] - ina.tau[c * L + 1]);
    sub[c * nt + 3] = ina.tau[c * L + 2];
  }
  CHECK(rtd_plan_set_eval_points(a, ntL, lev.data(), nphi, phi.data()) == 0 && rtd_plan_set_eval_points(b, ntL, lev.data(), 0, nullptr) == 0);
  CHECK(rtd_plan_run(a) == 0);
  CHECK(couple_u0(a, b) == RTD_ERR_STATE);  // the companion holds no evaluation
  CHECK(rtd_plan_run(b) == 0);
  int64_t a0 = 0, b0 = 0, a1 = 0, b1 = 0;
  CHECK(rtd_plan_synchronize(a) == 0 && rtd_plan_synchronize(b) == 0);
  CHECK(rtd_plan_device_bytes(a, &a0) == 0 && rtd_plan_device_bytes(b, &b0) == 0);
  CHECK(couple_u0(a, b) == 0);
  CHECK(rtd_plan_device_bytes(a, &a1) == 0 && rtd_plan_device_bytes(b, &b1) == 0 && a1 == a0 && b1 == b0);  // nothing stays with either plan
  // ---- RTD_ERR_ARG
  CHECK(couple_u0(nullptr, b) == RTD_ERR_ARG && couple_u0(a, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_couple_lambert(a, b, 0, t.shared.data(), 1, t.F.data(), t.s.data(), nullptr, nullptr, sink.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_couple_lambert(a, b, NA, nullptr, 1, t.F.data(), t.s.data(), nullptr, nullptr, sink.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_couple_lambert(a, b, NA, t.shared.data(), 1, nullptr, t.s.data(), nullptr, nullptr, sink.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_couple_lambert(a, b, NA, t.shared.data(), 1, t.F.data(), nullptr, nullptr, nullptr, sink.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  for (int rows : {0, 2, P, C + 1, -1})
    CHECK(rtd_plan_couple_lambert(a, b, NA, t.percol.data(), rows, t.F.data(), t.s.data(), nullptr, nullptr, sink.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  for (double bad : {-1e-9, std::nextafter(1.0, 2.0), std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
    vec al = t.percol;
    al[(C - 1) * NA + NA - 1] = bad;  // the last element of the per-column extent
    CHECK(rtd_plan_couple_lambert(a, b, NA, al.data(), C, t.F.data(), t.s.data(), nullptr, nullptr, sink.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
    al = t.shared;
    al[1] = bad;
    CHECK(rtd_plan_couple_lambert(a, b, NA, al.data(), 1, t.F.data(), t.s.data(), nullptr, nullptr, sink.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  }
  for (double bad : {-1e-300, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
    vec em = t.E;
    em[C - 1] = bad;
    CHECK(rtd_plan_couple_lambert(a, b, NA, t.shared.data(), 1, t.F.data(), t.s.data(), em.data(), nullptr, sink.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  }
  // ---- RTD_ERR_STATE
  CHECK(couple_u0(a, a) == RTD_ERR_STATE);  // the companion's dims: two modes and a beam
  CHECK(couple_u0(b, b) == 0);              // (a black beamless plan of one mode may be both)
  CHECK(rtd_plan_couple_lambert(a, b, NA, t.shared.data(), 1, t.F.data(), t.s.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sink.data()) ==
        RTD_ERR_STATE);  // view wanted, no angles
  CHECK(rtd_plan_couple_lambert_band(a, b, NA, t.shared.data(), 1, t.F.data(), t.s.data(), nullptr, nullptr, sink.data(), nullptr, nullptr, nullptr, nullptr) ==
        RTD_ERR_STATE);  // no weights
  {
    const rtd_dims small = {C - 1, L, NQ, NLEG, 1, 0, 0, 0}, thin = {C, L - 1, NQ, NLEG, 1, 0, 0, 0}, few = {C, L, NQ - 2, NLEG - 2, 1, 0, 0, 0},
                   lamb = {C, L, NQ, NLEG, M, 0, 1, 1}, iso = {C, L, NQ, NLEG, 1, 2, 0, 0};
    for (const rtd_dims& d : {small, thin, few, iso}) {
      rtd_plan* o = nullptr;
      CHECK(rtd_plan_create(&d, 0, &o) == 0);
      CHECK(couple_u0(a, o) == RTD_ERR_STATE);
      CHECK(rtd_plan_destroy(o) == 0);
    }
    rtd_plan* o = nullptr;
    CHECK(rtd_plan_create(&lamb, 0, &o) == 0);
    CHECK(couple_u0(o, b) == RTD_ERR_STATE);  // the primary has a BDRF
    CHECK(rtd_plan_destroy(o) == 0);
  }
  // the resident ntau and tau-order of the two
  CHECK(rtd_plan_evaluate(a, nt, sub.data(), nphi, phi.data(), 1 | 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(rtd_plan_evaluate(b, nt, sub.data(), 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(couple_u0(a, b) == RTD_ERR_STATE);  // antiderivative against value
  CHECK(rtd_plan_evaluate(b, nt, sub.data(), 0, nullptr, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(couple_u0(a, b) == RTD_ERR_STATE);  // antiderivative against derivative
  CHECK(rtd_plan_evaluate(b, nt, sub.data(), 0, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(couple_u0(a, b) == 0);
  {
    vec five(C * 5, 0.0);
    CHECK(rtd_plan_evaluate(b, 5, five.data(), 0, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(couple_u0(a, b) == RTD_ERR_STATE);  // five points against four
  }
  vec wb(K * G);
  for (int i = 0; i < K * G; ++i) wb[i] = (i % 3 == 1 ? -1.0 : 1.0) * std::pow(10.0, -3.0 + 6.0 * std::fabs(std::sin(1.0 + i)));
  CHECK(rtd_plan_set_band_weights(a, G, K, wb.data()) == 0);

  // ---- every entry behind the coupling, in all three tau-orders; shared, per-column and per-profile albedos; with and without emission
  const vec vshared = {0.83, -0.41, -ina.mu[1]};
  vec vpercol(C * NMU);
  for (int c = 0; c < C; ++c)
    for (int m = 0; m < NMU; ++m) vpercol[c * NMU + m] = ((c / G) % 2 ? -1.0 : 1.0) * vshared[m] * (m == 2 ? 1.0 : 1.0 - 0.01 * (c / G));
  struct Alb { const vec* a; int rows; } albs[3] = {{&t.shared, 1}, {&t.percol, C}, {&t.perprof, P}};
  int turn = 0;
  for (int order : {0, -1, 1}) {
    const int flags = order < 0 ? 1 : order > 0 ? 4 : 0;
    const Alb& al = albs[turn % 3];
    const bool emit = turn % 2 == 0;
    ++turn;
    CHECK(rtd_plan_set_view_mu(a, 0, nullptr, 0) == 0 && rtd_plan_set_view_mu(b, 0, nullptr, 0) == 0);
    // run + run at the interfaces
    CHECK(rtd_plan_set_eval_order(a, order) == 0 && rtd_plan_set_eval_order(b, order) == 0);
    CHECK(rtd_plan_set_eval_points(a, ntL, lev.data(), nphi, phi.data()) == 0 && rtd_plan_set_eval_points(b, ntL, lev.data(), 0, nullptr) == 0);
    CHECK(rtd_plan_run(a) == 0 && rtd_plan_run(b) == 0);
    if (couple_and_check(a, b, t, *al.a, al.rows, emit, ntL, nphi, true, false, wb)) return 1;
    // run_fetch, nothing copied
    vec fu(C * ntL);
    CHECK(rtd_plan_run_fetch(a, nullptr, nullptr, fu.data(), nullptr, nullptr) == 0 && rtd_plan_run_fetch(b, nullptr, nullptr, fu.data(), nullptr, nullptr) == 0);
    if (couple_and_check(a, b, t, t.percol, C, !emit, ntL, nphi, true, false, wb)) return 1;
    // evaluate with the flag word, whatever the stored order; u kept on the device; then views with shared and per-column angles
    CHECK(rtd_plan_set_eval_order(a, -order) == 0 && rtd_plan_set_eval_order(b, -order) == 0);
    CHECK(rtd_plan_evaluate(a, nt, sub.data(), nphi, phi.data(), flags | 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(rtd_plan_evaluate(b, nt, sub.data(), 0, nullptr, flags, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    if (couple_and_check(a, b, t, *al.a, al.rows, emit, nt, nphi, true, false, wb)) return 1;
    CHECK(rtd_plan_set_view_mu(a, NMU, vshared.data(), 0) == 0);
    CHECK(rtd_plan_couple_lambert(a, b, NA, t.shared.data(), 1, t.F.data(), t.s.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sink.data()) ==
          RTD_ERR_STATE);  // angles on the primary alone
    CHECK(rtd_plan_set_view_mu(b, NMU - 1, vshared.data(), 0) == 0);
    CHECK(rtd_plan_couple_lambert(a, b, NA, t.shared.data(), 1, t.F.data(), t.s.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sink.data()) ==
          RTD_ERR_STATE);  // nmu differs
    CHECK(rtd_plan_set_view_mu(b, NMU, vshared.data(), 0) == 0);
    if (couple_and_check(a, b, t, *al.a, al.rows, emit, nt, nphi, true, true, wb)) return 1;
    CHECK(rtd_plan_set_view_mu(a, NMU, vpercol.data(), 1) == 0 && rtd_plan_set_view_mu(b, NMU, vpercol.data(), 1) == 0);
    if (couple_and_check(a, b, t, t.shared, 1, !emit, nt, nphi, true, true, wb)) return 1;
    // u not wanted: none formed; no azimuths
    CHECK(rtd_plan_evaluate(a, nt, sub.data(), nphi, phi.data(), flags, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    if (couple_and_check(a, b, t, *al.a, al.rows, emit, nt, nphi, false, true, wb)) return 1;
    CHECK(rtd_plan_evaluate(a, nt, sub.data(), 0, nullptr, flags | 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    if (couple_and_check(a, b, t, *al.a, al.rows, emit, nt, 0, false, true, wb)) return 1;
    // evaluate_band on the primary
    vec bfu(P * K * nt);
    CHECK(rtd_plan_evaluate_band(a, nt, sub.data(), nphi, phi.data(), flags | 8, nullptr, nullptr, bfu.data(), nullptr, nullptr) == 0);
    if (couple_and_check(a, b, t, t.perprof, P, emit, nt, nphi, true, true, wb)) return 1;
    // a scratch block small enough for several chunks (one column, one profile at a time): the same bits
    Coupled big, small;
    if (couple_and_check(a, b, t, t.percol, C, true, nt, nphi, true, true, wb, &big)) return 1;
    setenv("RTD_LAMBERT_BYTES", "2048", 1);
    if (couple_and_check(a, b, t, t.percol, C, true, nt, nphi, true, true, wb, &small)) return 1;
    setenv("RTD_LAMBERT_BYTES", "8192", 1);  // u: four columns per chunk, the last chunk of three; u0: eight and seven
    Coupled mid;
    if (couple_and_check(a, b, t, t.percol, C, true, nt, nphi, true, true, wb, &mid)) return 1;
    unsetenv("RTD_LAMBERT_BYTES");
    CHECK(big.u == small.u && big.u0 == small.u0 && big.fup == small.fup && big.fdn == small.fdn && big.vu == small.vu && big.vu0 == small.vu0);
    CHECK(big.u == mid.u && big.u0 == mid.u0 && big.fup == mid.fup && big.fdn == mid.fdn && big.vu == mid.vu && big.vu0 == mid.vu0);
  }
  // unequal angles inside a band profile: the band entry refuses them, the unreduced one takes them
  {
    vec uneq = vpercol;
    uneq[(G + 2) * NMU + 1] += 0.05;
    CHECK(rtd_plan_set_band_weights(a, 0, 0, nullptr) == 0);
    CHECK(rtd_plan_set_view_mu(a, NMU, uneq.data(), 1) == 0);
    CHECK(rtd_plan_set_band_weights(a, G, K, wb.data()) == 0);
    CHECK(rtd_plan_couple_lambert_band(a, b, NA, t.shared.data(), 1, t.F.data(), t.s.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sink.data()) ==
          RTD_ERR_ARG);
    CHECK(rtd_plan_couple_lambert(a, b, NA, t.shared.data(), 1, t.F.data(), t.s.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sink.data()) == 0);
    CHECK(rtd_plan_set_view_mu(a, NMU, vshared.data(), 0) == 0);
  }
  // a column whose 1 - A s is not positive: NaN in that column's outputs, the others kept, no error of its own
  {
    Terms tb = t;
    tb.s[7] = 1.25;
    vec out(C * NA * nt, -7.0), ok(C * NA * nt, -7.0);
    CHECK(rtd_plan_couple_lambert(a, b, NA, t.shared.data(), 1, t.F.data(), tb.s.data(), nullptr, nullptr, nullptr, out.data(), nullptr, nullptr, nullptr) == 0);
    CHECK(rtd_plan_couple_lambert(a, b, NA, t.shared.data(), 1, t.F.data(), t.s.data(), nullptr, nullptr, nullptr, ok.data(), nullptr, nullptr, nullptr) == 0);
    for (long i = 0; i < (long)out.size(); ++i) CHECK(i / (NA * nt) == 7 ? std::isnan(out[i]) : out[i] == ok[i]);
    vec kap(C * NA);
    std::vector<int32_t> flag(C, -1);
    CHECK(rtd_lambert_kappa(0, C, NA, t.shared.data(), 1, t.F.data(), tb.s.data(), nullptr, kap.data(), flag.data()) == 0);
    for (int c = 0; c < C; ++c) CHECK(flag[c] == (c == 7));
    CHECK(rtd_lambert_kappa(0, C, NA, t.percol.data(), C, t.F.data(), t.s.data(), t.E.data(), kap.data(), nullptr) == 0);
    const long double u = std::ldexp(1.0L, -53);
    for (int c = 0; c < C; ++c)
      for (int i = 0; i < NA; ++i) {
        const long double A = t.percol[c * NA + i], want = (A * t.F[c] / PI_L + (1.0L - A) * t.E[c]) / (1.0L - A * t.s[c]);
        CHECK(std::fabs((long double)kap[c * NA + i] - want) <= 6.0L * u * std::fabs(want));
      }
    CHECK(rtd_lambert_kappa(0, 0, NA, t.shared.data(), 1, t.F.data(), t.s.data(), nullptr, kap.data(), nullptr) == RTD_ERR_ARG);
    CHECK(rtd_lambert_kappa(0, C, NA, t.shared.data(), 2, t.F.data(), t.s.data(), nullptr, kap.data(), nullptr) == RTD_ERR_ARG);
    CHECK(rtd_lambert_kappa(0, C, NA, t.shared.data(), 1, t.F.data(), t.s.data(), nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  }
  // new inputs, a new solve: the buffers of the earlier ones are refused
  CHECK(rtd_plan_solve(b) == 0);
  CHECK(couple_u0(a, b) == RTD_ERR_STATE);
  CHECK(rtd_plan_evaluate(b, nt, sub.data(), 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(rtd_plan_evaluate(a, nt, sub.data(), 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(couple_u0(a, b) == 0);
  if (set_cols(a, ina, false)) return 1;
  CHECK(couple_u0(a, b) == RTD_ERR_STATE);
  // a mode shard on either plan
  CHECK(rtd_plan_set_band_weights(a, 0, 0, nullptr) == 0);
  CHECK(rtd_plan_set_mode_shard(a, 0, 2, 2 * M) == 0);
  CHECK(rtd_plan_solve(a) == 0);
  CHECK(rtd_plan_evaluate(a, nt, sub.data(), 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(couple_u0(a, b) == RTD_ERR_STATE);
  CHECK(rtd_plan_destroy(a) == 0 && rtd_plan_destroy(b) == 0);
  return 0;
}

int main() {
  for (int kind = 0; kind < 3; ++kind)
    if (plan_scenario(kind)) return 1;
  CHECK(rtd_version() >= 219);
  std::printf("LAMBERT HOST OK\n");
  return 0;
}
