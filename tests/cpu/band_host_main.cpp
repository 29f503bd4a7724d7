// TEST PROGRAM (tests/test_band_host_sanitized_cpu.py): the k-distribution band entry points -- rtd_band_mix,
// rtd_plan_set_columns_band, rtd_plan_set_band_weights, rtd_plan_fetch_band, rtd_plan_evaluate_band (csrc/rtd_api.hip) -- over the
// stand-in runtime of fake_hip/ and the shadow launchers of host_asan_shadow.cpp, as a stand-alone program under the address /
// undefined-behaviour sanitizers.  The mix and reduction kernels belong to rtd_api.hip itself, so they RUN here, thread by thread,
// on heap memory: every index they form is bounds-checked, and their values are held to the same formulas in long double.  All
// caller arrays are heap blocks of exactly the documented extent.
//
// What the shadow evaluation writes: u[c][i] = omega'[c][0] + 1e-3 i and the fluxes (2, 3, 4) omega'[c][0] + 1e-3 t, omega' the
// PREPARED albedo of the plan.  The shadow of the device preparation writes 0.5 for every column, so after a band upload the
// reduced values check the element stride and the weights; the column's identity comes from a second pass on the same plan whose
// columns are uploaded prepared (rtd_plan_set_columns), a different albedo per column: a wrong column stride fails there.
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

struct Band {
  int P, G, S, L, nleg_all;
  vec abs, dspec, ospec, lspec;
  rtd_band view(int delta_m) const { return {P, G, S, nleg_all, delta_m, abs.data(), dspec.data(), ospec.data(), lspec.data()}; }
};

static Band make_band(int P, int G, int S, int L, int nleg_all, bool dead_layer) {
  Band b{P, G, S, L, nleg_all, vec(P * G * L), vec(P * L * S), vec(P * L * S), vec(S * nleg_all)};
  for (int p = 0; p < P; ++p)
    for (int g = 0; g < G; ++g)
      for (int l = 0; l < L; ++l) b.abs[(p * G + g) * L + l] = 0.01 + 0.37 * std::fabs(std::sin(1.0 + p + 3.1 * g + 7.3 * l));
  for (int i = 0; i < P * L * S; ++i) {
    b.dspec[i] = 0.05 + 0.61 * std::fabs(std::cos(0.7 + 1.9 * i));
    b.ospec[i] = 0.02 + 0.95 * std::fabs(std::sin(2.3 + 0.77 * i));
  }
  if (dead_layer)  // profile 1, layer 1: no scatterer scatters (one species absent, the other purely absorbing)
    for (int s = 0; s < S; ++s) {
      b.ospec[(1 * L + 1) * S + s] = 0.0;
      if (s == 0) b.dspec[(1 * L + 1) * S + s] = 0.0;
    }
  for (int s = 0; s < S; ++s)
    for (int k = 0; k < nleg_all; ++k) b.lspec[s * nleg_all + k] = k == 0 ? 1.0 : std::pow(0.55 + 0.3 * s / (double)S, k);
  return b;
}

// the definitions of include/rtd.h in long double; every term is >= 0, so the expression is its own sum of absolute values
static int check_mix(const Band& b, int nleg, int delta_m, const vec& tau, const vec& om, const vec& f, const vec& leg) {
  const long double bound = (b.S + b.L + 4) * std::ldexp(1.0L, -53);
  for (int p = 0; p < b.P; ++p)
    for (int g = 0; g < b.G; ++g) {
      const int c = p * b.G + g;
      long double run = 0.0L;
      for (int l = 0; l < b.L; ++l) {
        long double sca = 0.0L, ext = 0.0L;
        for (int s = 0; s < b.S; ++s) {
          sca += (long double)b.ospec[(p * b.L + l) * b.S + s] * b.dspec[(p * b.L + l) * b.S + s];
          ext += b.dspec[(p * b.L + l) * b.S + s];
        }
        const long double dtau = ext + b.abs[(p * b.G + g) * b.L + l];
        run += dtau;
        CHECK(std::fabs((long double)tau[c * b.L + l] - run) <= bound * run);
        CHECK(std::fabs((long double)om[c * b.L + l] - sca / dtau) <= bound * (sca / dtau));
        for (int k = 0; k <= nleg; ++k) {  // k = nleg: the truncation fraction
          if (k == nleg && !delta_m) {
            CHECK(f[c * b.L + l] == 0.0);
            continue;
          }
          long double num = 0.0L;
          for (int s = 0; s < b.S; ++s)
            num += (long double)b.ospec[(p * b.L + l) * b.S + s] * b.dspec[(p * b.L + l) * b.S + s] * b.lspec[s * b.nleg_all + k];
          const long double want = k == 0 ? 1.0L : sca == 0.0L ? 0.0L : num / sca;
          const double got = k == nleg ? f[c * b.L + l] : leg[(c * b.L + l) * nleg + k];
          if (k == 0 || sca == 0.0L) CHECK((long double)got == (k == nleg ? 0.0L : want));
          else CHECK(std::fabs((long double)got - want) <= bound * want);
        }
      }
    }
  return 0;
}

static int mix_cases() {
  const int nleg = 8;
  for (int nleg_all : {9, 12})
    for (int delta_m : {0, 1})
      for (int S : {2, 1}) {
        const Band b = make_band(3, 5, S, 3, nleg_all, true);
        const int C = 15, L = 3;
        vec tau(C * L, -1.0), om(C * L, -1.0), f(C * L, -1.0), leg(C * L * nleg, -1.0);
        rtd_band v = b.view(delta_m);
        CHECK(rtd_band_mix(0, L, nleg, &v, tau.data(), om.data(), f.data(), leg.data()) == 0);
        if (check_mix(b, nleg, delta_m, tau, om, f, leg)) return 1;
      }
  // more than one block of every kernel
  {
    const Band b = make_band(40, 7, 3, 4, 6, false);
    const int C = 280, L = 4, nl = 5;
    vec tau(C * L), om(C * L), f(C * L), leg(C * L * nl);
    rtd_band v = b.view(1);
    CHECK(rtd_band_mix(0, L, nl, &v, tau.data(), om.data(), f.data(), leg.data()) == 0);
    if (check_mix(b, nl, 1, tau, om, f, leg)) return 1;
  }
  // refusals
  const Band b = make_band(3, 5, 2, 3, 9, false);
  vec o(15 * 3 * 9);
  rtd_band v = b.view(1);
  CHECK(rtd_band_mix(0, 3, 8, nullptr, o.data(), o.data(), o.data(), o.data()) == RTD_ERR_ARG);
  CHECK(rtd_band_mix(0, 3, 8, &v, nullptr, o.data(), o.data(), o.data()) == RTD_ERR_ARG);
  CHECK(rtd_band_mix(0, 3, 8, &v, o.data(), o.data(), o.data(), nullptr) == RTD_ERR_ARG);
  CHECK(rtd_band_mix(0, 0, 8, &v, o.data(), o.data(), o.data(), o.data()) == RTD_ERR_ARG);
  CHECK(rtd_band_mix(0, 3, 9, &v, o.data(), o.data(), o.data(), o.data()) == RTD_ERR_ARG);  // delta_m needs nleg_all > nleg
  v.delta_m = 0;
  CHECK(rtd_band_mix(0, 3, 9, &v, o.data(), o.data(), o.data(), o.data()) == 0);
  CHECK(rtd_band_mix(0, 3, 10, &v, o.data(), o.data(), o.data(), o.data()) == RTD_ERR_ARG);
  v.nspecies = 0;
  CHECK(rtd_band_mix(0, 3, 8, &v, o.data(), o.data(), o.data(), o.data()) == RTD_ERR_ARG);
  v = b.view(0);
  v.ngpoints = 0;
  CHECK(rtd_band_mix(0, 3, 8, &v, o.data(), o.data(), o.data(), o.data()) == RTD_ERR_ARG);
  v = b.view(0);
  v.omega_spec = nullptr;
  CHECK(rtd_band_mix(0, 3, 8, &v, o.data(), o.data(), o.data(), o.data()) == RTD_ERR_ARG);
  return 0;
}

// reduced arrays against the weighted sums of what the shadow evaluation wrote, per column albedo om0[c]
static int check_reduced(int P, int G, int K, int Q, int nt, int np, const vec& w, const vec& om0, const vec* u, const vec* u0,
                         const vec* fl[3]) {
  auto close = [](double got, long double want, long double size) {
    return std::fabs((long double)got - want) <= std::ldexp(1.0L, -52) * std::fabs(want) + std::ldexp(1.0L, -60) * size;
  };
  for (int p = 0; p < P; ++p)
    for (int k = 0; k < K; ++k) {
      const long E = (long)Q * nt * np;
      for (long e = 0; u && e < E; ++e) {
        long double want = 0.0L, size = 0.0L;
        for (int g = 0; g < G; ++g) {
          const long double t = (long double)w[k * G + g] * (om0[p * G + g] + 1e-3 * (double)e);
          want += t;
          size += std::fabs(t);
        }
        CHECK(close((*u)[((long)p * K + k) * E + e], want, size));
      }
      for (long e = 0; u0 && e < (long)Q * nt; ++e) {
        long double want = 0.0L, size = 0.0L;
        for (int g = 0; g < G; ++g) {
          want += (long double)w[k * G + g] * 0.5;
          size += std::fabs((long double)w[k * G + g] * 0.5);
        }
        CHECK(close((*u0)[((long)p * K + k) * Q * nt + e], want, size));
      }
      for (int f = 0; f < 3; ++f)
        for (int t = 0; fl[f] && t < nt; ++t) {
          long double want = 0.0L, size = 0.0L;
          for (int g = 0; g < G; ++g) {
            const long double x = (long double)w[k * G + g] * ((2.0 + f) * om0[p * G + g] + 1e-3 * (double)t);
            want += x;
            size += std::fabs(x);
          }
          CHECK(close((*fl[f])[((long)p * K + k) * nt + t], want, size));
        }
    }
  return 0;
}

// kind 0: plan of one window; 1: windows of 4 columns (C = 15: the last window is short and no window is a multiple of G);
// 2: the same, retained
static int plan_scenario(int kind, bool thermal) {
  const int P = 3, G = 5, S = 2, L = 3, C = P * G, nquad = 8, N = 4, M = 2, nleg = 8;
  rtd_dims dims = {C, L, nquad, nleg, M, thermal ? 2 : 0, 0, 1};
  rtd_plan* p = nullptr;
  if (kind == 0) CHECK(rtd_plan_create(&dims, 0, &p) == 0);
  else if (kind == 1) CHECK(rtd_plan_create_windowed(&dims, 0, 4, &p) == 0);
  else CHECK(rtd_plan_create_retained_form(&dims, 0, 4, (int64_t)1 << 30, 1, &p) == 0);
  int32_t wc = 0, nw = 0;
  CHECK(rtd_plan_windows(p, &wc, &nw) == 0 && (kind == 0 ? nw == 1 : (wc == 4 && nw == 4)));
  vec mu(N), wq(N, 1.0 / N);
  for (int i = 0; i < N; ++i) mu[i] = (i + 0.5) / N;
  CHECK(rtd_plan_set_quadrature(p, mu.data(), wq.data()) == 0);
  const Band b = make_band(P, G, S, L, 12, true);
  rtd_band v = b.view(1);
  vec mu0(C, 0.6), I0(C, 1.0), phi0(C, 0.1), bp(C * M * N, 0.25), bn(C * M * N, 0.125), tau_out(C * L, -1.0);
  vec temper(C * (L + 1)), lo(C, 300.0), hi(C, 800.0), bt(C, 290.0), tt(C, 80.0);
  for (int i = 0; i < C * (L + 1); ++i) temper[i] = 200.0 + i;
  rtd_thermal th = {temper.data(), lo.data(), hi.data(), bt.data(), tt.data(), nullptr, nullptr};
  const rtd_thermal* T = thermal ? &th : nullptr;
  // the mixed tau of the plan-free form: the plan's tau_out must carry the same bits
  vec tau(C * L), om(C * L), f(C * L), leg(C * L * nleg);
  CHECK(rtd_band_mix(0, L, nleg, &v, tau.data(), om.data(), f.data(), leg.data()) == 0);
  // every optional pointer NULL in turn
  for (int variant = 0; variant < 5; ++variant) {
    const double *b_pos = variant == 1 ? nullptr : bp.data(), *b_neg = variant == 2 ? nullptr : bn.data();
    double* out = variant == 3 ? nullptr : tau_out.data();
    rtd_thermal t2 = th;
    if (variant == 4) { t2.btemp = nullptr; b_pos = nullptr; b_neg = nullptr; }
    CHECK(rtd_plan_set_columns_band(p, &v, mu0.data(), I0.data(), phi0.data(), b_pos, b_neg, nullptr, nullptr, thermal ? &t2 : nullptr, out) == 0);
    CHECK(tau_out == tau);
    CHECK(rtd_plan_solve(p) == 0 && rtd_plan_synchronize(p) == 0);
  }
  // refusals of the upload
  CHECK(rtd_plan_set_columns_band(p, nullptr, mu0.data(), I0.data(), phi0.data(), nullptr, nullptr, nullptr, nullptr, T, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_set_columns_band(p, &v, nullptr, I0.data(), phi0.data(), nullptr, nullptr, nullptr, nullptr, T, nullptr) == RTD_ERR_ARG);
  if (thermal)
    CHECK(rtd_plan_set_columns_band(p, &v, mu0.data(), I0.data(), phi0.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  {
    rtd_band bad = v;
    bad.ngpoints = 4;  // P G != ncols
    CHECK(rtd_plan_set_columns_band(p, &bad, mu0.data(), I0.data(), phi0.data(), nullptr, nullptr, nullptr, nullptr, T, nullptr) == RTD_ERR_ARG);
    bad = v;
    bad.nleg_all = nleg;  // delta_m needs one moment more
    CHECK(rtd_plan_set_columns_band(p, &bad, mu0.data(), I0.data(), phi0.data(), nullptr, nullptr, nullptr, nullptr, T, nullptr) == RTD_ERR_ARG);
    bad = v;
    bad.nspecies = 0;
    CHECK(rtd_plan_set_columns_band(p, &bad, mu0.data(), I0.data(), phi0.data(), nullptr, nullptr, nullptr, nullptr, T, nullptr) == RTD_ERR_ARG);
    bad = v;
    bad.dtau_abs = nullptr;
    CHECK(rtd_plan_set_columns_band(p, &bad, mu0.data(), I0.data(), phi0.data(), nullptr, nullptr, nullptr, nullptr, T, nullptr) == RTD_ERR_ARG);
  }
  CHECK(rtd_plan_set_columns_band(p, &v, mu0.data(), I0.data(), phi0.data(), bp.data(), bn.data(), nullptr, nullptr, T, tau_out.data()) == 0);

  // ---- the reduction ----
  const int Q = nquad, ntL = L + 1, nphi = 3;
  vec lev(C * ntL, 0.0), phi = {0.0, 1.0, 2.0};
  for (int c = 0; c < C; ++c)
    for (int l = 0; l < L; ++l) lev[c * ntL + 1 + l] = tau_out[c * L + l];
  vec dummy(C * Q * ntL * nphi);
  CHECK(rtd_plan_fetch_band(p, dummy.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_STATE);  // no weights yet
  CHECK(rtd_plan_evaluate_band(p, ntL, lev.data(), nphi, phi.data(), 0, dummy.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_STATE);
  vec w5(5 * G);
  for (int i = 0; i < 5 * G; ++i) w5[i] = (i % 3 == 1 ? -1.0 : 1.0) * std::pow(10.0, -3.0 + 6.0 * std::fabs(std::sin(1.0 + i)));
  CHECK(rtd_plan_set_band_weights(p, 4, 1, w5.data()) == RTD_ERR_ARG);  // 15 % 4
  CHECK(rtd_plan_set_band_weights(p, G, 0, w5.data()) == RTD_ERR_ARG);
  CHECK(rtd_plan_set_band_weights(p, G, 1, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_set_band_weights(p, G, 1, w5.data()) == 0);
  CHECK(rtd_plan_fetch_band(p, dummy.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_STATE);  // nothing run yet
  CHECK(rtd_plan_set_mode_shard(p, 0, 2, 3) == RTD_ERR_STATE);
  char id[128] = {0};
  CHECK(rtd_comm_init(p, id, 0, 1) == RTD_ERR_STATE);
  for (int pass = 0; pass < 2; ++pass) {
    vec om0(C, 0.5);  // pass 0: band upload (the shadow preparation writes 0.5 for every column)
    if (pass == 1) {  // pass 1: prepared columns with an albedo per column
      vec so(C * L), t0(C * (L + 1), 0.0), sc(C * L, 1.0), wl(C * L * nleg, 0.1), resc(C, 1.0), sp(C * L * 2, 0.0);
      for (int c = 0; c < C; ++c) {
        om0[c] = 0.03 + 0.06 * c;
        for (int l = 0; l < L; ++l) {
          so[c * L + l] = om0[c];
          t0[c * (L + 1) + l + 1] = tau_out[c * L + l];
        }
      }
      CHECK(rtd_plan_set_columns(p, so.data(), tau_out.data(), t0.data(), sc.data(), wl.data(), mu0.data(), I0.data(), phi0.data(),
                                 resc.data(), nullptr, nullptr, thermal ? sp.data() : nullptr, nullptr, nullptr) == 0);
    }
    for (int K : {1, 5}) {
      CHECK(rtd_plan_set_band_weights(p, G, K, w5.data()) == 0);
      // run + fetch_band at the interfaces (the fused evaluation of one-window plans)
      CHECK(rtd_plan_set_eval_points(p, ntL, lev.data(), nphi, phi.data()) == 0);
      CHECK(rtd_plan_run(p) == 0);
      vec u(P * K * Q * ntL * nphi, -7.0), u0(P * K * Q * ntL, -7.0), fu(P * K * ntL, -7.0), fd(P * K * ntL, -7.0), fr(P * K * ntL, -7.0);
      CHECK(rtd_plan_fetch_band(p, u.data(), u0.data(), fu.data(), fd.data(), fr.data()) == 0);
      const vec* fl[3] = {&fu, &fd, &fr};
      if (check_reduced(P, G, K, Q, ntL, nphi, w5, om0, &u, &u0, fl)) return 1;
      // NULL outputs in turn; the unreduced fetch still works beside the reduced one
      vec fu2(P * K * ntL, -7.0), u2(P * K * Q * ntL * nphi, -7.0);
      CHECK(rtd_plan_fetch_band(p, nullptr, nullptr, fu2.data(), nullptr, nullptr) == 0 && fu2 == fu);
      CHECK(rtd_plan_fetch_band(p, u2.data(), nullptr, nullptr, nullptr, nullptr) == 0 && u2 == u);
      CHECK(rtd_plan_fetch_band(p, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
      vec full(C * Q * ntL * nphi);
      CHECK(rtd_plan_fetch(p, full.data(), nullptr, nullptr, nullptr, nullptr) == 0);
      // evaluate_band at a subset of levels, nphi 1 and 3
      for (int np : {1, 3}) {
        const int nt = 2;
        vec sub(C * nt);
        for (int c = 0; c < C; ++c) {
          sub[c * nt] = lev[c * ntL + 1];
          sub[c * nt + 1] = lev[c * ntL + 3];
        }
        vec eu(P * K * Q * nt * np, -7.0), eu0(P * K * Q * nt, -7.0), efu(P * K * nt, -7.0), efd(P * K * nt, -7.0), efr(P * K * nt, -7.0);
        CHECK(rtd_plan_evaluate_band(p, nt, sub.data(), np, phi.data(), 0, eu.data(), eu0.data(), efu.data(), efd.data(), efr.data()) == 0);
        const vec* efl[3] = {&efu, &efd, &efr};
        if (check_reduced(P, G, K, Q, nt, np, w5, om0, &eu, &eu0, efl)) return 1;
        vec efd2(P * K * nt, -7.0);
        CHECK(rtd_plan_evaluate_band(p, nt, sub.data(), np, phi.data(), 0, nullptr, nullptr, nullptr, efd2.data(), nullptr) == 0 && efd2 == efd);
        CHECK(rtd_plan_evaluate_band(p, nt, sub.data(), np, phi.data(), 4, eu.data(), nullptr, nullptr, nullptr, nullptr) == 0);  // derivative
        CHECK(rtd_plan_evaluate_band(p, nt, sub.data(), np, phi.data(), 5, eu.data(), nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
        CHECK(rtd_plan_evaluate_band(p, nt, sub.data(), 0, nullptr, 0, nullptr, eu0.data(), nullptr, nullptr, nullptr) == 0);  // no azimuths
      }
    }
  }
  CHECK(rtd_plan_set_band_weights(p, 0, 0, nullptr) == 0);  // off
  CHECK(rtd_plan_fetch_band(p, nullptr, nullptr, nullptr, nullptr, nullptr) == RTD_ERR_STATE);
  CHECK(rtd_plan_set_mode_shard(p, 0, 1, M) == 0);  // the default shard is no shard
  CHECK(rtd_plan_destroy(p) == 0);
  return 0;
}

int main() {
  if (mix_cases()) return 1;
  for (int kind = 0; kind < 3; ++kind)
    for (int thermal = 0; thermal < 2; ++thermal)
      if (plan_scenario(kind, thermal != 0)) return 1;
  {  // a mode-sharded plan takes neither stage; evaluate_band before any solve
    rtd_dims dims = {15, 3, 8, 8, 2, 0, 0, 1};
    rtd_plan* p = nullptr;
    CHECK(rtd_plan_create(&dims, 0, &p) == 0);
    const Band b = make_band(3, 5, 2, 3, 9, false);
    rtd_band v = b.view(1);
    vec one(15, 0.5), w(5, 0.2), out(15 * 8 * 3);
    CHECK(rtd_plan_set_band_weights(p, 5, 1, w.data()) == 0);
    CHECK(rtd_plan_evaluate_band(p, 1, one.data(), 0, nullptr, 0, nullptr, out.data(), nullptr, nullptr, nullptr) == RTD_ERR_STATE);
    CHECK(rtd_plan_set_band_weights(p, 0, 0, nullptr) == 0);
    CHECK(rtd_plan_set_mode_shard(p, 0, 2, 3) == 0);
    CHECK(rtd_plan_set_columns_band(p, &v, one.data(), one.data(), one.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RTD_ERR_STATE);
    CHECK(rtd_plan_set_band_weights(p, 5, 1, w.data()) == RTD_ERR_STATE);
    CHECK(rtd_plan_destroy(p) == 0);
  }
  CHECK(rtd_plan_set_band_weights(nullptr, 5, 1, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_fetch_band(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_evaluate_band(nullptr, 1, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  std::printf("BAND HOST OK\n");
  return 0;
}
