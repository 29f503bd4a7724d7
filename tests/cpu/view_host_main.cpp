// TEST PROGRAM (tests/test_view_host_sanitized_cpu.py): radiances at user polar angles -- rtd_plan_set_view_mu, rtd_plan_fetch_view,
// rtd_plan_fetch_band_view (csrc/rtd_api.hip) -- over the stand-in runtime of fake_hip/ and the shadow launchers of
// host_asan_shadow.cpp, as a stand-alone program under the address / undefined-behaviour sanitizers.  rtd_view_basis_kernel,
// rtd_view_apply_kernel and rtd_band_reduce_kernel belong to rtd_api.hip itself, so they RUN here, thread by thread, on heap memory:
// every index they form is bounds-checked, and every element they write is recomputed in long double from the u / u0 fetched from
// the same plan.  The shadow evaluation launcher fills u with omega[c][0] + 1e-3 k (k the position in the column's block), so a
// wrong row, stride or column in the kernel's reads of u is a wrong number; u0 is one constant, there only the bounds check sees
// it (the GPU test holds both to the exact interpolating polynomial of a real u and u0).  All caller arrays are heap blocks of
// exactly the documented extent.
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

static const int P = 3, G = 5, C = P * G, L = 3, NQ = 8, N = 4, M = 2, NLEG = 8, K = 2, NMU = 9;

struct Cols {
  vec mu, wq, om, tau, ts0, sc, wl, mu0, I0, phi0, resc;
};

static Cols make_cols() {
  Cols c{vec(N), vec(N), vec(C * L), vec(C * L), vec(C * (L + 1), 0.0), vec(C * L), vec(C * L * NLEG, 0.1), vec(C), vec(C), vec(C, 0.1), vec(C)};
  for (int i = 0; i < N; ++i) {
    c.mu[i] = (i + 0.5) / N;
    c.wq[i] = 0.1 * (i + 1);
  }
  for (int k = 0; k < C; ++k) {
    c.mu0[k] = 0.3 + 0.04 * k;
    c.resc[k] = 1.0;
    c.I0[k] = 1.0;
    double t = 0.0;
    for (int l = 0; l < L; ++l) {
      const double dt = 0.2 + 0.05 * ((k + 2 * l) % 5);
      t += dt;
      c.om[k * L + l] = 0.03 + 0.06 * k;
      c.tau[k * L + l] = t;
      c.sc[k * L + l] = 0.75 + 0.01 * (k + l);
      c.ts0[k * (L + 1) + l + 1] = c.ts0[k * (L + 1) + l] + dt * c.sc[k * L + l];
    }
  }
  return c;
}

// 1, a node, the float next above a node, an interior point, +0, -0, an interior point below, a negated node, -1
static vec shared_angles(const Cols& in) {
  return {1.0, in.mu[1], std::nextafter(in.mu[1], 2.0), 0.37, 0.0, -0.0, -0.62, -in.mu[2], -1.0};
}
// [C][NMU]: the columns of a profile alike, the profiles not: the hemispheres swapped for odd profiles, the interior points moved
static vec column_angles(const Cols& in) {
  const vec s = shared_angles(in);
  vec a(C * NMU);
  for (int c = 0; c < C; ++c)
    for (int m = 0; m < NMU; ++m) {
      const int p = c / G;
      double v = s[m];
      if (m == 3 || m == 6) v += 0.01 * p;
      if (p % 2) v = -v;
      a[c * NMU + m] = v;
    }
  return a;
}

// every element of out [C][NMU][E] against the interpolating polynomial in long double, from X [C][NQ][E] of the same plan.
// Roundings of the kernels (counted in tests/test_gpu_view.py): weight, subtraction and quotient in each numerator (3), the
// normalisation (1), the N products and N - 1 additions of the chain (N); the denominator's N such numerators and N - 1 additions
// are relative to the sum of MAGNITUDES, Lambda = sum_j |l_j| times the denominator, and a relative error of a divisor counts
// twice: held at (N + 4 + 2 (N + 2) Lambda) u sum_j |l_j X_j|, with a unit to spare for the second-order terms.
static int check_view(const Cols& in, const vec& mu, bool per_column, long E, const vec& X, const vec& out) {
  const long double u = std::ldexp(1.0L, -53);
  long double b[N];
  for (int j = 0; j < N; ++j) {
    long double prod = 1.0L;
    for (int k = 0; k < N; ++k)
      if (k != j) prod *= (long double)in.mu[j] - (long double)in.mu[k];
    b[j] = 1.0L / prod;
  }
  for (int c = 0; c < C; ++c)
    for (int m = 0; m < NMU; ++m) {
      const double v = mu[(per_column ? c * NMU : 0) + m], a = std::fabs(v);
      const int half = v > 0.0 ? 0 : N;
      int hit = -1;
      for (int j = 0; j < N; ++j)
        if (a == in.mu[j]) hit = j;
      long double l[N], s = 0.0L, lam = 0.0L;
      if (hit < 0) {
        for (int j = 0; j < N; ++j) s += (l[j] = b[j] / ((long double)a - (long double)in.mu[j]));
        for (int j = 0; j < N; ++j) lam += std::fabs(l[j] /= s);
      }
      for (long e = 0; e < E; ++e) {
        const double got = out[((long)c * NMU + m) * E + e];
        const double* x = &X[((long)c * NQ + half) * E + e];
        if (hit >= 0) {
          CHECK(got == x[hit * E]);  // the node's row, bit for bit
          continue;
        }
        long double want = 0.0L, size = 0.0L;
        for (int j = 0; j < N; ++j) {
          want += l[j] * x[j * E];
          size += std::fabs(l[j] * x[j * E]);
        }
        CHECK(std::fabs((long double)got - want) <= (N + 5 + 2 * (N + 2) * lam) * u * size);
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

// fetch both arrays, each pointer NULL in turn, and hold them to the u / u0 of the same plan; then the reduced ones.  has_u: the
// latest evaluation formed u; without it u_mu is refused and u0_mu alone is checked.
static int fetch_and_check(rtd_plan* p, const Cols& in, const vec& mu, bool per_column, int nt, int np, bool has_u, const vec& wb) {
  const long Eu = (long)nt * np, Eu0 = nt;
  vec u(has_u ? C * NQ * Eu : 0, -7.0), u0(C * NQ * Eu0, -7.0), vu(has_u ? C * NMU * Eu : 1, -7.0), vu0(C * NMU * Eu0, -7.0);
  CHECK(rtd_plan_fetch(p, has_u ? u.data() : nullptr, u0.data(), nullptr, nullptr, nullptr) == 0);
  if (!has_u) {
    CHECK(rtd_plan_fetch_view(p, vu.data(), vu0.data()) == RTD_ERR_STATE);
    CHECK(rtd_plan_fetch_band_view(p, vu.data(), nullptr) == RTD_ERR_STATE);
  }
  CHECK(rtd_plan_fetch_view(p, has_u ? vu.data() : nullptr, vu0.data()) == 0);
  if (has_u && check_view(in, mu, per_column, Eu, u, vu)) return 1;
  if (check_view(in, mu, per_column, Eu0, u0, vu0)) return 1;
  CHECK(rtd_plan_fetch_view(p, nullptr, nullptr) == 0);
  if (has_u) {
    vec a(C * NMU * Eu, -7.0), b(C * NMU * Eu0, -7.0);
    CHECK(rtd_plan_fetch_view(p, a.data(), nullptr) == 0 && a == vu);
    CHECK(rtd_plan_fetch_view(p, nullptr, b.data()) == 0 && b == vu0);
  }
  vec ru(has_u ? P * K * NMU * Eu : 1, -7.0), ru0(P * K * NMU * Eu0, -7.0);
  CHECK(rtd_plan_fetch_band_view(p, has_u ? ru.data() : nullptr, ru0.data()) == 0);
  if (has_u && check_reduced(wb, NMU * Eu, vu, ru)) return 1;
  if (check_reduced(wb, NMU * Eu0, vu0, ru0)) return 1;
  CHECK(rtd_plan_fetch_band_view(p, nullptr, nullptr) == 0);
  if (has_u) {
    vec a(P * K * NMU * Eu, -7.0), b(P * K * NMU * Eu0, -7.0);
    CHECK(rtd_plan_fetch_band_view(p, a.data(), nullptr) == 0 && a == ru);
    CHECK(rtd_plan_fetch_band_view(p, nullptr, b.data()) == 0 && b == ru0);
  }
  return 0;
}

// kind 0: plan of one window; 1: windows of 4 columns (C = 15, G = 5: 4 divides neither); 2: the same, retained
static int plan_scenario(int kind) {
  rtd_dims dims = {C, L, NQ, NLEG, M, 0, 0, 1};
  rtd_plan* p = nullptr;
  if (kind == 0) CHECK(rtd_plan_create(&dims, 0, &p) == 0);
  else if (kind == 1) CHECK(rtd_plan_create_windowed(&dims, 0, 4, &p) == 0);
  else CHECK(rtd_plan_create_retained_form(&dims, 0, 4, (int64_t)1 << 30, 1, &p) == 0);
  int32_t wc = 0, nw = 0;
  CHECK(rtd_plan_windows(p, &wc, &nw) == 0 && (kind == 0 ? nw == 1 : (wc == 4 && nw == 4)));
  const Cols in = make_cols();
  const vec shared = shared_angles(in), percol = column_angles(in);
  vec out(C * NMU * (L + 1) * 2);
  CHECK(rtd_plan_set_view_mu(p, NMU, shared.data(), 0) == RTD_ERR_STATE);  // no quadrature yet
  CHECK(rtd_plan_set_quadrature(p, in.mu.data(), in.wq.data()) == 0);
  CHECK(rtd_plan_set_view_mu(p, NMU, nullptr, 0) == RTD_ERR_ARG);
  {
    vec bad = shared;
    bad[3] = std::nextafter(1.0, 2.0);
    CHECK(rtd_plan_set_view_mu(p, NMU, bad.data(), 0) == RTD_ERR_ARG);
    bad[3] = -1.5;
    CHECK(rtd_plan_set_view_mu(p, NMU, bad.data(), 0) == RTD_ERR_ARG);
    bad[3] = std::numeric_limits<double>::quiet_NaN();
    CHECK(rtd_plan_set_view_mu(p, NMU, bad.data(), 0) == RTD_ERR_ARG);
    vec badc = percol;
    badc[(C - 1) * NMU + NMU - 1] = 1.25;  // the last element of the per-column extent
    CHECK(rtd_plan_set_view_mu(p, NMU, badc.data(), 1) == RTD_ERR_ARG);
  }
  CHECK(rtd_plan_set_columns(p, in.om.data(), in.tau.data(), in.ts0.data(), in.sc.data(), in.wl.data(), in.mu0.data(), in.I0.data(),
                             in.phi0.data(), in.resc.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  int64_t bytes0 = 0, bytes1 = 0;
  CHECK(rtd_plan_solve(p) == 0 && rtd_plan_synchronize(p) == 0);
  const int ntL = L + 1, nphi = 2;
  vec lev(C * ntL, 0.0), phi = {0.0, 1.0};
  for (int c = 0; c < C; ++c)
    for (int l = 0; l < L; ++l) lev[c * ntL + 1 + l] = in.tau[c * L + l];
  CHECK(rtd_plan_set_eval_points(p, ntL, lev.data(), nphi, phi.data()) == 0);
  CHECK(rtd_plan_run(p) == 0);
  CHECK(rtd_plan_fetch_view(p, out.data(), nullptr) == RTD_ERR_STATE);  // evaluated, but no angles
  CHECK(rtd_plan_device_bytes(p, &bytes0) == 0);
  CHECK(rtd_plan_set_view_mu(p, NMU, shared.data(), 0) == 0);
  CHECK(rtd_plan_device_bytes(p, &bytes1) == 0 && bytes1 == bytes0);  // (the request alone allocates nothing)
  CHECK(rtd_plan_fetch_band_view(p, out.data(), nullptr) == RTD_ERR_STATE);  // no weights
  CHECK(rtd_plan_device_bytes(p, &bytes1) == 0 && bytes1 == bytes0);
  CHECK(rtd_plan_solve(p) == 0);
  CHECK(rtd_plan_fetch_view(p, out.data(), nullptr) == RTD_ERR_STATE);  // solved, nothing evaluated
  CHECK(rtd_plan_set_eval_points(p, ntL, lev.data(), nphi, phi.data()) == 0);
  CHECK(rtd_plan_fetch_view(p, out.data(), nullptr) == RTD_ERR_STATE);  // points stored, nothing evaluated at them
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
  for (int per_column = 0; per_column < 2; ++per_column) {
    const vec& mu = per_column ? percol : shared;
    CHECK(rtd_plan_set_view_mu(p, NMU, mu.data(), per_column) == 0);
    for (int order : {0, -1, 1}) {
      // run + fetch at the interfaces
      CHECK(rtd_plan_set_eval_order(p, order) == 0);
      CHECK(rtd_plan_set_eval_points(p, ntL, lev.data(), nphi, phi.data()) == 0);
      CHECK(rtd_plan_run(p) == 0);
      if (fetch_and_check(p, in, mu, per_column, ntL, nphi, true, wb)) return 1;
      // run_fetch, nothing of u copied
      vec fu(C * ntL);
      CHECK(rtd_plan_run_fetch(p, nullptr, nullptr, fu.data(), nullptr, nullptr) == 0);
      if (fetch_and_check(p, in, mu, per_column, ntL, nphi, true, wb)) return 1;
      // evaluate and evaluate_band with the flag word, whatever the stored order
      const int flags = order < 0 ? 1 : order > 0 ? 4 : 0;
      CHECK(rtd_plan_set_eval_order(p, -order) == 0);
      vec eu(C * NQ * nt * nphi);
      CHECK(rtd_plan_evaluate(p, nt, sub.data(), nphi, phi.data(), flags, eu.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
      if (fetch_and_check(p, in, mu, per_column, nt, nphi, true, wb)) return 1;
      CHECK(rtd_plan_evaluate(p, nt, sub.data(), nphi, phi.data(), flags | 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);  // u stays on the device
      if (fetch_and_check(p, in, mu, per_column, nt, nphi, true, wb)) return 1;
      CHECK(rtd_plan_evaluate(p, nt, sub.data(), nphi, phi.data(), flags, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);  // u not wanted: none formed
      if (fetch_and_check(p, in, mu, per_column, nt, nphi, false, wb)) return 1;
      CHECK(rtd_plan_evaluate(p, nt, sub.data(), 0, nullptr, flags | 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);  // no azimuths
      if (fetch_and_check(p, in, mu, per_column, nt, 0, false, wb)) return 1;
      vec bfu(P * K * nt);
      CHECK(rtd_plan_evaluate_band(p, nt, sub.data(), nphi, phi.data(), flags | 8, nullptr, nullptr, bfu.data(), nullptr, nullptr) == 0);
      if (fetch_and_check(p, in, mu, per_column, nt, nphi, true, wb)) return 1;
      CHECK(rtd_plan_evaluate_band(p, nt, sub.data(), nphi, phi.data(), flags, nullptr, nullptr, bfu.data(), nullptr, nullptr) == 0);
      if (fetch_and_check(p, in, mu, per_column, nt, nphi, false, wb)) return 1;
    }
  }
  CHECK(rtd_plan_device_bytes(p, &bytes1) == 0 && bytes1 > bytes0);  // (the buffers came with the first fetch)
  // one angle after nine: smaller extents on the grown buffers
  {
    const double one = 0.5;
    vec a(C * nt), b(C * nt);
    CHECK(rtd_plan_set_view_mu(p, 1, &one, 0) == 0);
    CHECK(rtd_plan_fetch_view(p, nullptr, a.data()) == 0);
    CHECK(rtd_plan_set_view_mu(p, NMU, shared.data(), 0) == 0);
  }
  // withdrawal
  CHECK(rtd_plan_set_view_mu(p, 0, nullptr, 0) == 0);
  CHECK(rtd_plan_fetch_view(p, nullptr, out.data()) == RTD_ERR_STATE);
  CHECK(rtd_plan_fetch_band_view(p, nullptr, out.data()) == RTD_ERR_STATE);
  // unequal angles inside a band profile: refused at once while the weights are present (the earlier request stands) ...
  vec uneq = percol;
  uneq[(G + 2) * NMU + 3] += 0.05;
  CHECK(rtd_plan_set_view_mu(p, NMU, shared.data(), 0) == 0);
  CHECK(rtd_plan_set_view_mu(p, NMU, uneq.data(), 1) == RTD_ERR_ARG);
  CHECK(rtd_plan_fetch_band_view(p, nullptr, out.data()) == 0);
  // ... and at the band fetch when they arrived first; the unreduced fetch takes them
  CHECK(rtd_plan_set_band_weights(p, 0, 0, nullptr) == 0);
  CHECK(rtd_plan_set_view_mu(p, NMU, uneq.data(), 1) == 0);
  CHECK(rtd_plan_fetch_band_view(p, nullptr, out.data()) == RTD_ERR_STATE);  // no weights
  CHECK(rtd_plan_set_band_weights(p, G, K, wb.data()) == 0);
  CHECK(rtd_plan_fetch_band_view(p, nullptr, out.data()) == RTD_ERR_ARG);
  CHECK(rtd_plan_fetch_view(p, nullptr, out.data()) == 0);
  CHECK(rtd_plan_set_view_mu(p, NMU, percol.data(), 1) == 0);
  // sticky across a new solve; the buffers of the earlier one are refused
  CHECK(rtd_plan_solve(p) == 0);
  CHECK(rtd_plan_fetch_view(p, nullptr, out.data()) == RTD_ERR_STATE);
  CHECK(rtd_plan_evaluate(p, nt, sub.data(), nphi, phi.data(), 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  if (fetch_and_check(p, in, percol, true, nt, nphi, true, wb)) return 1;
  CHECK(rtd_plan_set_columns(p, in.om.data(), in.tau.data(), in.ts0.data(), in.sc.data(), in.wl.data(), in.mu0.data(), in.I0.data(),
                             in.phi0.data(), in.resc.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(rtd_plan_fetch_view(p, nullptr, out.data()) == RTD_ERR_STATE);  // new inputs
  if (kind == 0) {
    CHECK(rtd_plan_solve_layers(p, 0, L) == 0 && rtd_plan_solve_bc(p) == 0);
    CHECK(rtd_plan_fetch_view(p, nullptr, out.data()) == RTD_ERR_STATE);
    CHECK(rtd_plan_fetch_band_view(p, nullptr, out.data()) == RTD_ERR_STATE);
  }
  // a new quadrature: the weights and the basis follow it
  vec mu2 = in.mu;
  mu2[1] = 0.3;
  Cols in2 = in;
  in2.mu = mu2;
  CHECK(rtd_plan_set_quadrature(p, mu2.data(), in.wq.data()) == 0);
  CHECK(rtd_plan_set_view_mu(p, NMU, shared.data(), 0) == 0);
  CHECK(rtd_plan_solve(p) == 0);
  CHECK(rtd_plan_evaluate(p, nt, sub.data(), nphi, phi.data(), 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  if (fetch_and_check(p, in2, shared, false, nt, nphi, true, wb)) return 1;
  CHECK(rtd_plan_destroy(p) == 0);
  return 0;
}

int main() {
  for (int kind = 0; kind < 3; ++kind)
    if (plan_scenario(kind)) return 1;
  const double one = 0.5;
  CHECK(rtd_plan_set_view_mu(nullptr, 1, &one, 0) == RTD_ERR_ARG);
  CHECK(rtd_plan_fetch_view(nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_plan_fetch_band_view(nullptr, nullptr, nullptr) == RTD_ERR_ARG);
  CHECK(rtd_version() >= 216);
  std::printf("VIEW HOST OK\n");
  return 0;
}
