// TEST PROGRAM (tests/test_surface_ocean_cpu.py): RTD_SURFACE_OCEAN through rtd_plan_request_surface and the raw uploads of
// csrc/rtd_api.hip, over the stand-in runtime of fake_hip/ and the shadow launchers of host_asan_shadow.cpp, as a stand-alone program
// under the address / undefined-behaviour sanitizers.  A host compiler takes csrc/rtd_surface_ocean.hip into rtd_api.hip's unit, so
// rtd_surface_ocean_kernel RUNS here, thread by thread (one lane per pair of cosines), on heap memory: every index it forms and every
// table entry it writes is bounds-checked, and the tables are checked BY VALUE against the 50-digit modes of the same quadrature rule
// (tests/golden/surface_ocean/modes_n6.npz, handed over by the test as a text file of hex floats: argv[1]) within
//      tol_m = [16 np_dist_modes + (52 m + 104 + nphi / 2 + 8) 2^-53] (2 - delta_m0) q^0
// -- tools/surface_ocean_truth.py states the bound, csrc/rtd_surface_ocean.hip derives its second part.
// Also: every refusal of the request (U negative or not finite, n <= 1, rho_w < 0, nphi odd, nphi < 4 nbdrf), plans in windows of 4
// (6 columns: 4 + 2), shared against repeated parameters, a band's rows per profile, the thermal upload, a plan without a beam, and
// that the request holds no scratch block whatever RTD_SURFACE_BYTES says.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

static int N, NB, NPHI, C;
static vec MU, WQ, MU0, PAR, Q, Q0;
static double NP_DIST;

static bool read_vec(std::FILE* f, vec* v, size_t n) {
  v->resize(n);
  for (size_t i = 0; i < n; ++i)
    if (std::fscanf(f, "%la", &(*v)[i]) != 1) return false;
  return true;
}

static double tol(int m) { return 16.0 * NP_DIST + (52.0 * m + 104.0 + NPHI / 2 + 8.0) * std::ldexp(1.0, -53); }

// kind 0 raw, 1 thermal (Kirchhoff emissivity from the device-formed zeroth mode), 2 band of P x G columns with one row per profile
static int scenario(int kind, bool beam, int window, const char* bytes) {
  const int S = 2, L = 3, nquad = 2 * N, M = NB, nleg = nquad, nall = nquad + 1, G = 2, P = C / G;
  const bool thermal = kind >= 1;
  if (*bytes) setenv("RTD_SURFACE_BYTES", bytes, 1);
  else unsetenv("RTD_SURFACE_BYTES");
  rtd_dims dims = {C, L, nquad, nleg, M, thermal ? 2 : 0, NB, beam ? 1 : 0};
  rtd_plan* p = nullptr;
  CHECK(rtd_plan_create_windowed(&dims, 0, window, &p) == 0);
  CHECK(rtd_plan_set_quadrature(p, MU.data(), WQ.data()) == 0);
  vec abs_(P * G * L, 0.2), dspec(P * L * S, 0.1), ospec(P * L * S, 0.7), lspec(S * nall, 0.5);
  for (int s = 0; s < S; ++s) lspec[s * nall] = 1.0;
  rtd_band bd = {P, G, S, nall, 1, abs_.data(), dspec.data(), ospec.data(), lspec.data()};
  vec tau(C * L), om(C * L, 0.6), f(C * L, 0.1), leg(C * L * nall, 0.5), I0(C, beam ? 1.0 : 0.0), phi0(C, 0.1);
  for (int c = 0; c < C; ++c)
    for (int l = 0; l < L; ++l) tau[c * L + l] = 0.3 * (l + 1) + 0.01 * c;
  vec temper(C * (L + 1), 250.0), lo(C, 300.0), hi(C, 800.0), bt(C, 290.0);
  rtd_thermal th = {temper.data(), lo.data(), hi.data(), bt.data(), nullptr, nullptr, nullptr};  // emissivity NULL: Kirchhoff
  auto upload = [&]() -> int {
    if (kind == 2) return rtd_plan_set_columns_band(p, &bd, MU0.data(), I0.data(), phi0.data(), nullptr, nullptr, nullptr, nullptr, &th, nullptr);
    if (kind == 1)
      return rtd_plan_set_columns_thermal(p, tau.data(), om.data(), leg.data(), nall, f.data(), MU0.data(), I0.data(), phi0.data(), nullptr, nullptr, nullptr,
                                          nullptr, &th);
    return rtd_plan_set_columns_raw(p, tau.data(), om.data(), leg.data(), nall, f.data(), MU0.data(), I0.data(), phi0.data(), nullptr, nullptr, nullptr, nullptr,
                                    nullptr);
  };
  int64_t bytes0 = 0, bytes1 = 0;
  CHECK(rtd_plan_device_bytes(p, &bytes0) == 0);
  // rows = C: the tables by value
  rtd_surface sf = {RTD_SURFACE_OCEAN, NPHI, C, PAR.data()};
  CHECK(rtd_plan_request_surface(p, &sf) == 0);
  CHECK(upload() == 0);
  vec q((size_t)C * NB * N * N, -7.0), q0((size_t)C * NB * N, -7.0);
  CHECK(rtd_plan_get_bdrf(p, q.data(), q0.data()) == 0);
  CHECK(rtd_plan_device_bytes(p, &bytes1) == 0 && bytes1 == bytes0);  // nothing is held between uploads
  double worst = 0.0, worst0 = 0.0;
  for (int c = 0; c < C; ++c)
    for (int m = 0; m < NB; ++m) {
      const double sc = m == 0 ? 1.0 : 2.0;
      for (int k = 0; k < N * N; ++k) {
        const size_t at = ((size_t)c * NB + m) * N * N + k;
        CHECK(std::isfinite(q[at]));
        const double e = std::fabs(q[at] - Q[at]) / (sc * Q[(size_t)c * NB * N * N + k]);
        worst = std::fmax(worst, e / tol(m));
        CHECK(e <= tol(m));
      }
      for (int k = 0; k < N; ++k) {
        const size_t at = ((size_t)c * NB + m) * N + k;
        if (!beam) {
          CHECK(q0[at] == 0.0);  // the mu0 column is skipped
          continue;
        }
        CHECK(std::isfinite(q0[at]));
        const double e = std::fabs(q0[at] - Q0[at]) / (sc * Q0[(size_t)c * NB * N + k]);
        worst0 = std::fmax(worst0, e / tol(m));
        CHECK(e <= tol(m));
      }
    }
  std::printf("kind %d beam %d window %d bytes '%s': worst error / bound %.3f (q), %.3f (q0)\n", kind, (int)beam, window, bytes, worst, worst0);
  // shared against repeated parameters: the same bits; and they differ from the per-column tables
  {
    vec rep((size_t)C * 4);
    for (int c = 0; c < C; ++c) std::memcpy(&rep[4 * c], &PAR[4 * 2], 32);
    rtd_surface one = {RTD_SURFACE_OCEAN, NPHI, 1, &PAR[4 * 2]}, many = {RTD_SURFACE_OCEAN, NPHI, C, rep.data()};
    vec qa(q.size()), q0a(q0.size()), qb(q.size()), q0b(q0.size());
    CHECK(rtd_plan_request_surface(p, &one) == 0 && upload() == 0 && rtd_plan_get_bdrf(p, qa.data(), q0a.data()) == 0);
    CHECK(rtd_plan_request_surface(p, &many) == 0 && upload() == 0 && rtd_plan_get_bdrf(p, qb.data(), q0b.data()) == 0);
    CHECK(qa == qb && q0a == q0b && qa != q);
    if (kind == 2) {  // a band's rows per profile: column c takes row c / G
      vec rows((size_t)P * 4), percol((size_t)C * 4);
      for (int r = 0; r < P; ++r) std::memcpy(&rows[4 * r], &PAR[4 * (r + 1)], 32);
      for (int c = 0; c < C; ++c) std::memcpy(&percol[4 * c], &rows[4 * (c / G)], 32);
      rtd_surface prof = {RTD_SURFACE_OCEAN, NPHI, P, rows.data()}, col = {RTD_SURFACE_OCEAN, NPHI, C, percol.data()};
      CHECK(rtd_plan_request_surface(p, &prof) == 0 && upload() == 0 && rtd_plan_get_bdrf(p, qa.data(), q0a.data()) == 0);
      CHECK(rtd_plan_request_surface(p, &col) == 0 && upload() == 0 && rtd_plan_get_bdrf(p, qb.data(), q0b.data()) == 0);
      CHECK(qa == qb && q0a == q0b);
    }
  }
  // solve through every window with the device-formed tables
  CHECK(rtd_plan_request_surface(p, &sf) == 0 && upload() == 0);
  CHECK(rtd_plan_solve(p) == 0 && rtd_plan_synchronize(p) == 0);
  // a mu0 that no model takes
  if (beam) {
    const double keep = MU0[C - 1];
    MU0[C - 1] = 0.0;
    CHECK(upload() == RTD_ERR_ARG);
    MU0[C - 1] = keep;
  }
  CHECK(rtd_plan_destroy(p) == 0);
  unsetenv("RTD_SURFACE_BYTES");
  return 0;
}

static int refusals() {
  const int nquad = 2 * N;
  rtd_dims dims = {C, 3, nquad, nquad, NB, 0, NB, 1};
  rtd_plan* p = nullptr;
  CHECK(rtd_plan_create(&dims, 0, &p) == 0);
  const double good[4] = {5.0, 1.34, 0.02, 0.0};
  rtd_surface sf = {RTD_SURFACE_OCEAN, 4 * NB, 1, good};
  CHECK(rtd_plan_request_surface(p, &sf) == 0);  // nphi = 4 nbdrf is the smallest admitted
  const double bad[][4] = {{-1.0, 1.34, 0.0, 0.0}, {NAN, 1.34, 0.0, 0.0}, {INFINITY, 1.34, 0.0, 0.0}, {5.0, 1.0, 0.0, 0.0}, {5.0, 0.9, 0.0, 0.0},
                           {5.0, NAN, 0.0, 0.0}, {5.0, 1.34, -0.01, 0.0}, {5.0, 1.34, NAN, 0.0}, {5.0, 1.34, 0.0, INFINITY}};
  for (const auto& row : bad) {
    rtd_surface b = {RTD_SURFACE_OCEAN, 512, 1, row};
    CHECK(rtd_plan_request_surface(p, &b) == RTD_ERR_ARG && std::strstr(rtd_last_error(), "row 0"));
    double mu = 0.5, out[4];
    CHECK(rtd_surface_samples(0, RTD_SURFACE_OCEAN, 1, row, &mu, &mu, 4, out) == RTD_ERR_ARG);
  }
  {
    vec rows(3 * 4, 0.0);
    for (int r = 0; r < 3; ++r) { rows[4 * r] = 5.0; rows[4 * r + 1] = r == 1 ? 1.0 : 1.34; }  // n = 1 in row 1
    rtd_surface b = {RTD_SURFACE_OCEAN, 512, 3, rows.data()};
    CHECK(rtd_plan_request_surface(p, &b) == RTD_ERR_ARG && std::strstr(rtd_last_error(), "row 1"));
  }
  for (int nphi : {4 * NB - 2, 4 * NB + 1, 511, 2 * NB, 16386}) {
    rtd_surface b = {RTD_SURFACE_OCEAN, nphi, 1, good};
    CHECK(rtd_plan_request_surface(p, &b) == RTD_ERR_ARG);
  }
  rtd_surface top = {RTD_SURFACE_OCEAN, 16384, 1, good}, none = {5, 512, 1, good};
  CHECK(rtd_plan_request_surface(p, &top) == 0);
  CHECK(rtd_plan_request_surface(p, &none) == RTD_ERR_ARG);  // the next id is unknown
  // the other models keep their rule: an odd nphi below 4 nbdrf is theirs to take
  const double hap[4] = {1.0, 0.06, 0.6, 0.0};
  rtd_surface h = {RTD_SURFACE_HAPKE, 2 * NB - 1, 1, hap};
  CHECK(rtd_plan_request_surface(p, &h) == 0);
  CHECK(rtd_plan_destroy(p) == 0);
  // the plan-free samples: mu = 1 and mu' = 1 give numbers, not NaN
  const double mus[] = {1.0, 1.0, 0.3, 0.0199}, mups[] = {1.0, 0.4, 1.0, 0.0199};
  vec par;
  for (int r = 0; r < 4; ++r) par.insert(par.end(), good, good + 4);
  vec rho(4 * 8, -7.0);
  CHECK(rtd_surface_samples(0, RTD_SURFACE_OCEAN, 4, par.data(), mus, mups, 8, rho.data()) == 0);
  for (double v : rho) CHECK(std::isfinite(v) && v >= 0.02);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  if (std::fscanf(f, "%d %d %d %d %la", &N, &NB, &NPHI, &C, &NP_DIST) != 5) return 2;
  if (!(read_vec(f, &MU, N) && read_vec(f, &WQ, N) && read_vec(f, &MU0, C) && read_vec(f, &PAR, (size_t)C * 4) &&
        read_vec(f, &Q, (size_t)C * NB * N * N) && read_vec(f, &Q0, (size_t)C * NB * N)))
    return 2;
  std::fclose(f);
  if (refusals()) return 1;
  for (int kind = 0; kind < 3; ++kind)
    for (int window : {C, 4})
      if (scenario(kind, true, window, "")) return 1;
  if (scenario(0, false, 4, "")) return 1;
  if (scenario(0, true, 4, "8")) return 1;  // a scratch budget of one double: nothing of the ocean's asks for it
  std::printf("SURFACE OCEAN HOST OK\n");
  return 0;
}
