// TEST PROGRAM (tests/test_plan_trace_cpu.py): what the host side of librtd (csrc/rtd_api.hip) DOES, call by call, as a text trace
// of the stand-in runtime of fake_hip/ and the shadow launchers of host_asan_shadow.cpp (both built with -DFAKE_HIP_TRACE).  Scripted
// scenarios go through the public C entry points; after every call the return code (and the message of a failure) is printed, at the
// end of a scenario the trace: every stream, event, copy, fill, allocation and launch, with streams and events as ordinals and device
// pointers as "allocation + byte offset".  The output is compared line for line with tests/golden/host_trace/<scenario>.txt, which
// were recorded before the host file was folded: a flag that is no longer cleared, a table launch that moved to another stream, an
// offset that lost a factor shows as a changed line on the CPU.  Run as: plan_trace_host <scenario>  (a, b, b_serial, c, d, e, f).
// The communicator entry points are not here: the n-rank tests over the stand-in transport hold them (tests/test_host_asan.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtd.h"

extern "C" const char* fake_trace_take(void);
extern "C" void fake_trace_mark(const char* text);

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rtd_last_error()); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

// one call: its text goes into the trace as a label, its code (and the message of a failure) to the output
static int report(const char* text, int rc) {
  if (rc) std::printf("rc=%d %s -- %s\n", rc, text, rtd_last_error());
  else std::printf("rc=0 %s\n", text);
  return rc;
}
#define CALL(expr) (fake_trace_mark(#expr), report(#expr, (expr)))

static void section(const char* name) {
  std::printf("== %s\n", name);
  fake_trace_mark(name);
}
static void dump_trace() { std::printf("-- trace\n%s-- end\n", fake_trace_take()); }

typedef std::vector<double> vec;

// prepared and raw inputs of a batch, of the shapes the entry points take; values are plain (the shadow kernels compute nothing)
struct Batch {
  int C, L, nquad, N, nleg, M, Ns, NB, nall;
  rtd_dims dims;
  vec mu, wq, so, tau, t0, sc, wl, mu0, I0, phi0, resc, bp, bn, sp, bq, bq0, f, leg, iface, mid, phi;
  Batch(int C_, int L_, int nquad_, int nleg_, int M_, int Ns_, int NB_, int beam = 1)
      : C(C_), L(L_), nquad(nquad_), N(nquad_ / 2), nleg(nleg_), M(M_), Ns(Ns_), NB(NB_), nall(nleg_ + 4) {
    dims = {C, L, nquad, nleg, M, Ns, NB, beam};
    mu.resize(N); wq.assign(N, 1.0 / N);
    for (int i = 0; i < N; ++i) mu[i] = (i + 0.5) / N;
    so.assign(C * L, 0.5); sc.assign(C * L, 1.0); wl.assign(C * L * nleg, 0.1); f.assign(C * L, 0.1); leg.assign(C * L * nall, 0.5);
    tau.resize(C * L); t0.assign(C * (L + 1), 0.0);
    for (int c = 0; c < C; ++c)
      for (int l = 0; l < L; ++l) {
        tau[c * L + l] = 0.3 * (l + 1) + 0.01 * c;
        t0[c * (L + 1) + l + 1] = tau[c * L + l];
        so[c * L + l] = 0.5 + 0.01 * c + 0.02 * l;  // (the layer order of the eigen stage is sorted by this)
      }
    mu0.assign(C, 0.6); I0.assign(C, beam ? 1.0 : 0.0); phi0.assign(C, 0.1); resc.assign(C, 1.0);
    bp.assign(C * M * N, 0.25); bn.assign(C * M * N, 0.125); sp.assign(C * L * (Ns > 0 ? Ns : 1), 0.5);
    bq.assign(C * (NB > 0 ? NB : 1) * N * N, 0.05); bq0.assign(C * (NB > 0 ? NB : 1) * N, 0.05);
    iface.assign(C * (L + 1), 0.0);
    for (int c = 0; c < C; ++c)
      for (int l = 0; l < L; ++l) iface[c * (L + 1) + 1 + l] = tau[c * L + l];
    mid.resize(C * 2);
    for (int c = 0; c < C; ++c) { mid[2 * c] = 0.1; mid[2 * c + 1] = 0.45; }
    phi = {0.0, 1.0};
  }
  const double* spoly() const { return Ns > 0 ? sp.data() : nullptr; }
  const double* q() const { return NB > 0 ? bq.data() : nullptr; }
  const double* q0() const { return NB > 0 ? bq0.data() : nullptr; }
  int quadrature(rtd_plan* p) const { return rtd_plan_set_quadrature(p, mu.data(), wq.data()); }
  int columns(rtd_plan* p, bool local = false) const {
    return (local ? rtd_plan_set_columns_local : rtd_plan_set_columns)(p, so.data(), tau.data(), t0.data(), sc.data(), wl.data(), mu0.data(), I0.data(),
                                                                        phi0.data(), resc.data(), bp.data(), bn.data(), spoly(), q(), q0());
  }
  int raw(rtd_plan* p) const {
    return rtd_plan_set_columns_raw(p, tau.data(), so.data(), leg.data(), nall, f.data(), mu0.data(), I0.data(), phi0.data(), bp.data(), nullptr, spoly(),
                                    q(), q0());
  }
  int points_iface(rtd_plan* p) const { return rtd_plan_set_eval_points(p, L + 1, iface.data(), 2, phi.data()); }
  // result arrays large enough for every evaluation below
  vec u, u0, fu, fd, fdir, ul, a0, a1, a2;
  void results(int ntau_max) {
    u.assign(C * nquad * ntau_max * 2, 0.0); u0.assign(C * nquad * ntau_max, 0.0); ul = u0;
    fu.assign(C * ntau_max, 0.0); fd = fdir = a0 = a1 = a2 = fu;
  }
};

// a. one window
static int scenario_a() {
  section("a: one-window plan");
  Batch b(5, 3, 16, 4, 2, 2, 0);
  b.results(b.L + 1);
  rtd_plan* p = nullptr;
  CHECK(CALL(rtd_plan_create(&b.dims, 0, &p)) == 0);
  CALL(b.quadrature(p));
  CALL(b.columns(p));  // (the thermal polynomials are shifted on the host)
  CALL(b.points_iface(p));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_fetch(p, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  CALL(rtd_plan_evaluate(p, 2, b.mid.data(), 2, b.phi.data(), 0, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data(), nullptr));
  CALL(rtd_plan_evaluate(p, 2, b.mid.data(), 2, b.phi.data(), 0, b.u.data(), nullptr, nullptr, nullptr, nullptr, b.ul.data()));
  CALL(b.columns(p, true));
  CALL(b.points_iface(p));
  CALL(rtd_plan_run_fetch(p, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  {
    const int Q = b.nquad, n = b.M * b.L * Q;
    vec GC(n * Q), K(n), B(n), Gim(b.L * Q), G(n * Q);
    CALL(rtd_plan_get_tensors(p, 1, GC.data(), K.data(), B.data(), Gim.data(), G.data()));
  }
  CALL(rtd_plan_enable_timing(p, 1));
  CALL(rtd_plan_run(p));
  double ms[7];
  int64_t nl[7];
  CALL(rtd_plan_get_timing(p, ms, nl, 1));
  std::printf("nlaunch %ld %ld %ld %ld %ld %ld %ld\n", (long)nl[0], (long)nl[1], (long)nl[2], (long)nl[3], (long)nl[4], (long)nl[5], (long)nl[6]);
  CALL(rtd_plan_destroy(p));
  dump_trace();
  return 0;
}

// b. windows of 2 of 5 columns: three windows, the last partial; pipelined unless RTD_NO_PIPELINE
static int scenario_b(bool serial) {
  section(serial ? "b_serial: windowed plan under RTD_NO_PIPELINE" : "b: windowed pipelined plan");
  if (serial) setenv("RTD_NO_PIPELINE", "1", 1);
  Batch b(5, 3, 16, 4, 2, 0, 0);
  b.results(b.L + 1);
  rtd_plan* p = nullptr;
  CHECK(CALL(rtd_plan_create_windowed(&b.dims, 0, 2, &p)) == 0);
  int32_t cw = 0, nw = 0;
  CALL(rtd_plan_windows(p, &cw, &nw));
  std::printf("windows %d x %d\n", nw, cw);
  CALL(b.quadrature(p));
  CALL(b.columns(p));
  CALL(b.points_iface(p));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_fetch(p, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  CALL(rtd_plan_run_fetch(p, nullptr, nullptr, b.fu.data(), b.fd.data(), b.fdir.data()));
  {
    const int Q = b.nquad, n = b.M * b.L * Q;
    vec GC(n * Q), K(n), B(n), Gim(b.L * Q), G(n * Q);
    CALL(rtd_plan_get_tensors(p, 4, GC.data(), K.data(), B.data(), Gim.data(), G.data()));
  }
  CALL(rtd_plan_invalidate_tables(p));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_set_mode_shard(p, 1, 2, 4));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_synchronize(p));
  CALL(rtd_plan_destroy(p));
  dump_trace();
  return 0;
}

// c. retained (form 1) and lean (form 2, 17 layers: three wavefront chunks of 8, one evaluation point selects one of them)
static int scenario_c() {
  for (int form = 1; form <= 2; ++form) {
    section(form == 1 ? "c: retained plan" : "c: lean plan");
    Batch b(5, form == 1 ? 3 : 17, 16, 4, 2, 0, 0);
    b.results(b.L + 1);
    rtd_plan* p = nullptr;
    CHECK(CALL(rtd_plan_create_retained_form(&b.dims, 0, 2, (int64_t)1 << 30, form, &p)) == 0);
    int32_t kind = -1;
    CALL(rtd_plan_retained(p, &kind));
    std::printf("retained form %d\n", kind);
    CALL(b.quadrature(p));
    CALL(b.columns(p));
    CALL(rtd_plan_solve(p));
    vec one(b.C, 0.1);
    CALL(rtd_plan_evaluate(p, 1, one.data(), 2, b.phi.data(), 0, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data(), nullptr));
    CALL(rtd_plan_evaluate(p, b.L + 1, b.iface.data(), 2, b.phi.data(), 0, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data(), b.ul.data()));
    {
      const int Q = b.nquad, n = b.M * b.L * Q;
      vec GC(n * Q), K(n), B(n), Gim(b.L * Q), G(n * Q);
      CALL(rtd_plan_get_tensors(p, 3, GC.data(), K.data(), B.data(), Gim.data(), G.data()));
    }
    CALL(rtd_plan_set_eval_order(p, 1));
    CALL(rtd_plan_run(p));
    CALL(rtd_plan_fetch_actinic(p, b.a0.data(), b.a1.data(), b.a2.data()));
    CALL(rtd_plan_destroy(p));
    dump_trace();
  }
  return 0;
}

// d. raw, thermal and band inputs with the Nakajima-Tanaka request; 12 streams (N = 6 padded to 8), one BDRF mode, windows of 4 of 6
static int scenario_d() {
  section("d: raw, thermal and band inputs");
  const int P = 2, G = 3, S = 2;
  Batch b(P * G, 3, 12, 6, 2, 2, 1);
  b.results(b.L + 1);
  const int C = b.C, L = b.L, N = b.N, nall = b.nall;
  rtd_plan* p = nullptr;
  CHECK(CALL(rtd_plan_create_windowed(&b.dims, 0, 4, &p)) == 0);
  CALL(b.quadrature(p));
  CALL(rtd_plan_request_nt(p, nall));
  CALL(b.raw(p));
  CALL(b.points_iface(p));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_fetch(p, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  int32_t rows = -1;
  {
    vec w(C * L * nall), ff(C * L), ic(C * nall), ip(C * 2);
    CALL(rtd_plan_get_nt(p, w.data(), ff.data(), ic.data(), ip.data(), &rows));
    std::printf("nt rows %d\n", rows);
  }
  vec temper(C * (L + 1), 250.0), lo(C, 300.0), hi(C, 800.0), bt(C, 290.0), tt(C, 200.0);
  rtd_thermal th = {temper.data(), lo.data(), hi.data(), bt.data(), tt.data(), nullptr, nullptr};
  CALL(rtd_plan_set_columns_thermal(p, b.tau.data(), b.so.data(), b.leg.data(), nall, b.f.data(), b.mu0.data(), b.I0.data(), b.phi0.data(), nullptr, nullptr,
                                    b.q(), b.q0(), &th));
  CALL(rtd_plan_run(p));
  vec abs_(P * G * L, 0.2), dspec(P * L * S, 0.1), ospec(P * L * S, 0.7), lspec(S * nall, 0.5), tau_out(C * L, -1.0);
  for (int s = 0; s < S; ++s) lspec[s * nall] = 1.0;
  rtd_band bd = {P, G, S, nall, 1, abs_.data(), dspec.data(), ospec.data(), lspec.data()};
  CALL(rtd_plan_set_columns_band(p, &bd, b.mu0.data(), b.I0.data(), b.phi0.data(), b.bp.data(), nullptr, b.q(), b.q0(), &th, tau_out.data()));
  CALL(rtd_plan_get_nt(p, nullptr, nullptr, nullptr, nullptr, &rows));
  std::printf("nt rows %d\n", rows);
  vec wts = {0.2, 0.3, 0.5, 1.0, 1.0, 1.0};
  CALL(rtd_plan_set_band_weights(p, G, 2, wts.data()));
  vec lev(C * (L + 1), 0.0);
  for (int c = 0; c < C; ++c)
    for (int l = 0; l < L; ++l) lev[c * (L + 1) + 1 + l] = tau_out[c * L + l];
  CALL(rtd_plan_evaluate_band(p, L + 1, lev.data(), 2, b.phi.data(), 0, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  CALL(rtd_plan_solve(p));
  CALL(rtd_plan_evaluate_band(p, L + 1, lev.data(), 2, b.phi.data(), 0, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  CALL(rtd_plan_set_eval_points(p, L + 1, lev.data(), 2, b.phi.data()));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_fetch_band(p, b.u.data(), b.u0.data(), b.fu.data(), nullptr, b.fdir.data()));
  CALL(rtd_plan_fetch_band_actinic(p, b.a0.data(), nullptr, b.a2.data()));
  {
    vec t(C * L), o(C * L), ff(C * L), lg(C * L * b.nleg);
    CALL(rtd_band_mix(0, L, b.nleg, &bd, t.data(), o.data(), ff.data(), lg.data()));
    bd.nleg_all = b.nleg;  // (delta_m needs one moment more)
    CALL(rtd_band_mix(0, L, b.nleg, &bd, t.data(), o.data(), ff.data(), lg.data()));
    bd.nleg_all = nall;
  }
  // the host-prepared corrections on prepared columns, then a surface from samples
  CALL(rtd_plan_set_band_weights(p, 0, 0, nullptr));
  CALL(rtd_plan_request_nt(p, 0));
  CALL(b.columns(p));
  {
    vec w(C * L * nall, 0.5), ic(C * nall, 0.5), ip(C * 2, 0.5);
    CALL(rtd_plan_set_nt(p, nall, w.data(), b.f.data(), ic.data(), ip.data()));
  }
  CALL(b.points_iface(p));
  CALL(rtd_plan_run(p));
  {
    const int nphi = 4;
    vec rqq(C * N * N * nphi, 0.1), rq0(C * N * nphi, 0.1);
    CALL(rtd_plan_set_bdrf_samples(p, nphi, rqq.data(), rq0.data()));
  }
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_fetch(p, b.u.data(), nullptr, nullptr, nullptr, nullptr));
  CALL(rtd_plan_destroy(p));
  dump_trace();
  return 0;
}

// e. what each of the eight "inputs changed" entry points, successful and failed, leaves of the plan's state: the five consumers
// right after it (codes and messages), then one run whose trace tells what the flags caused -- tables launched again or not, the
// eigen stream forked behind the plan's stream or not
static void probe(rtd_plan* p, Batch& b) {
  CALL(rtd_plan_fetch(p, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  CALL(rtd_plan_fetch_actinic(p, b.a0.data(), b.a1.data(), b.a2.data()));
  CALL(rtd_plan_evaluate(p, 2, b.mid.data(), 2, b.phi.data(), 0, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data(), nullptr));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_fetch_band(p, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  CALL(rtd_plan_run(p));
}
static int scenario_e() {
  section("e: refusals and what the flags cause");
  Batch b(3, 3, 16, 4, 2, 0, 1);  // windows of 2 of 3 columns, pipelined; one BDRF mode
  b.results(b.L + 1);
  rtd_plan* p = nullptr;
  CHECK(CALL(rtd_plan_create_windowed(&b.dims, 0, 2, &p)) == 0);
  CALL(b.quadrature(p));
  CALL(b.columns(p));
  CALL(b.points_iface(p));
  vec wts(3, 1.0);
  CALL(rtd_plan_set_band_weights(p, 3, 1, wts.data()));
  probe(p, b);  // (before anything was solved)
  const int Q = b.nquad, n = b.M * b.L * Q, nphi = 4;
  vec GC(n * Q), K(n), B(n), Gim(b.L * Q), G(n * Q), rqq(b.C * b.N * b.N * nphi, 0.1), rq0(b.C * b.N * nphi, 0.1);
  section("e1: set_quadrature");
  CALL(b.quadrature(p));
  probe(p, b);
  CALL(rtd_plan_set_quadrature(p, nullptr, b.wq.data()));
  probe(p, b);
  section("e2: set_columns");
  CALL(b.columns(p));
  probe(p, b);
  CALL(rtd_plan_set_columns(p, nullptr, b.tau.data(), b.t0.data(), b.sc.data(), b.wl.data(), b.mu0.data(), b.I0.data(), b.phi0.data(), b.resc.data(), nullptr,
                            nullptr, nullptr, b.q(), b.q0()));
  probe(p, b);
  section("e3: set_columns_raw");
  CALL(b.raw(p));
  probe(p, b);
  CALL(rtd_plan_set_columns_raw(p, b.tau.data(), b.so.data(), b.leg.data(), b.nall, b.f.data(), nullptr, b.I0.data(), b.phi0.data(), nullptr, nullptr, nullptr,
                                b.q(), b.q0()));
  probe(p, b);
  section("e4: set_bdrf_samples");
  CALL(rtd_plan_set_bdrf_samples(p, nphi, rqq.data(), rq0.data()));
  probe(p, b);
  CALL(rtd_plan_set_bdrf_samples(p, 1, rqq.data(), rq0.data()));
  probe(p, b);
  section("e5: set_mode_shard");
  CALL(rtd_plan_set_mode_shard(p, 0, 1, b.M));
  probe(p, b);
  CALL(rtd_plan_set_mode_shard(p, 0, 0, b.M));
  probe(p, b);
  section("e6: invalidate_tables");
  CALL(rtd_plan_invalidate_tables(p));
  probe(p, b);
  CALL(rtd_plan_invalidate_tables(nullptr));
  section("e7: solve_layers (refused on a plan of several windows)");
  CALL(rtd_plan_solve_layers(p, 0, 2));
  probe(p, b);
  section("e8: get_tensors");
  CALL(rtd_plan_get_tensors(p, 0, GC.data(), K.data(), B.data(), Gim.data(), G.data()));
  probe(p, b);
  CALL(rtd_plan_get_tensors(p, b.C, GC.data(), K.data(), B.data(), Gim.data(), G.data()));
  probe(p, b);
  CALL(rtd_plan_destroy(p));
  dump_trace();

  section("e: a plan of one window without a surface table");
  Batch o(3, 3, 16, 4, 2, 0, 0);
  o.results(o.L + 1);
  CHECK(CALL(rtd_plan_create(&o.dims, 0, &p)) == 0);
  CALL(o.quadrature(p));
  CALL(o.columns(p));
  CALL(o.points_iface(p));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_set_bdrf_samples(p, nphi, rqq.data(), rq0.data()));
  probe(p, o);
  CALL(rtd_plan_solve_layers(p, 1, 2));
  probe(p, o);
  CALL(rtd_plan_solve_layers(p, 1, 2));
  CALL(rtd_plan_solve_bc(p));
  CALL(rtd_plan_evaluate(p, 2, o.mid.data(), 2, o.phi.data(), 0, o.u.data(), o.u0.data(), o.fu.data(), o.fd.data(), o.fdir.data(), nullptr));
  CALL(rtd_plan_solve_layers(p, 2, 2));
  probe(p, o);
  CALL(rtd_plan_destroy(p));
  dump_trace();
  return 0;
}

// f. the one-call forms, each with one failing argument set and one good one, then the pool
static int scenario_f() {
  section("f: one-call forms and the pool");
  Batch b(5, 3, 16, 4, 2, 0, 0);
  b.results(2);
  rtd_inputs in = {b.mu.data(), b.wq.data(), b.so.data(), b.tau.data(), b.t0.data(), b.sc.data(), b.wl.data(), b.mu0.data(),
                   b.I0.data(), b.phi0.data(), b.resc.data(), b.bp.data(), b.bn.data(), nullptr, nullptr, nullptr};
  rtd_inputs bad = in;
  bad.mu_pos = nullptr;
  CALL(rtd_solve_batch(&b.dims, 0, &bad, 2, b.mid.data(), 2, b.phi.data(), b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  CALL(rtd_solve_batch(&b.dims, 0, &in, 2, b.mid.data(), 2, b.phi.data(), b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  const int Q = b.nquad, n = b.M * b.L * Q;
  vec GC(n * Q), K(n), B(n), Gim(b.L * Q), G(n * Q);
  CALL(rtd_solve_tensors(&b.dims, 0, &in, b.C, GC.data(), K.data(), B.data(), Gim.data(), G.data()));
  CALL(rtd_solve_tensors(&b.dims, 0, &in, 2, GC.data(), K.data(), B.data(), Gim.data(), G.data()));
  int64_t held = -1, prev = -1, released = -1, fr = -1, total = -1;
  CALL(rtd_pool_bytes(&held));
  std::printf("pool holds %ld\n", (long)held);
  CALL(rtd_pool_set_limit((int64_t)1 << 20, 0, &prev));
  std::printf("previous limit %ld\n", (long)prev);
  CALL(rtd_device_memory(0, &fr, &total));
  std::printf("device memory %ld of %ld\n", (long)fr, (long)total);
  CALL(rtd_pool_trim(-1, &released));
  std::printf("released %ld\n", (long)released);
  CALL(rtd_pool_bytes(&held));
  std::printf("pool holds %ld\n", (long)held);
  dump_trace();
  return 0;
}

int main(int argc, char** argv) {
  const std::string which = argc > 1 ? argv[1] : "";
  int rc = 2;
  if (which == "a") rc = scenario_a();
  else if (which == "b") rc = scenario_b(false);
  else if (which == "b_serial") rc = scenario_b(true);
  else if (which == "c") rc = scenario_c();
  else if (which == "d") rc = scenario_d();
  else if (which == "e") rc = scenario_e();
  else if (which == "f") rc = scenario_f();
  else std::fprintf(stderr, "usage: plan_trace_host a|b|b_serial|c|d|e|f\n");
  if (rc == 0) std::printf("PLAN TRACE %s OK\n", which.c_str());
  return rc;
}
