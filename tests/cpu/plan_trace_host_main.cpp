// TEST PROGRAM (tests/test_plan_trace_cpu.py): what the host side of librtd (csrc/rtd_api.hip) DOES, call by call, as a text trace
// of the stand-in runtime of fake_hip/ and the shadow launchers of host_asan_shadow.cpp (both built with -DFAKE_HIP_TRACE).  Scripted
// scenarios go through the public C entry points; after every call the return code (and the message of a failure) is printed, at the
// end of a scenario the trace: every stream, event, copy, fill, allocation and launch, with streams and events as ordinals and device
// pointers as "allocation + byte offset".  The output is compared line for line with tests/golden/host_trace/<scenario>.txt, which
// were recorded before the host file was folded: a flag that is no longer cleared, a table launch that moved to another stream, an
// offset that lost a factor shows as a changed line on the CPU.  Run as: plan_trace_host <scenario>  (a, b, b_serial, c, d, e, f, g, h, i).
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

// The three scenarios below use 6 columns = 3 profiles x 2 spectral points (8 streams, 3 layers, 2 weight sets, 2 points, 2 azimuths,
// 2 angles): the smallest batch that windows or chunks of 2 columns split in three -- a first, a middle and a last one.
static const int VP = 3, VG = 2, VK = 2, VMU = 2;
static const double VW[VK * VG] = {0.25, 0.75, 1.0, 1.0};

// g. radiances at viewing angles: the basis formed once per request, the fetches plain and reduced, the refusals; then the
// corrections at the angles themselves (rtd_plan_set_view_nt), formed inside the windows of an evaluation
struct ViewArrays {
  vec shared, percol, uneq, zero, u, u0;
  explicit ViewArrays(int C) : shared{0.8, -0.3}, percol(C * VMU), zero{0.8, 0.0}, u(C * VMU * 2 * 2), u0(C * VMU * 2) {
    for (int c = 0; c < C; ++c)
      for (int m = 0; m < VMU; ++m) percol[c * VMU + m] = shared[m] * (1.0 - 0.1 * (c / VG));  // (alike within a profile)
    uneq = percol;
    uneq[1 * VMU + 1] += 0.05;  // column 1 against column 0 of the same profile
  }
};
static int view_nt_part(bool windowed) {
  section(windowed ? "g: corrections at the angles, three windows" : "g: corrections at the angles, one window");
  Batch b(VP * VG, 3, 8, 4, 2, 0, 0);
  b.results(2);
  ViewArrays v(b.C);
  rtd_plan* p = nullptr;
  if (windowed) CHECK(CALL(rtd_plan_create_windowed(&b.dims, 0, 2, &p)) == 0);
  else CHECK(CALL(rtd_plan_create(&b.dims, 0, &p)) == 0);
  int32_t cw = 0, nw = 0;
  CALL(rtd_plan_windows(p, &cw, &nw));
  std::printf("windows %d x %d\n", nw, cw);
  CALL(b.quadrature(p));
  CALL(rtd_plan_request_nt(p, b.nall));
  CALL(b.raw(p));
  CALL(rtd_plan_set_eval_points(p, 2, b.mid.data(), 2, b.phi.data()));
  CALL(rtd_plan_set_view_mu(p, VMU, v.zero.data(), 0));
  CALL(rtd_plan_set_view_nt(p, 1));  // (refused: mu = 0 among the angles)
  CALL(rtd_plan_set_view_mu(p, VMU, v.shared.data(), 0));
  CALL(rtd_plan_set_view_nt(p, 1));
  CALL(rtd_plan_set_view_mu(p, VMU, v.zero.data(), 0));  // (refused by this setter; the earlier request stands)
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));
  CALL(rtd_plan_set_view_nt(p, 0));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));  // (mode 0: the fetch interpolates the corrected u)
  CALL(rtd_plan_set_view_nt(p, 1));                       // mode 1 set after the evaluation
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));
  CALL(rtd_plan_fetch_view(p, nullptr, v.u0.data()));
  CALL(rtd_plan_run_fetch(p, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  CALL(rtd_plan_fetch_view(p, v.u.data(), nullptr));
  CALL(rtd_plan_set_view_mu(p, VMU, v.percol.data(), 1));
  CALL(rtd_plan_evaluate(p, 2, b.mid.data(), 2, b.phi.data(), 0, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data(), nullptr));
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));
  CALL(rtd_plan_set_band_weights(p, VG, VK, VW));
  CALL(rtd_plan_fetch_band_view(p, v.u.data(), v.u0.data()));
  CALL(rtd_plan_destroy(p));
  dump_trace();
  return 0;
}
static int scenario_g() {
  section("g: viewing angles on a one-window plan");
  Batch b(VP * VG, 3, 8, 4, 2, 0, 0);
  b.results(2);
  ViewArrays v(b.C);
  rtd_plan* p = nullptr;
  CHECK(CALL(rtd_plan_create(&b.dims, 0, &p)) == 0);
  CALL(b.quadrature(p));
  CALL(b.columns(p));
  CALL(rtd_plan_set_eval_points(p, 2, b.mid.data(), 2, b.phi.data()));
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));  // before set_view_mu
  CALL(rtd_plan_set_view_mu(p, VMU, v.shared.data(), 0));
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));  // nothing solved
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));
  CALL(rtd_plan_fetch_view(p, nullptr, v.u0.data()));
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));  // (no new request: the basis is not formed again)
  CALL(rtd_plan_set_view_mu(p, VMU, v.percol.data(), 1));
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));
  CALL(rtd_plan_evaluate(p, 2, b.mid.data(), 0, nullptr, 0, nullptr, b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data(), nullptr));
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));  // u_mu after an evaluation that formed no u
  CALL(rtd_plan_fetch_view(p, nullptr, v.u0.data()));
  CALL(rtd_plan_fetch_band_view(p, v.u.data(), v.u0.data()));  // before set_band_weights
  CALL(rtd_plan_set_band_weights(p, VG, VK, VW));
  CALL(rtd_plan_set_view_mu(p, VMU, v.uneq.data(), 1));  // (refused: the angles differ within a profile; the earlier request stands)
  CALL(rtd_plan_set_eval_points(p, 2, b.mid.data(), 2, b.phi.data()));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_fetch_band_view(p, v.u.data(), v.u0.data()));
  CALL(rtd_plan_fetch_band_view(p, nullptr, v.u0.data()));
  CALL(rtd_plan_set_band_weights(p, 0, 0, nullptr));
  CALL(rtd_plan_set_view_mu(p, VMU, v.uneq.data(), 1));
  CALL(rtd_plan_set_band_weights(p, VG, VK, VW));
  CALL(rtd_plan_fetch_band_view(p, v.u.data(), v.u0.data()));  // (refused here instead)
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));
  CALL(rtd_plan_set_view_mu(p, 0, nullptr, 0));  // withdrawn
  CALL(rtd_plan_fetch_view(p, v.u.data(), v.u0.data()));
  CALL(rtd_plan_destroy(p));
  dump_trace();
  return view_nt_part(false) || view_nt_part(true);
}

// h. surfaces requested from the raw uploads (Lambert, a parametric model in three chunks of columns, the ocean), the tables read
// back, and the plan-free helpers
static int scenario_h() {
  section("h: surfaces and the plan-free helpers");
  unsetenv("RTD_SURFACE_BYTES");
  const int nphi = 4;
  Batch b(VP * VG, 3, 8, 4, 2, 2, 2);
  b.results(2);
  const int C = b.C, L = b.L, N = b.N, NB = b.NB, nall = b.nall;
  vec lam = {0.3, 0, 0, 0}, hap(C * 4), ocean(VP * 4), q(C * NB * N * N), q0(C * NB * N);
  for (int c = 0; c < C; ++c) { hap[4 * c] = 1.0; hap[4 * c + 1] = 0.06; hap[4 * c + 2] = 0.6 - 0.05 * c; hap[4 * c + 3] = 0.0; }
  for (int r = 0; r < VP; ++r) { ocean[4 * r] = 5.0 + r; ocean[4 * r + 1] = 1.34; ocean[4 * r + 2] = 0.01; ocean[4 * r + 3] = 0.0; }
  auto raw = [&](rtd_plan* p, const double* bq, const double* bq0) {
    return rtd_plan_set_columns_raw(p, b.tau.data(), b.so.data(), b.leg.data(), nall, b.f.data(), b.mu0.data(), b.I0.data(), b.phi0.data(), b.bp.data(),
                                    nullptr, b.spoly(), bq, bq0);
  };
  rtd_plan *p = nullptr, *black = nullptr;
  CHECK(CALL(rtd_plan_create(&b.dims, 0, &p)) == 0);
  // what request_surface refuses
  rtd_surface sf = {RTD_SURFACE_HAPKE, nphi, C, hap.data()};
  CALL(rtd_plan_request_surface(nullptr, &sf));
  {
    Batch o(C, 3, 8, 4, 2, 0, 0);
    CHECK(CALL(rtd_plan_create(&o.dims, 0, &black)) == 0);
    CALL(rtd_plan_request_surface(black, &sf));  // nbdrf = 0
    CALL(rtd_plan_destroy(black));
  }
  rtd_surface bad = sf;
  bad.model = 5;
  CALL(rtd_plan_request_surface(p, &bad));
  bad = sf; bad.rows = 0;
  CALL(rtd_plan_request_surface(p, &bad));
  bad = sf; bad.params = nullptr;
  CALL(rtd_plan_request_surface(p, &bad));
  bad = sf; bad.nphi = 2;
  CALL(rtd_plan_request_surface(p, &bad));
  bad = sf; bad.nphi = 16385;
  CALL(rtd_plan_request_surface(p, &bad));
  bad = {RTD_SURFACE_OCEAN, 9, VP, ocean.data()};
  CALL(rtd_plan_request_surface(p, &bad));
  bad.nphi = 6;
  CALL(rtd_plan_request_surface(p, &bad));
  {
    vec row = hap;
    row[4 * 2 + 2] = 0.0;  // W = 0 in row 2
    bad = sf; bad.params = row.data();
    CALL(rtd_plan_request_surface(p, &bad));
  }
  // the Lambert model; columns before the quadrature, tables beside the request, prepared columns under the request
  rtd_surface lm = {RTD_SURFACE_LAMBERT, nphi, 1, lam.data()};
  CALL(rtd_plan_request_surface(p, &lm));
  CALL(raw(p, nullptr, nullptr));  // (refused: the quadrature is missing)
  CALL(b.quadrature(p));
  CALL(raw(p, b.q(), b.q0()));
  CALL(b.columns(p));
  CALL(rtd_plan_get_bdrf(p, q.data(), q0.data()));  // (no columns yet)
  CALL(raw(p, nullptr, nullptr));
  CALL(rtd_plan_get_bdrf(p, q.data(), nullptr));
  CALL(rtd_plan_get_bdrf(p, nullptr, q0.data()));
  CALL(rtd_plan_get_bdrf(p, q.data(), q0.data()));
  // a parametric model, a row per column, the samples of two columns at a time: three chunks
  setenv("RTD_SURFACE_BYTES", "1280", 1);  // 2 x (N N + N) nphi doubles
  CALL(rtd_plan_request_surface(p, &sf));
  CALL(raw(p, nullptr, nullptr));
  CALL(rtd_plan_set_eval_points(p, 2, b.mid.data(), 2, b.phi.data()));
  CALL(rtd_plan_run(p));
  CALL(rtd_plan_fetch(p, b.u.data(), b.u0.data(), b.fu.data(), b.fd.data(), b.fdir.data()));
  sf.rows = 4;
  CALL(rtd_plan_request_surface(p, &sf));
  CALL(raw(p, nullptr, nullptr));  // (refused: rows is neither 1 nor ncols)
  sf.rows = C;
  {
    vec far = b.mu0;
    far[C - 1] = 1.5;
    CALL(rtd_plan_request_surface(p, &sf));
    CALL(rtd_plan_set_columns_raw(p, b.tau.data(), b.so.data(), b.leg.data(), nall, b.f.data(), far.data(), b.I0.data(), b.phi0.data(), b.bp.data(), nullptr,
                                  b.spoly(), nullptr, nullptr));  // (refused: mu0 outside (0, 1])
  }
  // thermal sources over the same surface: the Kirchhoff emissivity reads the tables just formed and the quadrature
  vec temper(C * (L + 1), 250.0), lo(C, 300.0), hi(C, 800.0), bt(C, 290.0);
  rtd_thermal th = {temper.data(), lo.data(), hi.data(), bt.data(), nullptr, nullptr, nullptr};
  CALL(rtd_plan_set_columns_thermal(p, b.tau.data(), b.so.data(), b.leg.data(), nall, b.f.data(), b.mu0.data(), b.I0.data(), b.phi0.data(), nullptr, nullptr,
                                    nullptr, nullptr, &th));
  unsetenv("RTD_SURFACE_BYTES");
  // the ocean, a row per profile of a band
  const int S = 2;
  vec abs_(VP * VG * L, 0.2), dspec(VP * L * S, 0.1), ospec(VP * L * S, 0.7), lspec(S * nall, 0.5), tau_out(C * L, -1.0);
  for (int s = 0; s < S; ++s) lspec[s * nall] = 1.0;
  rtd_band bd = {VP, VG, S, nall, 1, abs_.data(), dspec.data(), ospec.data(), lspec.data()};
  rtd_surface oc = {RTD_SURFACE_OCEAN, 8, VP, ocean.data()};
  CALL(rtd_plan_request_surface(p, &oc));
  CALL(raw(p, nullptr, nullptr));  // (refused: three rows for six plain columns)
  CALL(rtd_plan_set_columns_band(p, &bd, b.mu0.data(), b.I0.data(), b.phi0.data(), b.bp.data(), nullptr, nullptr, nullptr, &th, tau_out.data()));
  CALL(rtd_plan_get_bdrf(p, q.data(), q0.data()));
  oc.rows = 1;
  CALL(rtd_plan_request_surface(p, &oc));
  CALL(raw(p, nullptr, nullptr));
  CALL(rtd_plan_request_surface(p, nullptr));  // withdrawn: tables again
  CALL(raw(p, nullptr, nullptr));
  CALL(raw(p, b.q(), b.q0()));
  CALL(rtd_plan_destroy(p));
  // the plan-free helpers
  {
    setenv("RTD_SURFACE_BYTES", "160", 1);  // 2 rows of nphi + 6 doubles: two chunks
    vec par(4 * 4), mu = {0.2, 0.4, 0.6, 0.8}, mup = {0.9, 0.7, 0.5, 0.3}, rho(4 * nphi);
    for (int r = 0; r < 4; ++r) { par[4 * r] = 1.0; par[4 * r + 1] = 0.06; par[4 * r + 2] = 0.6; par[4 * r + 3] = 0.0; }
    CALL(rtd_surface_samples(0, RTD_SURFACE_HAPKE, 4, par.data(), mu.data(), mup.data(), nphi, rho.data()));
    unsetenv("RTD_SURFACE_BYTES");
    CALL(rtd_surface_samples(0, RTD_SURFACE_HAPKE, 4, par.data(), mu.data(), mup.data(), 0, rho.data()));
    mup[3] = 0.0;
    CALL(rtd_surface_samples(0, RTD_SURFACE_HAPKE, 4, par.data(), mu.data(), mup.data(), nphi, rho.data()));
    vec T = {250.0, 280.0, 300.0}, wlo(3, 300.0), whi(3, 800.0), out(3);
    CALL(rtd_planck_band(0, 3, T.data(), wlo.data(), whi.data(), out.data()));
    CALL(rtd_planck_band(0, 3, nullptr, wlo.data(), whi.data(), out.data()));
    vec t(C * L), o(C * L), ff(C * L), lg(C * L * b.nleg);
    CALL(rtd_band_mix(0, L, b.nleg, &bd, t.data(), o.data(), ff.data(), lg.data()));
    CALL(rtd_band_mix(0, L, b.nleg, &bd, nullptr, o.data(), ff.data(), lg.data()));
  }
  dump_trace();
  return 0;
}

// i. Lambertian coupling of a primary and a companion plan: every output, plain and under band weights, in one chunk and in several,
// and one refusal from each test of the arguments and of the plans' state
static int scenario_i() {
  section("i: Lambertian coupling");
  unsetenv("RTD_LAMBERT_BYTES");
  const int NA = 2;
  Batch a(VP * VG, 3, 8, 4, 2, 0, 0), c(VP * VG, 3, 8, 4, 1, 0, 0, 0);
  a.results(2);
  const int C = a.C, Q = a.nquad;
  ViewArrays v(C);
  vec shared = {0.0, 0.5}, percol(C * NA), perprof(VP * NA), F(C), s(C), E(C);
  for (int k = 0; k < C; ++k) {
    F[k] = 1.0 + 0.1 * k; s[k] = 0.05 + 0.1 * k; E[k] = 0.2 * k;
    for (int i = 0; i < NA; ++i) percol[k * NA + i] = shared[i] * (1.0 - 0.1 * k);
  }
  for (int r = 0; r < VP; ++r)
    for (int i = 0; i < NA; ++i) perprof[r * NA + i] = shared[i] * (1.0 - 0.2 * r);
  vec u(C * NA * Q * 2 * 2), u0(C * NA * Q * 2), fup(C * NA * 2), fdn(C * NA * 2), vu(C * NA * VMU * 2 * 2), vu0(C * NA * VMU * 2);
  rtd_plan *pa = nullptr, *pb = nullptr, *other = nullptr;
  CHECK(CALL(rtd_plan_create(&a.dims, 0, &pa)) == 0);
  CHECK(CALL(rtd_plan_create(&c.dims, 0, &pb)) == 0);
  auto couple = [&](rtd_plan* x, rtd_plan* y, int nalb, const double* alb, int rows, const double* fd, const double* sp, const double* em, bool all) {
    return rtd_plan_couple_lambert(x, y, nalb, alb, rows, fd, sp, em, all ? u.data() : nullptr, u0.data(), all ? fup.data() : nullptr,
                                   all ? fdn.data() : nullptr, all ? vu.data() : nullptr, all ? vu0.data() : nullptr);
  };
  auto couple_u0 = [&](rtd_plan* x, rtd_plan* y) { return couple(x, y, NA, shared.data(), 1, F.data(), s.data(), nullptr, false); };
  CALL(a.quadrature(pa));
  CALL(a.columns(pa));
  CALL(c.quadrature(pb));
  CALL(c.columns(pb));
  CALL(rtd_plan_set_eval_points(pa, 2, a.mid.data(), 2, a.phi.data()));
  CALL(rtd_plan_set_eval_points(pb, 2, a.mid.data(), 0, nullptr));
  CALL(couple_u0(pa, pb));  // nothing to couple
  CALL(rtd_plan_run(pa));
  CALL(rtd_plan_run(pb));
  // the arguments
  CALL(couple(pa, pb, 0, shared.data(), 1, F.data(), s.data(), nullptr, false));
  CALL(couple(pa, pb, NA, shared.data(), 1, nullptr, s.data(), nullptr, false));
  CALL(couple(pa, pb, NA, percol.data(), VP, F.data(), s.data(), nullptr, false));  // (rows per profile: the band entry's alone)
  {
    vec al = percol, em = E;
    al[C * NA - 1] = 1.5;
    em[C - 1] = -1.0;
    CALL(couple(pa, pb, NA, al.data(), C, F.data(), s.data(), nullptr, false));
    CALL(couple(pa, pb, NA, shared.data(), 1, F.data(), s.data(), em.data(), false));
  }
  // the plans' state
  {
    Batch o(C - 1, 3, 8, 4, 1, 0, 0, 0), l(C, 3, 8, 4, 2, 0, 1);
    CHECK(CALL(rtd_plan_create(&o.dims, 0, &other)) == 0);
    CALL(couple_u0(pa, other));  // columns differ
    CALL(rtd_plan_destroy(other));
    CHECK(CALL(rtd_plan_create(&l.dims, 0, &other)) == 0);
    CALL(couple_u0(other, pb));  // the primary has a BDRF
    CALL(rtd_plan_destroy(other));
  }
  CALL(couple_u0(pa, pa));  // the companion's dims: two modes and a beam
  CALL(rtd_plan_set_mode_shard(pa, 0, 2, 4));
  CALL(couple_u0(pa, pb));  // a mode shard
  CALL(rtd_plan_set_mode_shard(pa, 0, 1, 2));
  CALL(couple_u0(pa, pb));  // nothing to couple: the shard undid the solution
  CALL(rtd_plan_run(pa));
  CALL(rtd_plan_evaluate(pb, 1, a.mu0.data(), 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  CALL(couple_u0(pa, pb));  // one point against two
  CALL(rtd_plan_set_eval_points(pb, 2, a.mid.data(), 0, nullptr));
  CALL(rtd_plan_run(pb));
  CALL(couple(pa, pb, NA, shared.data(), 1, F.data(), s.data(), nullptr, true));  // view outputs without angles
  CALL(rtd_plan_set_view_mu(pa, VMU, v.shared.data(), 0));
  CALL(rtd_plan_set_view_mu(pb, 1, v.shared.data(), 0));
  CALL(couple(pa, pb, NA, shared.data(), 1, F.data(), s.data(), nullptr, true));  // one angle against two
  CALL(rtd_plan_set_view_mu(pb, VMU, v.shared.data(), 0));
  CALL(rtd_plan_evaluate(pa, 2, a.mid.data(), 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  CALL(couple(pa, pb, NA, shared.data(), 1, F.data(), s.data(), nullptr, true));  // u wanted, none formed
  CALL(rtd_plan_couple_lambert(pa, pb, NA, shared.data(), 1, F.data(), s.data(), nullptr, nullptr, nullptr, nullptr, nullptr, vu.data(), nullptr));  // u_mu likewise
  CALL(rtd_plan_set_eval_points(pa, 2, a.mid.data(), 2, a.phi.data()));
  CALL(rtd_plan_run(pa));
  // every output: a shared list without emission, a list per column with it
  CALL(couple(pa, pb, NA, shared.data(), 1, F.data(), s.data(), nullptr, true));
  CALL(couple(pa, pb, NA, percol.data(), C, F.data(), s.data(), E.data(), true));
  CALL(couple_u0(pa, pb));
  setenv("RTD_LAMBERT_BYTES", "1024", 1);  // u: two columns per chunk, three chunks; u0: four and two, two chunks
  CALL(couple(pa, pb, NA, shared.data(), 1, F.data(), s.data(), nullptr, true));
  CALL(couple(pa, pb, NA, percol.data(), C, F.data(), s.data(), E.data(), true));
  unsetenv("RTD_LAMBERT_BYTES");
  // under band weights, a list per profile
  auto couple_band = [&](const double* alb, int rows, const double* em) {
    return rtd_plan_couple_lambert_band(pa, pb, NA, alb, rows, F.data(), s.data(), em, u.data(), u0.data(), fup.data(), fdn.data(), vu.data(), vu0.data());
  };
  CALL(couple_band(perprof.data(), VP, nullptr));  // before set_band_weights
  CALL(rtd_plan_set_band_weights(pa, VG, VK, VW));
  CALL(couple_band(perprof.data(), VP, nullptr));
  CALL(couple_band(shared.data(), 1, E.data()));
  setenv("RTD_LAMBERT_BYTES", "1024", 1);  // (a profile at a time)
  CALL(couple_band(perprof.data(), VP, E.data()));
  unsetenv("RTD_LAMBERT_BYTES");
  CALL(rtd_plan_destroy(pa));
  CALL(rtd_plan_destroy(pb));
  // the plan-free coupling term
  {
    vec kap(C * NA);
    std::vector<int32_t> flag(C, -1);
    vec big = s;
    big[2] = 1.25;  // 1 - A s not positive in column 2
    CALL(rtd_lambert_kappa(0, C, NA, shared.data(), 1, F.data(), big.data(), nullptr, kap.data(), flag.data()));
    std::printf("flags %d %d %d %d %d %d\n", flag[0], flag[1], flag[2], flag[3], flag[4], flag[5]);
    CALL(rtd_lambert_kappa(0, C, NA, percol.data(), C, F.data(), s.data(), E.data(), kap.data(), nullptr));
    CALL(rtd_lambert_kappa(0, C, NA, shared.data(), 2, F.data(), s.data(), nullptr, kap.data(), nullptr));
    CALL(rtd_lambert_kappa(0, 0, NA, shared.data(), 1, F.data(), s.data(), nullptr, kap.data(), nullptr));
  }
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
  else if (which == "g") rc = scenario_g();
  else if (which == "h") rc = scenario_h();
  else if (which == "i") rc = scenario_i();
  else std::fprintf(stderr, "usage: plan_trace_host a|b|b_serial|c|d|e|f|g|h|i\n");
  if (rc == 0) std::printf("PLAN TRACE %s OK\n", which.c_str());
  return rc;
}
