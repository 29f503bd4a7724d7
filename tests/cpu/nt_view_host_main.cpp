// TEST PROGRAM (tests/test_nt_view_cpu.py): csrc/rtd_nt_view.hip -- the two kernels of the Nakajima-Tanaka corrections at the viewing
// angles, with the routines of csrc/rtd_nt_view.h they run -- compiled over the stand-in runtime of tests/cpu/fake_hip into a stand-alone
// host program under the address / undefined-behaviour sanitizers.  The launchers run the kernels thread by thread on heap memory; no
// Python is loaded under a sanitizer, nothing is preloaded.
//
//   nt_view_host_main <input> : text, hexadecimal floats throughout (no decimal conversion anywhere)
//     "C L P nall nmu ntau nphi per_column window order group"   (order: -1 antiderivative, 0 value, +1 derivative; group: columns that
//       share a row of wfull, as the spectral points of a band profile do -- C % group == 0)
//     then the prepared inputs as the plan holds them:  omega[C][L] tau[C][L] taus0[C][L+1] scale[C][L] wleg[C][L][P] mu0[C] I0[C] phi0[C]
//       rescale[C] wfull[C / group][L][nall] f[C][L] ims_coef[C][nall] ims_par[C][2] mu[C or 1][nmu] evtau[C][ntau] phi[nphi]
//     -> per column one line: out[nmu][ntau][nphi], which started as zero (so it is rescale * (TMS + IMS))
//   The columns are processed in windows of `window` columns with the pointer offsets rtd_api.hip's window_dev / window_eval /
//   window_nt / window_nt_view apply, the table T sized for ONE window.
// Every array is a heap block of exactly its documented extent: an index out of range is a sanitizer report.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../pythonic-disort_amd/csrc/rtd_nt_view.hip"

thread_local fake_idx blockIdx, threadIdx, blockDim, gridDim;

typedef std::vector<double> vec;

static bool read(FILE* f, vec& v) {
  for (double& x : v)
    if (std::fscanf(f, "%la", &x) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* in = std::fopen(argv[1], "r");
  if (!in) return 2;
  int C, L, P, nall, nmu, ntau, nphi, per_column, window, order, group;
  if (std::fscanf(in, "%d %d %d %d %d %d %d %d %d %d %d", &C, &L, &P, &nall, &nmu, &ntau, &nphi, &per_column, &window, &order, &group) != 11) return 3;
  if (group < 1 || C % group != 0) return 3;
  const size_t c = C, l = L;
  vec omega(c * l), tau(c * l), taus0(c * (l + 1)), scale(c * l), wleg(c * l * P), mu0(c), I0(c), phi0(c), rescale(c), wfull(c / group * l * nall),
      f(c * l), coef(c * nall), par(c * 2), mu((per_column ? c : 1) * nmu), evtau(c * ntau), phi(nphi);
  for (vec* v : {&omega, &tau, &taus0, &scale, &wleg, &mu0, &I0, &phi0, &rescale, &wfull, &f, &coef, &par, &mu, &evtau, &phi})
    if (!read(in, *v)) return 3;
  std::fclose(in);
  vec T((size_t)std::min(window, C) * l * nmu), out(c * nmu * ntau * nphi, 0.0);
  for (long c0 = 0; c0 < C; c0 += window) {
    const int cnt = (int)std::min<long>(window, C - c0);
    RtdDev d{};
    d.C = cnt; d.L = L; d.P = P;
    d.omega = omega.data() + c0 * L; d.tau = tau.data() + c0 * L; d.taus0 = taus0.data() + c0 * (L + 1); d.scale = scale.data() + c0 * L;
    d.wleg = wleg.data() + c0 * L * P; d.mu0 = mu0.data() + c0; d.I0 = I0.data() + c0; d.phi0 = phi0.data() + c0; d.rescale = rescale.data() + c0;
    RtdNt nt{};
    nt.nleg_all = nall; nt.group = group; nt.c0 = group > 1 ? c0 : 0;  // (window_nt: shared rows are not offset, windows are not aligned to group)
    nt.wfull = wfull.data() + (group > 1 ? 0 : c0 * L * nall); nt.f = f.data() + c0 * L; nt.ims_coef = coef.data() + c0 * nall; nt.ims_par = par.data() + c0 * 2;
    RtdEval e{};
    e.ntau = ntau; e.nphi = nphi; e.antider = order < 0; e.deriv = order > 0;
    e.tau = evtau.data() + c0 * ntau; e.phi = phi.data();
    RtdNtView v{};
    v.nmu = nmu; v.mu_stride = per_column ? nmu : 0; v.mu = mu.data() + c0 * v.mu_stride; v.T = T.data();
    v.out = out.data() + c0 * nmu * ntau * nphi;
    rtd_launch_nt_view_tables(d, v, e.antider, nullptr);
    rtd_launch_nt_view_apply(d, nt, e, v, nullptr);
  }
  for (size_t i = 0; i < c; ++i) {
    for (size_t k = 0; k < (size_t)nmu * ntau * nphi; ++k) std::printf("%a ", out[i * nmu * ntau * nphi + k]);
    std::printf("\n");
  }
  return 0;
}
