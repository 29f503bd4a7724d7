// rtd_nt_view.hip -- Nakajima-Tanaka intensity corrections (TMS + IMS) evaluated at the viewing angles themselves.
//
// rtd_nt.hip adds the corrections to u at the quadrature nodes; a radiance at a user polar angle interpolated from that u carries the
// forward peak of the full phase function only as far as a polynomial through the nodes can.  The corrections are closed forms of the
// inputs and of (mu, tau, phi), so here they are evaluated AT the requested angles and added to the interpolant of the uncorrected u
// (rtd_api.hip: launch_windows, rtd_plan_set_view_nt).  The arithmetic -- with the forms that stay finite and accurate where the node
// formulas are infinity times zero (|mu| = mu0, |mu| = the IMS scaled mu0) -- is rtd_nt_view.h, shared with the host.
//
//   rtd_nt_view_tables_kernel  the other-layer sums of every (column, angle) for the hemisphere of that angle and the tau-order of this
//                              evaluation, T [C][L][nmu]: O(L) prefix / suffix recurrences, each layer's exp and expm1 formed once.
//                              One thread per (column, angle), the angle fastest: a wavefront's stores of one layer are consecutive.
//   rtd_nt_view_apply_kernel   out [C][nmu][ntau][nphi] += rescale * (TMS + IMS).  One workgroup per (column, tau) point, its threads
//                              over (angle, azimuth): the layer of the point, hence the rows of the three Legendre series, are the same
//                              for the whole workgroup (uniform loads, no staging in LDS), and P_l(nu) runs ONCE per output with the
//                              full, the truncated and the IMS series accumulated side by side.  Every output is one chain of
//                              additions in a fixed order, written by one thread: no atomics, no cross-lane reduction, so the bits
//                              depend on neither the launch geometry nor the window size.
// Thread mapping: chosen for the uniform coefficient rows; with few angles and azimuths per point (one angle, one azimuth: one active
// lane per workgroup) most lanes idle, and a mapping with the points across the lanes would fill them at the price of divergent row
// addresses.  The two were NOT measured against each other; tools/nt_view_timing.py records what this one costs.  The launch bounds
// are the launchers' largest workgroups (64 and 256): without them the compiler budgets the registers of a 1024-thread workgroup and
// the apply kernel spills (10 VGPRs, 44 bytes of scratch per lane in the code object's metadata).
#include "rtd_device.h"
#include "rtd_nt_view.h"

namespace {

__global__ void __launch_bounds__(64) rtd_nt_view_tables_kernel(RtdDev d, RtdNtView v, int antider) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (c, m)
  if (idx >= (long)d.C * v.nmu) return;
  const int m = (int)(idx % v.nmu), L = d.L;
  const long c = idx / v.nmu;
  rtd_ntv_table(L, d.taus0 + c * (L + 1), d.scale + c * L, v.mu[c * v.mu_stride + m], d.mu0[c], antider, v.T + c * L * v.nmu + m, v.nmu);
}

__global__ void __launch_bounds__(256) rtd_nt_view_apply_kernel(RtdDev d, RtdNt nt, RtdEval ev, RtdNtView v) {
  const int t = (int)(blockIdx.x % ev.ntau), L = d.L;
  const long c = blockIdx.x / ev.ntau;
  const double* tau_arr = d.tau + c * L;
  const double* ts0 = d.taus0 + c * (L + 1);
  RtdNtvPoint q;
  q.tau = ev.tau[c * ev.ntau + t];
  int l = 0;
  while (l < L - 1 && !(q.tau <= tau_arr[l])) ++l;  // the layer of the point, as rtd_nt_apply_kernel finds it
  q.order = ev.deriv != 0 ? 1 : ev.antider != 0 ? -1 : 0;
  q.others = L > 1;
  q.sc = d.scale[c * L + l];
  q.dtop = (q.tau - (l > 0 ? tau_arr[l - 1] : 0.0)) * q.sc;
  q.dbot = (tau_arr[l] - q.tau) * q.sc;
  q.ts = ts0[l + 1] - q.dbot;
  q.tb = ts0[l + 1];
  q.tt = ts0[l];
  q.mu0 = d.mu0[c];
  q.att = exp(-q.ts / q.mu0);
  q.smu0 = nt.ims_par[c * 2 + 0];
  const double amp = nt.ims_par[c * 2 + 1], phi0 = d.phi0[c];
  const double tms_amp = d.omega[c * L + l] * (d.I0[c] / (4.0 * 3.14159265358979323846));
  const double one_m_f = 1.0 - nt.f[c * L + l];
  const double* wfull = nt.wfull + (((nt.c0 + c) / nt.group) * L + l) * nt.nleg_all;  // (group 1: c0 = 0, the view's own rows)
  const double* wtrun = d.wleg + (c * L + l) * d.P;
  const double* imsc = nt.ims_coef + c * nt.nleg_all;
  const double s0 = sqrt(1.0 - q.mu0 * q.mu0), rescale = d.rescale[c];
  const double* Tl = v.T + (c * L + l) * v.nmu;
  for (int idx = threadIdx.x; idx < v.nmu * ev.nphi; idx += blockDim.x) {
    const int m = idx / ev.nphi, p = idx % ev.nphi;
    const double mu = v.mu[c * v.mu_stride + m];
    const double nu = -q.mu0 * mu + s0 * sqrt(1.0 - mu * mu) * cos(phi0 - ev.phi[p]);
    double tms, chi, series, ims;
    rtd_ntv_factors(q, mu, q.others ? Tl[m] : 0.0, &tms, &chi);
    rtd_ntv_series(wfull, imsc, nt.nleg_all, wtrun, d.P, one_m_f, nu, !(mu > 0.0), &series, &ims);
    double corr = tms_amp * series * tms;
    if (!(mu > 0.0)) corr += amp * ims * chi;
    v.out[((c * v.nmu + m) * ev.ntau + t) * ev.nphi + p] += rescale * corr;
  }
}

}  // namespace

void rtd_launch_nt_view_tables(const RtdDev& d, const RtdNtView& v, int antider, hipStream_t s) {
  if (d.L < 2) return;  // one layer: no other-layer sums, and the apply kernel reads none
  const long n = (long)d.C * v.nmu;
  hipLaunchKernelGGL(rtd_nt_view_tables_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d, v, antider);
}

void rtd_launch_nt_view_apply(const RtdDev& d, const RtdNt& nt, const RtdEval& e, const RtdNtView& v, hipStream_t s) {
  const long per_point = (long)v.nmu * e.nphi;
  const unsigned block = (unsigned)(per_point >= 256 ? 256 : 64 * ((per_point + 63) / 64));
  hipLaunchKernelGGL(rtd_nt_view_apply_kernel, dim3((unsigned)((long)e.ntau * d.C)), dim3(block), 0, s, d, nt, e, v);
}
