// rtd_nt_prep.h -- the column-level inputs of the Nakajima-Tanaka corrections (host and device): what the reference forms once per
// call in pydisort.py:601-611 (restated in pydisort_amd/_nt.py: nt_inputs), as routines that one thread runs for one output element
// (the moments) or one lane runs for its share of a column (the IMS constants).  rtd_api.hip launches them; tests/cpu runs the very
// same routines on the host.
//
//   rtd_mix_moment   moment k of a band's species mixture in one layer: sum_s omega_s dtau_s leg_s[k] / sum_s omega_s dtau_s, s
//                    ascending -- the ONE expression behind rtd_band_mix's moments and the band's full weighted phase function,
//                    which therefore agree bit for bit.  It does not depend on the spectral point.
//   rtd_nt_ims_lane  the IMS constants of one column, for the moments k = lane, lane + nlanes, ...:
//                      w_l = omega_l tau_arr[l]        (the CUMULATIVE tau_arr: the reference's convention, :601-610)
//                      omega_avg = sum w / sum tau_arr,   f_avg = sum f w / sum w
//                      r_k = sum_l resid_lk w_l / sum_l f_l w_l,   resid = f (k < nleg), the full moment (k >= nleg)
//                      ims_coef[k] = (2k + 1)(2 r_k - r_k^2)
//                      ims_par = (mu0 / (1 - omega_avg f_avg),  I0 / (4 pi) (omega_avg f_avg)^2 / (1 - omega_avg f_avg))
//                    Every sum is ONE chain, l ascending, in the calling lane: no atomics, no cross-lane reduction -- the bits depend
//                    on nothing but the inputs.  The three scalar sums are formed by every lane alike (L is tens); lane 0 writes
//                    ims_par.
//                    A column with sum f omega tau = 0 (nothing truncated, or nothing scatters) has no IMS term: the reference's
//                    formulas give 0 / 0 there.  Such a column gets ims_coef = 0, amplitude 0 and the scaled mu0 = mu0, so its
//                    IMS term is exactly 0 and its TMS term is what the formulas say.
#pragma once
#include "rtd_dd.h"

RTD_HD double rtd_mix_moment(const double* dt, const double* om, const double* lspec, int S, int nleg_all, int k) {
  double sca = 0.0, num = 0.0;
  for (int s = 0; s < S; ++s) {
    const double t = om[s] * dt[s];
    sca += t;
    num += t * lspec[(long)s * nleg_all + k];
  }
  return k == 0 ? 1.0 : sca != 0.0 ? num / sca : 0.0;
}

// tau, omega, f: the column's [L]; leg: the [L][nleg_all] full moments of the column's row; I0: the plan's rescaled beam
RTD_HD void rtd_nt_ims_lane(int L, int nleg, int nleg_all, const double* tau, const double* omega, const double* f, const double* leg,
                            double mu0, double I0, int lane, int nlanes, double* ims_coef, double* ims_par) {
  double sw = 0.0, st = 0.0, sfw = 0.0;
  for (int l = 0; l < L; ++l) {
    const double w = omega[l] * tau[l];
    sw += w;
    st += tau[l];
    sfw += f[l] * w;
  }
  const bool live = sfw > 0.0;
  for (int k = lane; k < nleg_all; k += nlanes) {
    double num = 0.0;
    for (int l = 0; l < L; ++l) {
      const double w = omega[l] * tau[l];
      num += (k < nleg ? f[l] : leg[(long)l * nleg_all + k]) * w;
    }
    const double r = live ? num / sfw : 0.0;
    ims_coef[k] = (2.0 * k + 1.0) * (2.0 * r - r * r);
  }
  if (lane == 0) {
    const double of = live ? (sw / st) * (sfw / sw) : 0.0;
    ims_par[0] = mu0 / (1.0 - of);
    ims_par[1] = I0 / (4.0 * 3.14159265358979323846) * (of * of) / (1.0 - of);
  }
}
