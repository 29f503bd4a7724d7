// rtd_nt_view.h -- the Nakajima-Tanaka corrections (TMS + IMS) at an ARBITRARY polar-angle cosine (host and device): the arithmetic of
// rtd_nt_view.hip, as routines that one thread runs for one (column, angle) -- the other-layer sums -- or for one output element.
// tests/cpu runs the very same routines on the host.
//
// The formulas are those of rtd_nt.hip (pydisort.py:409-638), which evaluates them at the quadrature nodes only and is safe there
// because a node is almost never a special value.  A viewing angle routinely is one: an almucantar scan has mu = -mu0 exactly.  With
// a = |mu|, D the scaled depth below the top of a segment (the point's layer down to the point, or a whole layer above it):
//
//   TMS, downward.  mu0 / (mu0 - a) (e^{-D/mu0} - e^{-D/a}) is infinity times zero at a = mu0.  With z = D (1/a - 1/mu0), formed as
//     D (mu0 - a) / (a mu0) -- the difference of nearby numbers is exact -- the factor folds in:
//       mu0 / (mu0 - a) (e^{-D/mu0} - e^{-D/a}) = (D / a) phi1(|z|) e^{-D / max(mu0, a)},   phi1(z) = -expm1(-z) / z,  phi1(0) = 1
//     (z >= 0: e^{-D/mu0} is factored out, z < 0: e^{-D/a}; so nothing overflows for a thick layer).  Call that H.  The other orders
//     follow from H and the two exponentials without a second cancellation:
//       derivative      mu0 / (mu0 - a) (-e^{-D/mu0} / mu0 + e^{-D/a} / a) = e^{-D/a} / a - H / mu0
//       antiderivative  mu0 / (mu0 - a) (-mu0 e^{-D/mu0} + a e^{-D/a})     = -(a H + mu0 e^{-D/mu0})
//     (times scale / 1 / scale of the layer).  The same H, over a whole layer, is what every layer above the point contributes.
//   TMS, upward.  mu0 / (mu0 + a) has no pole; the in-layer value att - e is formed as -att expm1(-(tb - t)(1/a + 1/mu0)), which keeps
//     its digits as the point nears the bottom of its layer.
//   IMS (downward only).  x = 1/a - 1/s, s the scaled mu0 (ims_par[0]); chi divides by x^2.  With z = tau x = tau (s - a) / (a s),
//     e0 = e^{-tau/s}, e1 = e^{-tau/a} and psi2(z) = (e^{-z} - 1 + z) / z^2:
//       value           chi = tau^2 Psi / (a s),                       Psi = e0 psi2(z)
//       derivative      (-tau^2 Psi / s + tau Phi) / (a s),            Phi = e0 phi1(z)
//       antiderivative  -(tau^2 Psi / s + e0 (s + tau))                (the reference's closed form :619-623, rearranged exactly)
//     For z < 0 (a > s) e0 e^{-z} = e1 is used in place of e^{-z}, so a large tau cannot overflow: Psi = e1 (1 - (1 + w) e^{-w}) / w^2,
//     Phi = e1 phi1(w), w = -z.
//     psi2's closed form cancels to z^2 / 2 from terms of size z: it loses 2 eps / |z|.  Below |z| = 1/2 the series
//     sum_k (-z)^k / (k + 2)! is used instead: k <= 16, remainder below (1/2)^17 / 19! = 6.3e-23 against psi2 >= 0.42 there; at the
//     threshold the closed form is within 4 eps.  The series serves both signs of z (no exponential of z is formed there).
//   mu = +-1: sqrt(1 - mu^2) = 0 and nothing else is special.  Tiny |mu|: the exponentials underflow to zero, which is their limit.
//   mu = 0 has no closed form of this kind (the plane-parallel limit differs by hemisphere): rtd_api.hip refuses it in this mode.
#pragma once
#include "rtd_dd.h"

RTD_HD double rtd_ntv_phi1(const double z) {  // z >= 0
  return z > 0.0 ? -expm1(-z) / z : 1.0;
}

RTD_HD double rtd_ntv_psi2_series(const double z) {  // |z| < 1/2
  double s = 1.0 / 6402373705728000.0;  // 1 / 18!
  const double inv[15] = {1.0 / 355687428096000.0, 1.0 / 20922789888000.0, 1.0 / 1307674368000.0, 1.0 / 87178291200.0,
                          1.0 / 6227020800.0,      1.0 / 479001600.0,      1.0 / 39916800.0,      1.0 / 3628800.0,
                          1.0 / 362880.0,          1.0 / 40320.0,          1.0 / 5040.0,          1.0 / 720.0,
                          1.0 / 120.0,             1.0 / 24.0,             1.0 / 6.0};  // 1 / 17! ... 1 / 3!
  for (int k = 0; k < 15; ++k) s = inv[k] - z * s;
  return 0.5 - z * s;
}

// Psi = e0 psi2(z) and Phi = e0 phi1(z), e1 = e0 e^{-z} given: sided so that no exponential of z grows
RTD_HD void rtd_ntv_psi_phi(const double z, const double e0, const double e1, double* Psi, double* Phi) {
  if (z >= 0.0) {
    *Phi = e0 * rtd_ntv_phi1(z);
    *Psi = e0 * (z < 0.5 ? rtd_ntv_psi2_series(z) : (expm1(-z) + z) / (z * z));
  } else {
    const double w = -z;
    *Phi = e1 * rtd_ntv_phi1(w);
    *Psi = w < 0.5 ? e0 * rtd_ntv_psi2_series(z) : e1 * ((-expm1(-w) - w * exp(-w)) / (w * w));
  }
}

// H = mu0 / (mu0 - a) (E0 - Ea) from the two attenuations themselves: E0 = pre e^{-D/mu0}, Ea = pre e^{-D/a}, D >= 0
RTD_HD double rtd_ntv_fold(const double D, const double a, const double mu0, const double E0, const double Ea) {
  const double z = D * (mu0 - a) / (a * mu0);
  return (D / a) * rtd_ntv_phi1(fabs(z)) * (z >= 0.0 ? E0 : Ea);
}

// The other-layer sums of one (column, angle), for the hemisphere of mu only, T[l * stride], l < L (pydisort.py:489-589), with the
// factor mu0 / (mu0 +- a) folded in.  antider: each layer's term carries +-a / scale[r] (:513-515, :524, :570); the derivative reads
// the value's sums.  O(L): upward  T[l-1] = X_l + e^{-dt_l/a} T[l]  from the bottom, downward  T[l+1] = X_l + e^{-dt_l/a} T[l]  from
// the top; per layer one exp(-dt/a), one exp(-t/mu0) and one expm1.  One chain per output, l in a fixed order.
RTD_HD void rtd_ntv_table(const int L, const double* ts0, const double* sc, const double mu, const double mu0, const int antider,
                          double* T, const long stride) {
  const double a = fabs(mu);
  if (mu > 0.0) {
    const double g = mu0 / (mu0 + a), rate = 1.0 / a + 1.0 / mu0;
    double acc = 0.0;
    T[(long)(L - 1) * stride] = 0.0;
    for (int l = L - 1; l >= 1; --l) {
      const double dt = ts0[l + 1] - ts0[l];
      double X = g * -expm1(-dt * rate) * exp(-ts0[l] / mu0);
      if (antider) X *= a / sc[l];
      acc = X + exp(-dt / a) * acc;
      T[(long)(l - 1) * stride] = acc;
    }
  } else {
    double acc = 0.0, etop = 1.0;  // e^{-ts0[l] / mu0}, carried from layer to layer (ts0[0] = 0)
    T[0] = 0.0;
    for (int l = 0; l + 1 < L; ++l) {
      const double dt = ts0[l + 1] - ts0[l];
      const double ea = exp(-dt / a), ebot = exp(-ts0[l + 1] / mu0);
      double X = rtd_ntv_fold(dt, a, mu0, ebot, etop * ea);
      if (antider) X *= -a / sc[l];
      acc = X + ea * acc;
      T[(long)(l + 1) * stride] = acc;
      etop = ebot;
    }
  }
}

// what the angles and azimuths of one (column, tau) point share
struct RtdNtvPoint {
  int order;             // -1 the tau-antiderivative, 0 the value, +1 the tau-derivative
  int others;            // L > 1: the other-layer sums enter
  double tau, ts, tt, tb, sc;  // the point, its scaled depth, the scaled top and bottom of its layer, the layer's scale
  double dtop, dbot;     // the scaled depth of the point below its layer's top and above its bottom, EACH formed from the unscaled
                         // difference times sc: exactly 0 at the boundary and accurate relative to itself.  ts - tt and tb - ts carry
                         // eps ts instead, which 1 / |mu| amplifies: 1e3 eps at |mu| = 1e-3 and tau = 0, where e^{-D/a} = 1 is the whole term
  double mu0, att;       // att = e^{-ts / mu0}
  double smu0;           // the IMS scaled mu0
};

// The TMS attenuation factor of the point at mu (factor mu0 / (mu0 +- a) included; Tl = the angle's other-layer sum of the point's
// layer) and, for mu < 0, the IMS chi; *chi = 0 for mu > 0.
RTD_HD void rtd_ntv_factors(const RtdNtvPoint& q, const double mu, const double Tl, double* tms, double* chi) {
  const double a = fabs(mu), sc = q.sc, mu0 = q.mu0;
  if (mu > 0.0) {
    const double g = mu0 / (mu0 + a), down = q.dbot;
    const double ea = exp(-down / a), e = ea * exp(-q.tb / mu0);
    double fac;
    if (q.order < 0) fac = -g * (mu0 * q.att + a * e) / sc;
    else if (q.order > 0) fac = -g * sc * (q.att / mu0 + e / a);
    else fac = g * q.att * -expm1(-down * (1.0 / a + 1.0 / mu0));
    if (q.others) fac += q.order > 0 ? Tl * ea * (sc / a) : Tl * ea;
    *tms = fac;
    *chi = 0.0;
    return;
  }
  const double D = q.dtop;
  const double ea = exp(-D / a), e = ea * exp(-q.tt / mu0);
  const double H = rtd_ntv_fold(D, a, mu0, q.att, e);
  double fac;
  if (q.order < 0) fac = -(a * H + mu0 * q.att) / sc;
  else if (q.order > 0) fac = sc * (e / a - H / mu0);
  else fac = H;
  if (q.others) fac += q.order > 0 ? Tl * ea * (-sc / a) : Tl * ea;
  *tms = fac;
  const double s = q.smu0, tau = q.tau;
  const double z = tau * (s - a) / (a * s), e0 = exp(-tau / s), e1 = exp(-tau / a);
  double Psi, Phi;
  rtd_ntv_psi_phi(z, e0, e1, &Psi, &Phi);
  if (q.order < 0) *chi = -(tau * tau * Psi / s + e0 * (s + tau));
  else if (q.order > 0) *chi = (-tau * tau * Psi / s + tau * Phi) / (a * s);
  else *chi = tau * tau * Psi / (a * s);
}

// ONE pass of the forward Legendre recurrence at nu with the three series accumulated side by side, each k ascending:
//   *tms = sum_k wfull[k] P_k / (1 - f) - sum_{k < P} wtrun[k] P_k,   *ims = sum_k imsc[k] P_k  (only when want_ims)
RTD_HD void rtd_ntv_series(const double* wfull, const double* imsc, const int nall, const double* wtrun, const int P, const double one_m_f,
                           const double nu, const bool want_ims, double* tms, double* ims) {
  double pm1 = 1.0, p = nu;
  double full = nall > 0 ? wfull[0] : 0.0, trun = P > 0 ? wtrun[0] : 0.0, is = (want_ims && nall > 0) ? imsc[0] : 0.0;
  if (nall > 1) full += wfull[1] * nu;
  if (P > 1) trun += wtrun[1] * nu;
  if (want_ims && nall > 1) is += imsc[1] * nu;
  const int n = nall > P ? nall : P;
  for (int l = 1; l + 1 < n; ++l) {
    const double pn = ((2.0 * l + 1.0) * nu * p - l * pm1) / (l + 1.0);
    pm1 = p;
    p = pn;
    if (l + 1 < nall) {
      full += wfull[l + 1] * p;
      if (want_ims) is += imsc[l + 1] * p;
    }
    if (l + 1 < P) trun += wtrun[l + 1] * p;
  }
  *tms = full / one_m_f - trun;
  *ims = is;
}
