// rtd_planck.h -- the band-integrated Planck function (host and device): what the reference's thermal helpers obtain from
// scipy.integrate.quad_vec over Planck(T, WVNM) (subroutines.py:322-350, :354-377, :413-454), as ONE closed routine that a
// thread evaluates for one (temperature, band) -- the level emissions of a column, its boundary emissions, or an element of
// rtd_planck_band's arrays (include/rtd.h).
//
//   E(T, lo, hi) = Int_lo^hi 2e8 h c^2 nu^3 e^-x / (1 - e^-x) dnu,   x = 100 h c nu / (k T)        [W / m^2; nu in cm^-1]
//                = 2e8 h c^2 (T / c2)^4  Int_xlo^xhi x^3 / (e^x - 1) dx,   c2 = 100 h c / k
//
// with the exact SI values of h, c, k (those of scipy.constants).  Evaluation: composite 10-point Gauss-Legendre panels of at
// most 2 in x (the integrand's nearest poles are at +-2 pi i: the rule is exact to below 1e-17 of a panel), summed compensated.
//  * The integrand is taken relative to the band's lower end: x^3 e^-(x - xlo) / (1 - e^-x), with 1 - e^-x from expm1, and the
//    factor e^-xlo is applied once at the end, in two halves -- nothing overflows, the Rayleigh-Jeans end (x -> 0) keeps its
//    digits, and the Wien tail (x ~ 1150 at 100 K, 80 000 cm^-1) loses precision only where the RESULT is subnormal.
//  * The panels are laid from xlo by offsets d = x - xlo, and the band's width in x comes from (hi - lo), never from xhi - xlo:
//    a band of relative width 7e-6 (2702.99 ... 2703.01) cancels nothing.
//  * xlo itself is carried as a double-double (c2 lo / T with its rounding error): e^-xlo would otherwise be xlo ulps off.
//  * Beyond max(xlo, 3) + 50 the integrand is below 2^-53 of the result; the panels stop there (<= 27 panels, 270 nodes).
// No table, no shared memory, no cross-lane operation: one thread, one integral.
#pragma once
#include "rtd_dd.h"

RTD_HD double rtd_planck_band(double T, double wvnmlo, double wvnmhi) {
  if (T == 0.0 || wvnmlo == wvnmhi) return 0.0;
  double sign = 1.0;
  if (wvnmlo > wvnmhi) {
    const double t = wvnmlo;
    wvnmlo = wvnmhi;
    wvnmhi = t;
    sign = -1.0;
  }
  const double c2 = 1.4387768775039338, c2_lo = 8.967968474929929e-18;  // 100 h c / k [cm K], head and tail
  const double c1 = 1.1910429723971885e-08;                             // 2e8 h c^2
  // nodes and weights of the 10-point Gauss-Legendre rule on [-1, 1] (symmetric: the positive half)
  constexpr double xg[5] = {0.14887433898163121, 0.43339539412924719, 0.67940956829902441, 0.86506336668898451,
                            0.97390652851717172};
  constexpr double wg[5] = {0.29552422471475287, 0.26926671930999636, 0.21908636251598204, 0.14945134915058059,
                            0.066671344308688138};
  // xlo = c2 lo / T = q + r
  const rtd_dd p = rtd_two_prod(c2, wvnmlo);
  const double q = p.hi / T;
  const double r = (fma(-q, T, p.hi) + fma(c2_lo, wvnmlo, p.lo)) / T;
  double w = c2 * (wvnmhi - wvnmlo) / T;  // xhi - xlo
  w = fmin(w, 50.0 + fmax(3.0 - q, 0.0));
  int n = (int)ceil(0.5 * w);
  if (n < 1) n = 1;
  const double hh = 0.5 * w / n;  // half a panel
  rtd_dd acc = {0.0, 0.0};
  for (int k = 0; k < n; ++k) {
    const double mid = (2 * k + 1) * hh;
    for (int j = 0; j < 5; ++j)
      for (int s = -1; s <= 1; s += 2) {
        const double d = fma(s * hh, xg[j], mid), x = q + d;
        const double f = x > 0.0 ? x * x * x * exp(-d) / -expm1(-x) : 0.0;
        acc = rtd_two_sum(acc.hi, fma(wg[j], f, acc.lo));
      }
  }
  const double t = T / c2, t2 = t * t, e = exp(-0.5 * q);
  return sign * (c1 * (t2 * t2) * (hh * (acc.hi + acc.lo)) * e) * e * (1.0 - r);
}
