// rtd_lambert.h -- the Lambertian coupling of two solutions (host and device): the arithmetic of rtd_lambert.hip, as routines that one
// thread runs for one (column, albedo) -- the factor kappa -- or for one output element.  rtd_api.hip launches them
// (rtd_plan_couple_lambert, rtd_plan_couple_lambert_band); tests/cpu runs the very same routines on the host.
//
// The adding formula of a Lambertian surface below a plane-parallel atmosphere, exact in the discrete-ordinate system:
//   x(A)  = x_black + kappa(A) x_below
//   kappa = (A F / pi + (1 - A) E) / (1 - A s)
// x_black: any field (u, u0, a flux, a view of either, in any tau-order) of the problem over a black, non-emitting surface;
// x_below: the same field of the source-free layers lit from below by unit isotropic intensity; F the downward flux (diffuse +
// direct, value order) of the black problem at the bottom; s the spherical albedo, flux_down of the lit-from-below problem at the
// bottom over pi; E the black-body emission of the surface, which enters with Kirchhoff's emissivity 1 - A.
//
//   rtd_lambert_kappa   the operations, in this order, each rounded once (u = 2^-53):
//                         g = F / RTD_LAMBERT_PI          division by the float64 nearest pi (itself within 0.4 u of pi)
//                         e = fma(-A, E, E)               (1 - A) E; exactly E at A = 0 and exactly 0 at A = 1
//                         n = fma(A, g, e)
//                         d = fma(-A, s, 1.0)             1 - A s
//                         kappa = n / d
//                       A g and e are not negative for admissible inputs (0 <= A <= 1, E >= 0, F >= 0), so n carries no
//                       cancellation: n = n_exact (1 + 3.4 u), d = d_exact (1 + u) for the inputs as given, and
//                         |kappa - kappa_exact| <= 6 u (A |F| / pi + (1 - A) E) / (1 - A s)          (RTD_LAMBERT_KAPPA_ULPS = 6)
//                       (5.4 u and the second-order terms; with F < 0 the bound holds in the magnitudes as written).
//                       *bad is set when d <= 0 or d or n is not finite: the formula has no meaning there (s >= 1 / A).
//   rtd_lambert_couple  fma(kappa, b, a), one rounding; kappa == 0 returns a itself, bit for bit (a signed zero included):
//                         |out - (a + kappa_exact b)| <= 8 u (|a| + |kappa b|)                       (RTD_LAMBERT_COUPLE_ULPS = 8)
//                       (u (|a| + |kappa b|) of the fma, 6 u |kappa b| of kappa, and their product).
// Both bounds are for results in the normal range (a product that underflows carries 2^-1075 absolutely instead).
// Every output is one fixed chain: the bits depend on the inputs alone.
#pragma once
#include "rtd_dd.h"

#define RTD_LAMBERT_PI 3.14159265358979323846
#define RTD_LAMBERT_KAPPA_ULPS 6
#define RTD_LAMBERT_COUPLE_ULPS 8

RTD_HD double rtd_lambert_kappa(const double A, const double F, const double s, const double E, int* bad) {
  const double g = F / RTD_LAMBERT_PI;
  const double e = __builtin_fma(-A, E, E);
  const double n = __builtin_fma(A, g, e);
  const double d = __builtin_fma(-A, s, 1.0);
  *bad = !(d > 0.0) || !(d <= 1.7976931348623157e308) || !(n >= -1.7976931348623157e308 && n <= 1.7976931348623157e308);
  return n / d;
}

RTD_HD double rtd_lambert_couple(const double a, const double b, const double kappa) {
  return kappa == 0.0 ? a : __builtin_fma(kappa, b, a);
}
