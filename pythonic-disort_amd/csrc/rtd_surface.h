// rtd_surface.h -- parametric surface reflectance models (host and device): rho(mu, mu', dphi) of a Lambertian surface, Hapke's
// soil, the Ross-Thick / Li-Sparse-Reciprocal kernels (MODIS BRDF product) and Rahman-Pinty-Verstraete, as ONE routine that a thread
// evaluates for one sample -- an element of rtd_surface_samples' array, or of the scratch block from which rtd_bdrf_modes_kernel
// forms a plan's BDRF Fourier modes (include/rtd.h: rtd_plan_request_surface).
//
// mu is the REFLECTED cosine, mu' the INCIDENT one, both in (0, 1]; the azimuth enters as c = cos dphi, s = sin dphi, where dphi is
// the difference of the PROPAGATION azimuths, as the reference's BDRF callables take it (pydisotest/6_test.py:11-24): backscatter
// -- the hot spot, the sun behind the observer -- is at dphi = pi.  All four models are reciprocal and depend on dphi through c and
// s^2 only, so the cosine series the solver uses is complete.
//
// Geometry.  With the scattering angle xi between the incident and the reflected direction (Hapke's phase angle alpha):
//   cos xi = mu mu' - sm sp c,   sm = sqrt((1 - mu)(1 + mu)),  sp likewise.
// At the hot spot cos xi -> 1 and arccos(cos xi) loses half its digits (the Hapke reflectance evaluated that way is off by 8e-8
// relative on the diagonal mu = mu', dphi = pi).  Everything below is therefore formed from the two half squared chords
//   h = 1 - cos xi = 1/2 [(sm c + sp)^2 + (sm s)^2 + (mu - mu')^2]      (unit vectors r and -i ... their distance squared / 2)
//   g = 1 + cos xi = 1/2 [(sm c - sp)^2 + (sm s)^2 + (mu + mu')^2]
// -- sums of squares, no cancellation; g >= (mu + mu')^2 / 2 > 0 -- as
//   cos xi = 1 - h,  tan(xi / 2) = sqrt(h / g),  sin xi = sqrt(h g),  xi = 2 asin(sqrt(h / 2))        (g = 2 - h)
//   ti = sm / mu,  tv = sp / mu',  sec = 1 / mu + 1 / mu',  D^2 = (ti - tv)^2 + 2 ti tv (1 + c).
//
// Models (par[4], unused entries 0):
//   RTD_SURFACE_LAMBERT  albedo                rho = albedo
//   RTD_SURFACE_HAPKE    B0, HH, W             rho = W / (4 (mu + mu')) [(1 + B) P + H(mu) H(mu') - 1],   B = B0 HH / (HH + tan(xi/2)),
//                                              P = 1 + cos(xi) / 2,  H(x) = (1 + 2x) / (1 + 2x sqrt(1 - W))          (6_test.py:11-24)
//   RTD_SURFACE_ROSSLI   f_iso, f_vol, f_geo   rho = max(0, f_iso + f_vol K_vol + f_geo K_geo), h/b = 2, b/r = 1:
//                                              K_vol = ((pi/2 - xi) cos xi + sin xi) / (mu + mu') - pi/4
//                                              cos t = min(1, 2 sqrt(D^2 + (ti tv s)^2) / sec),  O = (t - sin t cos t) sec / pi
//                                              K_geo = O - sec + (1 + cos xi) / (2 mu mu')
//   RTD_SURFACE_RPV      rho0, k, Theta, rho_c rho = rho0 (mu mu' (mu + mu'))^(k-1) (1 - Theta^2) / (1 + Theta^2 + 2 Theta cos xi)^(3/2)
//                                                    (1 + (1 - rho_c) / (1 + sqrt(D^2)));  Theta < 0 is backscattering
//   RTD_SURFACE_OCEAN    U, n, rho_w           the wind-roughened ocean (Cox-Munk glint, isotropic slopes): with sigma^2 = 0.003 + 0.00512 U,
//                                              the facet's incidence cos w = sqrt(g / 2), sin^2 w = 1 - g / 2, its tilt
//                                              mu_n^2 = (mu + mu')^2 / (2 g),  tan^2 b = [(sm c - sp)^2 + (sm s)^2] / (mu + mu')^2,
//                                              F = 1/2 [((cos w - r) / (cos w + r))^2 + ((n^2 cos w - r) / (n^2 cos w + r))^2], r = sqrt(n^2 - sin^2 w),
//                                              S = 1 / (1 + L(mu) + L(mu')),  L(x) = max(0, 1/2 [exp(-v^2) / (sqrt(pi) v) - erfc v]),
//                                              v = x / (sigma sqrt((1 - x)(1 + x))),  L(1) = 0:
//                                              rho = F exp(-tan^2 b / sigma^2) S / (4 sigma^2 mu mu' mu_n^4) + rho_w
//                                              The glint is at dphi = 0 (propagation azimuths); tan^2 b is a sum of squares like g.
// The clamp of Ross-Li at 0 is DELIBERATE.  The kernels are fitted to moderate angles and are unbounded below at grazing ones: at
// the smallest double-Gauss node of 16 streams (0.020) the ordinary weights (0.3, 0.1, 0.05) give rho = -1.8, at 34 streams -9.  A
// negative reflectance makes the boundary-condition system of the solver unphysical; 0 is the nearest admissible value.
// The RPV denominator 1 + Theta^2 + 2 Theta cos xi is formed as (1 + Theta)^2 - 2 Theta h for Theta <= 0 and as
// (1 - Theta)^2 + 2 Theta g otherwise: the same number, as a sum of two non-negative terms.
// The shadowing S of the ocean is ALWAYS ON, and that is DELIBERATE too.  Without it the hemispherical albedo
// Sum_j 2 mu_j w_j q^0(mu_i, mu_j) at the smallest node exceeds 1 from 16 streams upward (1.26 at 16 streams and U = 5 m/s, 4.8 at 34
// streams, 17.9 at 64 streams and U = 15): a surface that reflects more than it receives.  With it the worst value over U = 0, 1, 5,
// 15 and 6 / 16 / 34 / 64 streams is 0.74 (tests/test_surface_ocean_cpu.py holds albedo <= 1 at every node).  For large v the
// difference inside L cancels in relative terms, which is harmless next to the 1 in S; at x = 1 (v infinite) L is set to 0 rather
// than formed as exp(-inf) / inf, and an exponential that underflows to 0 is the right answer.
// No table, no shared memory, no cross-lane operation: one thread, one sample.
//
// The ocean's clustered azimuth rule (csrc/rtd_surface_ocean.hip forms the modes with it; tools/surface_ocean_truth.py shares every
// definition here).  The glint's azimuthal width at a pair of cosines is delta = sigma (mu + mu') / sqrt(sm sp), 1e-3 rad at grazing
// pairs of 34 or 64 streams, which a uniform grid cannot afford.  With psi_p = 2 pi p / nphi uniform,
//   dphi(psi) = psi - a sin psi = b psi + a (psi - sin psi),   weight (1 - a cos psi_p) / nphi = (b + 2 a sin^2(psi_p / 2)) / nphi,   a = 1 - b,
// is periodic and analytic in psi, so the trapezoid rule stays spectral, and its nodes crowd at dphi = 0 with spacing b 2 pi / nphi.
// b is rtd_ocean_cluster_b below: min(1, 2 delta) formed in float64, ROUNDED TO FLOAT32 and held in [2^-20, 1]; 1 (a = 0, the
// uniform grid) when sm sp = 0.  The rounding to float32 is what lets a truth in other arithmetic share the rule: a last-bit
// difference in delta (another sqrt, a contracted multiply-add) moves b only if delta sits within 1e-16 of a float32 rounding
// boundary; a = 1 - b is then exact in float64.  Both forms above are sums of non-negative terms.
#pragma once
#include "../../include/rtd.h"  // the model ids RTD_SURFACE_LAMBERT ... RTD_SURFACE_OCEAN = 0 ... 4
#include "rtd_dd.h"

enum { RTD_SURFACE_NMODELS = 5 };

// cos(pi x), sin(pi x) for 0 <= x < 2: the device's cospi / sinpi; on the host the argument is reduced exactly first (x = 2 p / nphi:
// the quadrant boundaries are hit exactly, so dphi = pi/2, pi, 3 pi/2 give exact zeros and ones there too)
RTD_HD void rtd_surface_cs(const double x, double* c, double* s) {
#if defined(__HIP_DEVICE_COMPILE__)
  *c = cospi(x);
  *s = sinpi(x);
#else
  const double pi = 3.141592653589793238462643383279502884;
  const int q = (int)(2.0 * x + 0.5);  // nearest multiple of 1/2
  const double r = x - 0.5 * q;        // exact: |r| <= 1/4
  const double cr = std::cos(pi * r), sr = std::sin(pi * r);
  switch (q & 3) {
    case 0: *c = cr; *s = sr; break;
    case 1: *c = -sr; *s = cr; break;
    case 2: *c = -cr; *s = -sr; break;
    default: *c = sr; *s = -cr; break;
  }
#endif
}

// The ocean's slope variance (Cox and Munk 1954, isotropic) and its shadowing term L(x) (clamped at 0; 0 at x = 1 and beyond the
// underflow of exp(-v^2))
RTD_HD double rtd_ocean_sigma2(const double U) { return 0.003 + 0.00512 * U; }
RTD_HD double rtd_ocean_lambda(const double x, const double sig) {
  if (!(x < 1.0)) return 0.0;
  const double v = x / (sig * sqrt((1.0 - x) * (1.0 + x)));
  return fmax(0.0, 0.5 * (exp(-v * v) / (1.7724538509055160272981674833411 * v) - erfc(v)));
}

// b = 1 - a of the ocean's clustered azimuth rule for one pair of cosines (the header's comment defines it): float32(min(1, 2 delta))
// held in [2^-20, 1]; 1 when sm sp = 0 (delta infinite: the division is never made)
RTD_HD double rtd_ocean_cluster_b(const double U, const double mu, const double mup) {
  const double sm = sqrt((1.0 - mu) * (1.0 + mu)), sp = sqrt((1.0 - mup) * (1.0 + mup)), q = sm * sp;
  if (!(q > 0.0)) return 1.0;
  const double d2 = 2.0 * sqrt(rtd_ocean_sigma2(U)) * (mu + mup) / sqrt(q);
  if (!(d2 < 1.0)) return 1.0;
  return fmax((double)(float)d2, 1.0 / 1048576.0);
}

RTD_HD double rtd_surface_rho(const int model, const double* par, const double mu, const double mup, const double c, const double s) {
  if (model == RTD_SURFACE_LAMBERT) return par[0];
  const double pi = 3.141592653589793238462643383279502884;
  const double sm = sqrt((1.0 - mu) * (1.0 + mu)), sp = sqrt((1.0 - mup) * (1.0 + mup));
  const double ss = sm * s, dm = mu - mup, sm_ = mu + mup, a = sm * c + sp, b = sm * c - sp;
  const double h = 0.5 * (a * a + ss * ss + dm * dm);    // 1 - cos xi
  const double g = 0.5 * (b * b + ss * ss + sm_ * sm_);  // 1 + cos xi
  const double cosxi = 1.0 - h;
  if (model == RTD_SURFACE_HAPKE) {
    const double B0 = par[0], HH = par[1], W = par[2];
    const double B = B0 * HH / (HH + sqrt(h / g));
    const double P = 1.0 + 0.5 * cosxi;
    const double gam = sqrt(1.0 - W);
    const double H0 = (1.0 + 2.0 * mup) / (1.0 + 2.0 * mup * gam), H = (1.0 + 2.0 * mu) / (1.0 + 2.0 * mu * gam);
    return W / 4.0 / (mu + mup) * ((1.0 + B) * P + H0 * H - 1.0);
  }
  if (model == RTD_SURFACE_OCEAN) {
    const double n2 = par[1] * par[1], sig2 = rtd_ocean_sigma2(par[0]), sig = sqrt(sig2);
    const double cw = sqrt(0.5 * g), r = sqrt(n2 - (1.0 - 0.5 * g));  // (n > 1 >= sin^2 w: r > 0)
    const double fs = (cw - r) / (cw + r), fp = (n2 * cw - r) / (n2 * cw + r);
    const double F = 0.5 * (fs * fs + fp * fp);
    const double mun2 = sm_ * sm_ / (2.0 * g);  // (facet normal's cosine)^2, <= 1
    const double tan2 = (b * b + ss * ss) / (sm_ * sm_);
    const double S = 1.0 / (1.0 + rtd_ocean_lambda(mu, sig) + rtd_ocean_lambda(mup, sig));
    return F * exp(-tan2 / sig2) * S / (4.0 * sig2 * mu * mup * mun2 * mun2) + par[2];
  }
  const double ti = sm / mu, tv = sp / mup, sec = 1.0 / mu + 1.0 / mup, dt = ti - tv;
  const double D2 = dt * dt + 2.0 * ti * tv * (1.0 + c);
  if (model == RTD_SURFACE_ROSSLI) {
    const double sinxi = sqrt(h * g);
    const double xi = 2.0 * asin(sqrt(0.5 * h));
    const double Kvol = ((0.5 * pi - xi) * cosxi + sinxi) / (mu + mup) - 0.25 * pi;
    const double tts = ti * tv * s;
    const double cost = fmin(1.0, 2.0 * sqrt(D2 + tts * tts) / sec);
    const double t = acos(cost), sint = sqrt((1.0 - cost) * (1.0 + cost));
    const double O = (t - sint * cost) * sec / pi;
    const double Kgeo = O - sec + g / (2.0 * mu * mup);
    return fmax(0.0, par[0] + par[1] * Kvol + par[2] * Kgeo);
  }
  // RTD_SURFACE_RPV
  const double rho0 = par[0], k = par[1], Th = par[2], rhoc = par[3];
  const double den = Th <= 0.0 ? (1.0 + Th) * (1.0 + Th) - 2.0 * Th * h : (1.0 - Th) * (1.0 - Th) + 2.0 * Th * g;
  const double F = (1.0 - Th) * (1.0 + Th) / (den * sqrt(den));
  return rho0 * pow(mu * mup * (mu + mup), k - 1.0) * F * (1.0 + (1.0 - rhoc) / (1.0 + sqrt(D2)));
}

// The parameter ranges (host): nullptr when par[4] is admissible for `model`, else what is wrong with it.
inline const char* rtd_surface_bad(const int model, const double* par) {
  if (model < 0 || model >= RTD_SURFACE_NMODELS) return "unknown model";
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(par[k])) return "parameters must be finite";
  switch (model) {
    case RTD_SURFACE_LAMBERT: return par[0] >= 0.0 && par[0] <= 1.0 ? nullptr : "lambert: need 0 <= albedo <= 1";
    case RTD_SURFACE_HAPKE: return par[0] >= 0.0 && par[1] > 0.0 && par[2] > 0.0 && par[2] <= 1.0 ? nullptr : "hapke: need B0 >= 0, HH > 0, 0 < W <= 1";
    case RTD_SURFACE_ROSSLI: return par[0] >= 0.0 && par[1] >= 0.0 && par[2] >= 0.0 ? nullptr : "rossli: need f_iso, f_vol, f_geo >= 0";
    case RTD_SURFACE_RPV: return par[0] >= 0.0 && par[1] > 0.0 && std::fabs(par[2]) < 1.0 ? nullptr : "rpv: need rho0 >= 0, k > 0, |Theta| < 1";
    default: return par[0] >= 0.0 && par[1] > 1.0 && par[2] >= 0.0 ? nullptr : "ocean: need U >= 0, n > 1, rho_w >= 0";
  }
}
