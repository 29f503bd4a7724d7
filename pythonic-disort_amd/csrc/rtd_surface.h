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
// The clamp of Ross-Li at 0 is DELIBERATE.  The kernels are fitted to moderate angles and are unbounded below at grazing ones: at
// the smallest double-Gauss node of 16 streams (0.020) the ordinary weights (0.3, 0.1, 0.05) give rho = -1.8, at 34 streams -9.  A
// negative reflectance makes the boundary-condition system of the solver unphysical; 0 is the nearest admissible value.
// The RPV denominator 1 + Theta^2 + 2 Theta cos xi is formed as (1 + Theta)^2 - 2 Theta h for Theta <= 0 and as
// (1 - Theta)^2 + 2 Theta g otherwise: the same number, as a sum of two non-negative terms.
// No table, no shared memory, no cross-lane operation: one thread, one sample.
#pragma once
#include "../../include/rtd.h"  // the model ids RTD_SURFACE_LAMBERT ... RTD_SURFACE_RPV = 0 ... 3
#include "rtd_dd.h"

enum { RTD_SURFACE_NMODELS = 4 };

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
    default: return par[0] >= 0.0 && par[1] > 0.0 && std::fabs(par[2]) < 1.0 ? nullptr : "rpv: need rho0 >= 0, k > 0, |Theta| < 1";
  }
}
