// rtd_dd.h -- double-double helpers (host and device) for the ONE place where the path needs more than float64: moving the
// origin of the thermal source polynomials from tau = 0 to the top of their own layer.
//
// The reference gives the isotropic source of layer l as a polynomial in the ABSOLUTE optical depth, s_l(tau) = sum_j a_j tau^j
// (pydisort.py:316-338 -> scaled_s_poly_coeffs; subroutines.py:746-862 builds the particular solution sum_q b_q(K) tau^q from
// it).  Deep in an atmosphere every float64 evaluation of such a polynomial cancels (a_0 and a_1 tau are both ~ tau_top / dtau
// times the source): the particular solution at the two sides of an interface, in the rows of the boundary-condition system and
// in the evaluators is then consistent to eps x tau_top / dtau only (test 8ARTS_A: 3e-5 pointwise at intensities 1e-6 of the
// largest).  The device therefore keeps the coefficients about the top of the layer: s_l(tau) = sum_i b_i (tau - tau_top)^i, and
// so the particular solution (its construction is translation invariant).  b = Taylor shift of a, done ONCE in double-double --
// exact to the last bit of the result for the coefficients as given, whatever their number -- instead of implicitly, in float64, at every evaluation.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RTD_HD __host__ __device__ __forceinline__
#else
#define RTD_HD inline
#endif
#include <cmath>

// The error-free transformations below are identities of ROUNDED sums and products.  A compiler that contracts a * b + c into one
// fused operation -- the default for device code -- puts an exact product where they count on the rounded one and leaves float64
// accuracy behind (measured on gfx950: 2e-8 of the field at degree 9 and optical depth 90, 2e-3 at degree 19).  Every routine that
// relies on them switches contraction off for its own statements; the fused operations they want are written out as fma().
#ifdef __clang__
#define RTD_FP_EXACT _Pragma("clang fp contract(off)")
#else
#define RTD_FP_EXACT
#endif

struct rtd_dd {
  double hi, lo;
};
RTD_HD rtd_dd rtd_two_sum(const double a, const double b) {
  RTD_FP_EXACT
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
RTD_HD rtd_dd rtd_two_prod(const double a, const double b) {
  RTD_FP_EXACT
  const double p = a * b;
  return {p, fma(a, b, -p)};
}
RTD_HD rtd_dd rtd_dd_add(const rtd_dd x, const rtd_dd y) {
  RTD_FP_EXACT
  rtd_dd s = rtd_two_sum(x.hi, y.hi);
  s.lo += x.lo + y.lo;
  return rtd_two_sum(s.hi, s.lo);
}
RTD_HD rtd_dd rtd_dd_mul_d(const rtd_dd x, const double t) {  // x * t
  RTD_FP_EXACT
  rtd_dd p = rtd_two_prod(x.hi, t);
  p.lo = fma(x.lo, t, p.lo);
  return rtd_two_sum(p.hi, p.lo);
}
RTD_HD rtd_dd rtd_dd_div_d(const rtd_dd x, const double t) {  // x / t
  RTD_FP_EXACT
  const double q = x.hi / t;
  const rtd_dd p = rtd_two_prod(q, t);
  const double r = ((x.hi - p.hi) - p.lo + x.lo) / t;
  return rtd_two_sum(q, r);
}
// coefficients c[0..n) of p(x) = sum_j c_j x^j  ->  coefficients of the same polynomial in (x - t), in place, in double-double for
// any n (the reference puts no limit on Nscoeffs).  Up to 16 coefficients -- every practical source polynomial -- the Horner /
// Ruffini scheme, n (n - 1) / 2 multiply-adds on 16 double-doubles of a thread's stack.  Beyond, the triangle has no place there:
// b_k = sum_{j >= k} C(j, k) c_j t^(j - k) is one double-double Horner pass per output coefficient, O(1) storage, the binomials
// carried along in double-double (integers: exact while they fit 106 bits, 32 digits beyond); b_k reads c_k ... c_(n-1) only, so
// ascending k overwrites nothing that is still to be read.
RTD_HD void rtd_taylor_shift(double* c, const int n, const double t) {
  RTD_FP_EXACT
  if (n > 16) {
    for (int k = 0; k < n; ++k) {
      rtd_dd bin = {1.0, 0.0};  // C(j, k), j = k ... n - 1
      for (int j = k; j < n - 1; ++j) bin = rtd_dd_div_d(rtd_dd_mul_d(bin, (double)(j + 1)), (double)(j + 1 - k));
      rtd_dd acc = {0.0, 0.0};
      for (int j = n - 1; j >= k; --j) {
        acc = rtd_dd_add(rtd_dd_mul_d(acc, t), rtd_dd_mul_d(bin, c[j]));
        if (j > k) bin = rtd_dd_div_d(rtd_dd_mul_d(bin, (double)(j - k)), (double)j);  // C(j - 1, k)
      }
      c[k] = acc.hi + acc.lo;
    }
    return;
  }
  rtd_dd w[16];
  for (int j = 0; j < n; ++j) w[j] = {c[j], 0.0};
  for (int k = 0; k < n - 1; ++k)
    for (int j = n - 2; j >= k; --j) w[j] = rtd_dd_add(w[j], rtd_dd_mul_d(w[j + 1], t));
  for (int j = 0; j < n; ++j) c[j] = w[j].hi + w[j].lo;
}
// The same shift from a[0..n) into another array b[0..n).
RTD_HD void rtd_taylor_shift_to(const double* a, double* b, const int n, const double t) {
  for (int j = 0; j < n; ++j) b[j] = a[j];
  rtd_taylor_shift(b, n, t);
}
// The thermal source of one layer as the kernels want it: s(tau) = sum_j a_j tau^j in the ABSOLUTE, unscaled optical depth (the
// user's s_poly_coeffs) -> coefficients about the layer's top in the delta-M-scaled depth x = sc (tau - top), times the factor
// (1 - omega) / sc of the scaled source (pydisort.py:326-329, :338).  b = Taylor shift of a by `top` (double-double), coefficient i
// divided by sc^i.  One routine for the device preparation (rtd_prep.hip) and the host's (rtd_source_polynomials_local): the
// float64 coefficients in the absolute scaled depth, which the reference forms first, cannot hold a deep polynomial of degree >= 5.
RTD_HD void rtd_source_local(const double* a, double* o, const int Ns, const double top, const double sc, const double om) {
  rtd_taylor_shift_to(a, o, Ns, top);
  const double rsc = 1.0 / sc;
  double sci = 1.0;  // sc^-i
  for (int i = 0; i < Ns; ++i) {
    o[i] *= sci;
    sci *= rsc;
  }
  const double k = (1.0 - om) * rsc;
  for (int i = 0; i < Ns; ++i) o[i] *= k;
}
