// rtd_lambert.hip -- Lambertian albedo sweeps from one solve: the results of a plan solved over a black surface coupled with those of
// its companion, the same layers without a source lit from below by unit isotropic intensity, for many albedos at once
// (rtd_api.hip: rtd_plan_couple_lambert, rtd_plan_couple_lambert_band).  The arithmetic and its rounding bound are rtd_lambert.h,
// shared with the host.
//
//   rtd_lambert_kappa_kernel   kappa [C][A] and flag [C].  One thread per column, the albedos in ascending order in that thread: the
//                              flag of a column is written by one thread, no atomics.  flag bits: 1 some albedo of the column has
//                              1 - A s <= 0 or a non-finite factor; 2 Fourier mode 0 of the column failed in either plan; 4 a mode
//                              m > 0 of the primary failed (u and its view alone).
//   rtd_lambert_couple_kernel  out [C][A][E] = X [C][E] + kappa [C][A] Y [C][E / nrep].  One thread per output element, e -- for u
//                              the (tau, phi) axis -- fastest across the lanes: a wavefront reads and writes runs of consecutive
//                              doubles.  nrep: azimuths per point when X is u (the companion is azimuth-independent, its u0 stands
//                              for every phi), else 1.  A column whose flag meets `mask` is NaN.  One fma per output, written by one
//                              thread: no atomics, no cross-lane step, so the bits depend on neither the launch geometry nor the
//                              chunk or window size.
// Both kernels are bound by their memory traffic; neither uses LDS or scratch.
#include "rtd_device.h"
#include "rtd_lambert.h"

namespace {

__global__ void __launch_bounds__(256) rtd_lambert_kappa_kernel(const double* albedo, long group, int nalb, const double* fdown,
                                                                const double* sph, const double* emission, const int* st_a,
                                                                const int* st_b, long C, double* kappa, int* flag) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double* A = albedo + (c / group) * nalb;
  const double F = fdown[c], s = sph[c], E = emission ? emission[c] : 0.0;
  const int sa = st_a ? st_a[c] : 0, sb = st_b ? st_b[c] : 0;  // (the plan-free form has no plans: no status)
  int f = (((sa | sb) & 0xFF) ? 2 : 0) | ((sa & 0xFF00) ? 4 : 0);
  for (int a = 0; a < nalb; ++a) {
    int bad;
    kappa[c * nalb + a] = rtd_lambert_kappa(A[a], F, s, E, &bad);
    f |= bad;
  }
  flag[c] = f;
}

__global__ void __launch_bounds__(256) rtd_lambert_couple_kernel(const double* X, const double* Y, const double* kappa, const int* flag,
                                                                 int mask, long C, int nalb, long E, int nrep, double* out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= C * nalb * E) return;
  const long e = idx % E, ca = idx / E, c = ca / nalb;
  const double v = rtd_lambert_couple(X[c * E + e], Y[c * (E / nrep) + e / nrep], kappa[ca]);
  out[idx] = (flag[c] & mask) ? __builtin_nan("") : v;
}

}  // namespace

void rtd_launch_lambert_kappa(const double* albedo, long group, int nalb, const double* fdown, const double* sph, const double* emission,
                              const int* st_a, const int* st_b, long C, double* kappa, int* flag, hipStream_t s) {
  hipLaunchKernelGGL(rtd_lambert_kappa_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, albedo, group, nalb, fdown, sph, emission,
                     st_a, st_b, C, kappa, flag);
}

void rtd_launch_lambert_couple(const double* X, const double* Y, const double* kappa, const int* flag, int mask, long C, int nalb, long E,
                               int nrep, double* out, hipStream_t s) {
  const long total = C * nalb * E;
  hipLaunchKernelGGL(rtd_lambert_couple_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, X, Y, kappa, flag, mask, C, nalb, E,
                     nrep, out);
}
