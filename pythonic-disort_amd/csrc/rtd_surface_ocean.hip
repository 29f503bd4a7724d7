// rtd_surface_ocean.hip -- BDRF Fourier modes of the wind-roughened ocean (RTD_SURFACE_OCEAN; csrc/rtd_surface.h has the
// reflectance and defines the clustered azimuth rule), written straight into the plan's tables bdrfq [C][NBDRF][NP][NP] and
// bdrfq0 [C][NBDRF][NP].  No samples in memory: the glint's azimuthal width at a grazing pair of 34 or 64 streams is 1e-3 rad, the
// uniform grid of rtd_surface_samples_kernel + rtd_bdrf_modes_kernel would need more than 16384 samples per pair there.
//
// A TEAM of RTD_OCEAN_LANES lanes (a wavefront holds 64 / RTD_OCEAN_LANES teams) takes one pair of cosines -- (c, i, j): mu_i, mu_j,
// or (c, i): mu_i and the column's raw mu0.  With b = rtd_ocean_cluster_b of the pair, a = 1 - b, psi_p = 2 pi p / nphi and rho even
// in dphi, the lane handles the samples p = lane, lane + LANES, ... <= nphi / 2:
//      dphi_p = b psi_p + a (psi_p - sin psi_p),   w_p = e_p (b + 2 a sin^2(psi_p / 2)),  e_p = 1/2 at p = 0 and p = nphi / 2, else 1,
//      v_p = w_p rho(mu, mu', cos dphi_p, sin dphi_p)                                      (rtd_surface_rho: the bits of every other caller)
//      acc[m] += v_p cos(m dphi_p)   for all modes of the pass at once,
// then the team sums acc[m] across its lanes (xor butterfly) and lane 0 writes q^m = (2 - delta_m0) (2 / nphi) acc[m].
// The nodes are not equispaced, so no cosine table applies; cos(m dphi_p) is formed per sample in BLOCKS OF 8 MODES: the block's
// first two factors are computed directly, T_m0 = cos(m0 dphi) and T_m0+1 = T_m0 cos dphi - sin(m0 dphi) sin dphi from one sincos
// (m0 = 0: 1 and cos dphi exactly), the other six by T_k+1 = fma(2 cos dphi, T_k, -T_k-1).
//
// Rounding of the factors, from the loop as written (u = 2^-53, c = cos dphi as computed, |c - cos dphi| <= u after libm's < 1 ulp):
// the error e_k of T_m0+k obeys e_k+1 = 2 c e_k - e_k-1 + r_k with r_k = (one rounding of the fma, <= u) + (2 u T_k: c is off by u),
// |r_k| <= 3 u, and the homogeneous solutions are the Chebyshev U polynomials, |U_n| <= n + 1:
//      |e_k| <= k |e_1| + (k - 1) |e_0| + 3 u Sum_{j=1}^{k-1} (k - j)  =  k |e_1| + (k - 1) |e_0| + 3 u k (k - 1) / 2 .
// Seeds: the product m0 dphi is rounded (<= u m0 pi), sincos is good to 1 ulp: |e_0| <= (m0 pi + 1) u; T_m0+1 is two products and a
// difference of numbers <= 1 on top: |e_1| <= (m0 pi + 1) u (|c| + |s|) + 2 u (1 + ...) <= (1.5 m0 pi + 5) u.  At k = 7:
//      |e_7| <= 7 (1.5 m0 pi + 5) u + 6 (m0 pi + 1) u + 63 u  <=  (52 m0 + 104) u,
// 3.7e-13 at m0 = 56 and 1.2e-14 at m0 = 0; without the restart the c-term alone grows like m^2 u and sits at dphi -> 0, where the
// glint is.  The dominant part, u m0 pi, is the rounding of the angle m0 dphi itself and is shared by a direct evaluation of every
// factor, which would cost a cosine per mode and sample where this costs one sincos per eight.  A mode's error from its factors is
// therefore <= (52 m + 104) u (2 - delta_m0) (2 / nphi) Sum_p |v_p|, to which the summation adds (nphi / 2 + 8) u of the same sum.
// rho >= 0, so that sum is q^0 itself.  tools/surface_ocean_truth.py states the whole bound next to the 50-digit modes.
//
// Team width, measured (profiles/surface_ocean.json, "team_width": 10^5 benchmark columns of 32 streams, nphi = 512, the whole call
// in seconds at NBDRF = 8 / 32): 64 lanes 0.547 / 0.692, 16 lanes 0.505 / 0.596, 4 lanes 0.497 / 0.580 beside 0.47 with a one-mode
// Lambert table.  257 samples leave a wide team's last round nearly empty (1 lane of 64 busy in the fifth round) and the butterfly
// costs a step per doubling and mode; 4 lanes waste 3 lanes of one round in 65.  148 / 160 / 220 / 332 VGPRs for MB = 8 / 16 / 32 /
// 64, nothing spilled (tools/kernel_resources.py).
//
// LDS: none.  Barriers: none.  Cross-lane: the butterfly at the end.  NBDRF <= 64 is one pass with every accumulator in registers
// (the template's MB = 8, 16, 32 or 64); beyond that, passes of 64 modes.
#include "rtd_device.h"
#include "rtd_surface.h"

#ifndef RTD_OCEAN_LANES
#define RTD_OCEAN_LANES 4
#endif

namespace {

struct RtdOceanDev {
  int nphi, group, with_q0, mbase;  // group: columns per parameter row; mbase: first mode of this pass
  long par_rows;
  const double* par;                // [par_rows][4]: U, n, rho_w, 0
  const double* mu0;                // [C] raw (null without a beam)
};

// LANES = 1 is the form the stand-in runtime of tests/cpu runs thread by thread: the same samples, one lane's order of summation
template <int LANES, int MB>
__global__ __launch_bounds__(64) void rtd_surface_ocean_kernel(RtdDev d, RtdOceanDev v) {
  const int lane = (int)threadIdx.x % LANES, team = (int)threadIdx.x / LANES;
  const long N = d.N, NP = d.NP, NB = d.NBDRF;
  const long nqq = (long)d.C * N * N, nvec = nqq + (v.with_q0 ? (long)d.C * N : 0);
  long vec = (long)blockIdx.x * (64 / LANES) + team;
  if (vec >= nvec) return;  // (the whole team leaves together)
  long col, mstride;
  double mu, mup;
  double* out;
  if (vec < nqq) {
    col = vec / (N * N);
    const long i = (vec / N) % N, j = vec % N;
    mu = d.mu[i]; mup = d.mu[j];
    out = const_cast<double*>(d.bdrfq) + (col * NB * NP + i) * NP + j;
    mstride = NP * NP;
  } else {
    vec -= nqq;
    col = vec / N;
    const long i = vec % N;
    mu = d.mu[i]; mup = v.mu0[col];
    out = const_cast<double*>(d.bdrfq0) + col * NB * NP + i;
    mstride = NP;
  }
  const double* par = v.par + 4 * (v.par_rows == 1 ? 0 : col / v.group);
  const double pi = 3.141592653589793238462643383279502884;
  const double b = rtd_ocean_cluster_b(par[0], mu, mup), a = 1.0 - b;
  const int half = v.nphi / 2;
  double acc[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) acc[m] = 0.0;
  for (int p = lane; p <= half; p += LANES) {
    double cpsi, spsi, ch, sh;
    const double x = 2.0 * (double)p / (double)v.nphi;
    rtd_surface_cs(x, &cpsi, &spsi);
    rtd_surface_cs((double)p / (double)v.nphi, &ch, &sh);
    const double psi = pi * x;
    const double dphi = b * psi + a * (psi - spsi);
    const double w = (p == 0 || p == half ? 0.5 : 1.0) * (b + 2.0 * a * sh * sh);
    const double c = cos(dphi), s = sin(dphi);
    const double val = w * rtd_surface_rho(RTD_SURFACE_OCEAN, par, mu, mup, c, s);
    const double c2 = 2.0 * c;
#pragma unroll
    for (int m0 = 0; m0 < MB; m0 += 8) {
      double t0, t1;
      if (m0 == 0 && v.mbase == 0) {
        t0 = 1.0; t1 = c;
      } else {
        const double ang = (double)(v.mbase + m0) * dphi;
        const double s0 = sin(ang);
        t0 = cos(ang);
        t1 = t0 * c - s0 * s;
      }
      acc[m0] += val * t0;
      acc[m0 + 1] += val * t1;
#pragma unroll
      for (int k = 2; k < 8; ++k) {
        const double t2 = fma(c2, t1, -t0);
        acc[m0 + k] += val * t2;
        t0 = t1; t1 = t2;
      }
    }
  }
  const double scale = 2.0 / (double)v.nphi;
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    double t = acc[m];
#if defined(__HIPCC__)
#pragma unroll
    for (int o = LANES / 2; o >= 1; o >>= 1) t += __shfl_xor(t, o, LANES);
#endif
    const long mode = v.mbase + m;
    if (lane == 0 && mode < NB) out[mode * mstride] = t * (mode == 0 ? scale : 2.0 * scale);
  }
}

template <int LANES, int MB>
void launch(const RtdDev& d, const RtdOceanDev& v, long nvec, hipStream_t s) {
  const int teams = 64 / LANES;
  hipLaunchKernelGGL((rtd_surface_ocean_kernel<LANES, MB>), dim3((unsigned)((nvec + teams - 1) / teams)), dim3(64), 0, s, d, v);
}

}  // namespace

// par: the device copy of the request's rows [par_rows][4]; mu0_raw: the staged raw mu0 [C] (read only when the plan has a beam);
// group: columns per parameter row.  The tables' padding is the caller's (zeroed beforehand); every real entry is written here.
void rtd_launch_surface_ocean(const RtdDev& d, int nphi, const double* par, long par_rows, int group, const double* mu0_raw, hipStream_t s) {
#if defined(__HIPCC__)
  constexpr int LANES = RTD_OCEAN_LANES;
#else
  constexpr int LANES = 1;  // (the stand-in runtime has no cross-lane operation)
#endif
  static_assert(LANES == 1 || LANES == 2 || LANES == 4 || LANES == 8 || LANES == 16 || LANES == 32 || LANES == 64, "a team is a power of two of lanes");
  RtdOceanDev v{};
  v.nphi = nphi; v.group = group; v.with_q0 = d.beam ? 1 : 0; v.par_rows = par_rows; v.par = par; v.mu0 = d.beam ? mu0_raw : nullptr;
  const long nvec = (long)d.C * d.N * (d.N + (d.beam ? 1 : 0));
  if (nvec <= 0) return;
  for (int mbase = 0; mbase < d.NBDRF; mbase += 64) {
    v.mbase = mbase;
    const int left = d.NBDRF - mbase;
    if (left <= 8) launch<LANES, 8>(d, v, nvec, s);
    else if (left <= 16) launch<LANES, 16>(d, v, nvec, s);
    else if (left <= 32) launch<LANES, 32>(d, v, nvec, s);
    else launch<LANES, 64>(d, v, nvec, s);
  }
}
