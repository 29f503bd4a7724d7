// rtd_bc_rows.hip -- the row-per-lane boundary-condition kernels: the last resort of the 64-stream kernel (rtd_bc_tile2.hip).
//
// The recursion of rtd_bc.hip's header with partial pivoting in every elimination, for the (column, mode) chains that
// rtd_bc_tile2_kernel could not solve (a singular carry block) and flagged in d.need_split; nothing else runs here.  Two kernels:
// rtd_iface_kernel (all (column, mode, interface) in parallel: Wp, Wq, rho through HBM) and rtd_sweep_kernel (per (column, mode):
// forward carry recursion, bottom boundary, backward sweep).  32 lanes per chain, two chains per wavefront, lane i owns row i of
// the carry system.  A wavefront none of whose chains is flagged leaves at once: an ordinary launch costs two empty grids.
// The interface points of a window in which a chain was handed over come from the evaluation kernel (d.split_any,
// rtd_launch_eval).  (The pair used to be a stage of its own at other stream counts: HISTORY.md.)
#include <cstdlib>
#include <type_traits>

#include "rtd_device.h"

namespace {

#include "rtd_bc_common.h"

constexpr int NP = 32, Q = 64, GPW = 2, LD = NP + 1;  // lanes per chain, streams, chains per wavefront, LDS row stride
using W = Ws<NP>;

// ------------------------------------------------------------------------------------------------
// Interface kernel: per (c, m, l < L-1):  Wp, Wq, rho_t, rho_b.  `only` is d.need_split: the chains handed over by the tiled
// kernel (the others keep what that kernel stored); it is never null.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rtd_iface_kernel(RtdDev d, const int* only) {
  __shared__ double sA[GPW][NP * LD];  // A_l  (natural [i][j])
  __shared__ double sY[GPW][NP * LD];  // Y_l
  const int grp = threadIdx.x / NP, j = threadIdx.x % NP;
  const int Lm1 = d.L - 1;
  const long nprob = (long)d.C * d.M * Lm1;
  long pid = (long)blockIdx.x * GPW + grp;
  bool valid = pid < nprob;
  if (!valid) pid = nprob - 1;
  valid = valid && only[pid / Lm1] != 0;
  const unsigned long long want = __ballot(valid);
  if (want == 0) return;
  // groups with nothing to do redo the work of one that has (well-defined data, no stores)
  const int src = __ffsll((long long)want) - 1;
  const int pid_w = __shfl((int)pid, src, 64);
  if (!valid) pid = pid_w;
  const int l = (int)(pid % Lm1);
  const long cm = pid / Lm1;
  const int m = (int)(cm % d.M), c = (int)(cm / d.M);
  const long p0 = cm * d.L + l, p1 = p0 + 1;
  double* A0 = sA[grp];
  double* Y0 = sY[grp];
  {
    const double* Am = d.Am + p0 * NP * NP;
    const double* Ym = d.Ym + p0 * NP * NP;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      A0[i * LD + j] = Am[i * NP + j];
      Y0[i * LD + j] = Ym[i * NP + j];
    }
  }
  // V^-1 V' = A^T Y'   and   U^-1 U' = diag(k) Y^T A' diag(1/k')   (T cancels)
  const double rk1 = 1.0 / d.kk[p1 * NP + j];
  double* ws = d.Fws + (cm * Lm1 + l) * W::SLOT;
  {
    // column j of Y' and A' of layer l+1
    double ycol[NP], acol[NP];
    {
      const double* Ym = d.Ym + p1 * NP * NP;
      const double* Am = d.Am + p1 * NP * NP;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        ycol[i] = Ym[i * NP + j];
        acol[i] = Am[i * NP + j];
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < NP; ++r) {
      double vv = 0.0, uu = 0.0;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        vv += A0[i * LD + r] * ycol[i];
        uu += Y0[i * LD + r] * acol[i];
      }
      uu *= d.kk[p0 * NP + r] * rk1;
      if (valid) {
        ws[W::WP + r * NP + j] = 0.5 * (vv + uu);
        ws[W::WQ + r * NP + j] = 0.5 * (vv - uu);
      }
    }
  }
  // particular-solution jump r_l at the interface (:184-205, :242-245) and rho = G_l^-1 r_l:
  //   rho_t/b = 1/4 [ V^-1 (r_up + r_dn) +- U^-1 (r_up - r_dn) ],  V^-1[j][i] = T_i A[i][j],  U^-1[j][i] = -k_j T_i Y[i][j]
  const double* ts0 = d.taus0 + (long)c * (d.L + 1);
  const double tb = ts0[l + 1];
  const double att = d.beam ? exp(-tb / d.mu0[c]) : 0.0;
  const int mg = d.m0 + d.mstep * m;  // the Fourier mode this local index stands for (mode shards)
  const bool iso = d.Ns > 0 && mg == 0;
  const double kj = d.kk[p0 * NP + j];
  double rt = 0.0, rb = 0.0;
#pragma unroll 4
  for (int i = 0; i < NP; ++i) {
    double ru = 0.0, rd = 0.0;
    if (d.beam) {
      ru = (d.Bv[p1 * Q + i] - d.Bv[p0 * Q + i]) * att;
      rd = (d.Bv[p1 * Q + NP + i] - d.Bv[p0 * Q + NP + i]) * att;
    }
    if (iso) {  // v_{l+1} at its top minus v_l at its bottom: the eigen kernel's boundary values (vb), no polynomial evaluated here
      const double* vb0 = d.vb + ((long)c * d.L + l) * 4 * NP;
      ru += vb0[4 * NP + i] - vb0[2 * NP + i];
      rd += vb0[5 * NP + i] - vb0[3 * NP + i];
    }
    const double Ti = d.T[i];
    const double a = Ti * A0[i * LD + j] * (ru + rd), b = -kj * Ti * Y0[i * LD + j] * (ru - rd);
    rt += a + b;
    rb += a - b;
  }
  if (valid) {
    ws[W::RT + j] = 0.25 * rt;
    ws[W::RB + j] = 0.25 * rb;
  }
}

// ------------------------------------------------------------------------------------------------
// Sweep kernel: per (c, m): forward carry recursion over the layers, bottom BC, backward sweep.  `only` as above.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64, 1) void rtd_sweep_kernel(RtdDev d, const int* only) {
  __shared__ double sA[GPW][NP * LD];  // Wq (forward) / S (bottom)
  __shared__ double sB[GPW][NP * LD];  // Wp
  __shared__ double sV[GPW][4][NP];
  const int grp = threadIdx.x / NP, j = threadIdx.x % NP;
  const long nprob = (long)d.C * d.M;
  long cm = (long)blockIdx.x * GPW + grp;
  bool valid = cm < nprob;
  if (!valid) cm = nprob - 1;
  valid = valid && only[cm] != 0;
  const unsigned long long want = __ballot(valid);
  if (want == 0) return;
  // groups with nothing to do redo the work of one that has (well-defined data -- their own interface operators were
  // not formed -- and no stores)
  const int src = __ffsll((long long)want) - 1;
  const int cm_w = __shfl((int)cm, src, 64);
  if (!valid) cm = cm_w;
  const int m = (int)(cm % d.M), c = (int)(cm / d.M);
  const int L = d.L, Lm1 = L - 1;
  double* A_ = sA[grp];
  double* B_ = sB[grp];
  double* v0 = sV[grp][0];
  double* v1 = sV[grp][1];
  double* v2 = sV[grp][2];
  double* v3 = sV[grp][3];
  const double* Ym = d.Ym + cm * L * NP * NP;
  const double* Am = d.Am + cm * L * NP * NP;
  const double* kk = d.kk + cm * L * NP;
  const double rTj = 1.0 / d.T[j];  // row scaling of G: Gp = (Y - A/k)/T, Gm = (Y + A/k)/T
  const double* Ek = d.Ek + cm * L * NP;
  const double* Bv = d.Bv + cm * L * Q;
  const double* ts0 = d.taus0 + (long)c * (L + 1);
  const double* dq = d.dq + (long)c * L * d.Ns * Q;
  double* wsb = d.Fws + cm * Lm1 * W::SLOT;
  double* coef = d.coef + cm * L * Q;
  const int mg = d.m0 + d.mstep * m;  // the Fourier mode this local index stands for (mode shards)
  const bool iso = d.Ns > 0 && mg == 0;
  const bool beam = d.beam != 0;
  const double mu0 = beam ? d.mu0[c] : 1.0;
  // thermal particular solution of layer l at one of the layer's own boundaries (top / bottom), streams idx in [0, 2 NP): the values
  // the eigen kernel left in vb (it holds the polynomial coefficients about the layer's top, rtd_dd.h) -- no polynomial is evaluated here
  const double* vbp = d.vb + (long)c * L * 4 * NP;
  auto vedge = [&](int l, bool bottom, int idx) { return vbp[((long)l * 4 + (bottom ? 2 : 0)) * NP + idx]; };

  // carry rows, one per lane: Ta C- + Tb C+ = t.  Top boundary (down-streams at tau = 0) (:161-179, :284-285)
  double ta[NP], tb[NP], tt;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const double yv = Ym[j * NP + k], av = Am[j * NP + k] / kk[k];
    ta[k] = (yv + av) * rTj;          // Gm_0
    tb[k] = (yv - av) * rTj * Ek[k];  // Gp_0 E_0
  }
  tt = d.bneg[cm * NP + j];
  if (beam) tt -= Bv[NP + j];
  if (iso) tt -= dq[NP + j];

  int pc = -1;
  for (int l = 0; l < L; ++l) {
    pc = -1;
    GjStep<NP, NP, 0>::run(ta, tb, tt, pc, grp);  // lane now holds row pc of S = Ta^-1 Tb and s[pc]
    // a chain that has gone NaN (failed eigen stage of its mode) finds no pivots: its lanes keep their own row index, so
    // that what they write below stays inside their group's LDS and workspace (the other chain of the wavefront is
    // another mode or another column); the NaN coefficients raise RTD_ST_BC for this chain's mode at the end
    if (pc < 0) pc = j;
    if (l == Lm1) break;
    double* ws = wsb + (long)l * W::SLOT;
    __syncthreads();
    {  // stage Wq, Wp of this interface in LDS (coalesced rows); store S row and s for the backward sweep
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        A_[i * LD + j] = ws[W::WQ + i * NP + j];
        B_[i * LD + j] = ws[W::WP + i * NP + j];
      }
      v0[j] = ws[W::RB + j];
      v1[j] = Ek[(l + 1) * NP + j];
      if (valid) {
#pragma unroll
        for (int k = 0; k < NP; ++k) ws[W::S + pc * NP + k] = tb[k];
        ws[W::SV + pc] = tt;
      }
    }
    __syncthreads();
    const double Er = Ek[l * NP + pc];
    double srb = 0.0;
#pragma unroll
    for (int k = 0; k < NP; ++k) srb += tb[k] * v0[k];  // (S rho_b)[pc]
    const double tnew = ws[W::RT + pc] - Er * (tt - srb);
    double nbuf[NP];
#pragma unroll
    for (int cc = 0; cc < NP; ++cc) {
      double swq = 0.0, swp = 0.0;
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        swq += tb[k] * A_[k * LD + cc];
        swp += tb[k] * B_[k * LD + cc];
      }
      ta[cc] = -(Er * swq + B_[pc * LD + cc]);           // Ta' = -(E S Wq + Wp)
      nbuf[cc] = -(Er * swp + A_[pc * LD + cc]) * v1[cc];  // Tb' = -(E S Wp + Wq) E'  (tb is still an input)
      RTD_FENCE();
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) tb[k] = nbuf[k];
    tt = tnew;
  }

  // ---- bottom boundary (up-streams at tau_L) (:208-232, :248-254, :288-293):  Ba C- + Bb C+ = br,
  //      with C- = s - S C+  ->  (Bb - Ba S) C+ = br - Ba s.
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NP; ++k) A_[pc * LD + k] = tb[k];  // S at its true row index
  v0[pc] = tt;                                            // s
  __syncthreads();
  {
    const int l = Lm1;
    const double* ymL = Ym + (long)l * NP * NP;
    const double* amL = Am + (long)l * NP * NP;
    const double* kl = kk + (long)l * NP;
    const double att = beam ? exp(-ts0[L] / mu0) : 0.0;
    // Ba = Gp - R Gm, Bb = Gm - R Gp  built from  P = (I - R) Y / T-rows and  Qd = (I + R) A / (k T-rows):
    //   Gp = P0 - Q0, Gm = P0 + Q0 with P0 = Y/T, Q0 = A/(kT)  =>  Ba = (P0 - R P0) - (Q0 + R Q0), Bb = (P0 - R P0) + (Q0 + R Q0)
    double pa[NP], qa[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      pa[k] = ymL[j * NP + k] * rTj;
      qa[k] = amL[j * NP + k] * rTj;
    }
    double br = d.bpos[cm * NP + j];
    if (mg < d.NBDRF) {
      const double delta = (mg == 0) ? 2.0 : 1.0;
      const double* qt = d.bdrfq + (((long)c * d.NBDRF + mg) * NP + j) * NP;
      double rbm = 0.0, rvm = 0.0;
      for (int j2 = 0; j2 < NP; ++j2) {
        const double Rij = delta * qt[j2] * d.mu[j2] * d.w[j2] / d.T[j2];  // R = (1 + delta_m0) q (mu w), times 1/T_j2
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          pa[k] -= Rij * ymL[j2 * NP + k];
          qa[k] += Rij * amL[j2 * NP + k];
        }
        const double Rraw = Rij * d.T[j2];
        if (beam) rbm += Rraw * Bv[l * Q + NP + j2];
        if (iso) rvm += Rraw * vedge(l, true, NP + j2);
      }
      if (beam) {
        const double Xs = mu0 * d.I0[c] / M_PI * d.bdrfq0[((long)c * d.NBDRF + mg) * NP + j];
        br += (Xs + rbm - Bv[l * Q + j]) * att;
      }
      if (iso) br += rvm - vedge(l, true, j);
    } else {
      if (beam) br -= Bv[l * Q + j] * att;
      if (iso) br -= vedge(l, true, j);
    }
    double ba[NP], bb[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const double qk = qa[k] / kl[k];
      ba[k] = pa[k] - qk;
      bb[k] = pa[k] + qk;
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) ba[k] *= Ek[l * NP + k];
    // am = Bb - Ba S,  bvec = br - Ba s
    double am[NP], dummy[1] = {0.0};
#pragma unroll
    for (int cc = 0; cc < NP; ++cc) {
      double a = bb[cc];
#pragma unroll
      for (int k = 0; k < NP; ++k) a -= ba[k] * A_[k * LD + cc];
      am[cc] = a;
      RTD_FENCE();
    }
    double bvec = br;
#pragma unroll
    for (int k = 0; k < NP; ++k) bvec -= ba[k] * v0[k];
    int pc2 = -1;
    GjStep<NP, 1, 0>::run(am, dummy, bvec, pc2, grp);  // lane holds C+[pc2]
    if (pc2 < 0) pc2 = j;  // (NaN chain, as above)
    v1[pc2] = bvec;
    __syncthreads();
    double cmin = tt;  // C-[pc] = s[pc] - S[pc][:] C+
#pragma unroll
    for (int k = 0; k < NP; ++k) cmin -= tb[k] * v1[k];
    v2[pc] = cmin;
    __syncthreads();
    if (valid) {
      coef[(long)l * Q + j] = v2[j];
      coef[(long)l * Q + NP + j] = v1[j];
      // singular system (the reference's solve_banded / solve raises LinAlgError, :326-333, :383)
      if (!(fabs(v2[j]) + fabs(v1[j]) < 1e300)) rtd_raise(d, RTD_ST_BC, mg, c);
    }
  }
  // ---- backward sweep: C+_l = Wq C-' + Wp E' C+' + rho_b ;  C-_l = s - S C+_l
  for (int l = Lm1 - 1; l >= 0; --l) {
    const double* ws = wsb + (long)l * W::SLOT;
    double cp = ws[W::RB + j];
#pragma unroll 4
    for (int k = 0; k < NP; ++k)
      cp += ws[W::WQ + j * NP + k] * v2[k] + ws[W::WP + j * NP + k] * (Ek[(l + 1) * NP + k] * v1[k]);
    v3[j] = cp;
    __syncthreads();
    double cmin = ws[W::SV + j];
#pragma unroll 4
    for (int k = 0; k < NP; ++k) cmin -= ws[W::S + j * NP + k] * v3[k];
    __syncthreads();
    v1[j] = cp;
    v2[j] = cmin;
    if (valid) {
      coef[(long)l * Q + j] = cmin;
      coef[(long)l * Q + NP + j] = cp;
    }
    __syncthreads();
  }
}

}  // namespace

// the interface operators of every flagged chain (all interfaces in parallel), then carry recursion / bottom BC / backward sweep
void rtd_launch_bc_rows(const RtdDev& d, hipStream_t s) {
  const long nch = (long)d.C * d.M, nif = nch * (d.L - 1);
  if (nif > 0) hipLaunchKernelGGL(rtd_iface_kernel, dim3((unsigned)((nif + 1) / 2)), dim3(64), 0, s, d, (const int*)d.need_split);
  hipLaunchKernelGGL(rtd_sweep_kernel, dim3((unsigned)((nch + 1) / 2)), dim3(64), 0, s, d, (const int*)d.need_split);
}
