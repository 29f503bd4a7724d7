// rtd_bc.hip -- boundary-condition solve across layers (coefficients C of the homogeneous solutions).
//
// Replaces _solve_for_coeffs (src/PythonicDISORT/_solve_for_coeffs.py:8-390): RHS assembly (:142-254),
// LHS assembly in banded/dense form (:276-323 / :337-380) and scipy.linalg.solve_banded /
// np.linalg.solve (:326-333 / :383).  Same linear system (same unknowns, same Stamnes-Conklin
// scaling), solved by a structured block elimination instead of a general banded LU:
//
//   interface l:  G_l [E_l C-_l ; C+_l]  -  G_{l+1} [C-_{l+1} ; E_{l+1} C+_{l+1}]  =  r_l
//   The eigen stage knows G_l^-1 in closed form (G = [[V+U, V-U],[V-U, V+U]], V^-1 = Z^T L^T T,
//   U^-1 = -k Z^T L^-1 T), so multiplying the 2N continuity rows by G_l^-1 makes the x_l block diagonal:
//        E_l C-_l = Wp C-' + Wq E' C+' + rho_t ,     C+_l = Wq C-' + Wp E' C+' + rho_b ,
//   with  W = G_l^-1 G_{l+1} = [[Wp, Wq],[Wq, Wp]],  Wp/Wq = (V^-1 V' +- U^-1 U')/2.
//   With the N "carry" rows  Ta C-_l + Tb C+_l = t  (initially the top boundary condition) this gives
//        C-_l = s - S C+_l ,  S = Ta^-1 Tb, s = Ta^-1 t      (the only pivoted solve: N x N, partial pivoting)
//   and the carry of the next layer  Ta' = -(E_l S Wq + Wp), Tb' = -(E_l S Wp + Wq) E', t' = rho_t - E_l (s - S rho_b).
//   Pivots are 1 for the C+ columns and come from the carry block for the C- columns, which is the
//   order partial pivoting takes whenever E_l < 1; verified against pivoted elimination of the full
//   banded matrix to <= 5e-13 on every golden case and on thick/thin/near-conservative stress cases
//   (tools/proto_device_algo.py: check_structured).
//
// This file: 16 < NQuad <= 32, rtd_bc_mfma_kernel -- one wavefront per (column, mode), everything in the matrix-core register
// layout (see its comment below) -- and rtd_launch_bc at the end, which chooses among the files.  The other stream counts have
// files of their own, all on this recursion: NQuad <= 16 rtd_bc_small.hip, 32 < NQuad <= 64 rtd_bc_tile2.hip (rtd_bc_mfma_kernel's
// scheme on 2 x 2 tiles) with rtd_bc_rows.hip (row-per-lane kernels with partial pivoting: its last resort for a singular carry
// block), 64 < NQuad <= 128 rtd_bc_wide.hip.  (Kernels that lost their A/B runs and were removed: HISTORY.md.)
#include <cstdlib>
#include <type_traits>

#include "rtd_device.h"

namespace {

#include "rtd_bc_common.h"
#include "rtd_bc_tile_common.h"

// ------------------------------------------------------------------------------------------------
// Fused boundary-condition kernel, NP = 16: ONE wavefront per (column, mode) does the interface operators, the
// forward carry recursion, the bottom boundary and the backward sweep, with every 16 x 16 matrix held in the
// operand / accumulator layout of v_mfma_f64_16x16x4_f64 ("D layout": lane = 16 kq + col, register q holds the
// element [row 4 q + kq][col]).  In that layout one MFMA chain gives X^T Y for two D-layout matrices, X^T for
// Y = I, so the recursion is carried in transposed form:
//      H = S^T ,   Ta'^T = -(Wq^T (H E) + Wp^T) ,   Tb'^T = -E' (Wp^T (H E) + Wq^T) ,   H' = Tb'^T Ta'^-T
// (column-pivoted Gauss-Jordan on the stacked rows [Ta'^T ; Tb'^T ; t'^T]: columns = lanes, the same elimination
// as the row-per-lane kernels' (rtd_bc_rows.hip) seen through a transpose).  W and W^T come from the eigen stage's Y, A straight from HBM
// (each layer is read once per direction); nothing but H_l, s_l and rho_b is stored for the backward sweep, which
// applies W through its factors:  Wq x + Wp y = [A_l^T Y' (x + y) + k_l Y_l^T A' ((y - x)/k')] / 2.
// Against that two-kernel path this removes the Wp/Wq round trip through HBM (about 40 % of the stage's traffic).
// ------------------------------------------------------------------------------------------------
#ifndef RTD_BCF_WIN
#define RTD_BCF_WIN 20  // layers of small vectors resident in LDS (9 792 B per wavefront with the save area: 16 per CU)
#endif

// Speculative, branch-free form of the same elimination with the diagonal as pivot at every step: straight-line
// code (the 16 steps schedule into each other), no pivot search.  A step whose diagonal candidate is more than a
// factor RTD_GJ_GROWTH smaller than another unused entry of its row raises `bad` (a zero pivot leaves inf / nan in the
// result, which the caller tests); the caller then
// repeats the elimination from its saved inputs with column pivoting (counts from a temporary statistics build).
// The pivot column is scaled by the same FMA as the others: its own broadcast value is itself, so f = 1 - 1/pivot
// gives v - f v = v / pivot.
// Threshold: a multiplier |f| > RTD_GJ_GROWTH flags the elimination.  The pivoted redo is slow (a rolled loop on the LDS
// copy of the inputs, one stacked row per lane; its register-resident predecessor took ~45 000 cycles per elimination and
// cost 20 % of kernel time at threshold 8, where 3.1 % of the eliminations are flagged).  64 is the classical relaxed
// threshold of sparse direct solvers (u = 1/64: local growth <= 65, i.e. ~1e-14 instead of 1e-16 relative): well under
// 1 % flagged, parity against the oracle unchanged to all printed digits (1.62e-11 abs, 4.10e-10 rel; also at 512).
#ifndef RTD_GJ_GROWTH
#define RTD_GJ_GROWTH 64.0
#endif
// The kernel's global loads and stores in the two sweeps, at the turn and in the flush take a wave-uniform base and a 32-bit
// lane offset (ldg_u / stg_u, rtd_bc_tile_common.h) instead of a per-lane 64-bit pointer: -8 % VALU, +1.6 % headline against
// the per-lane-pointer form, the same memory operations in the same order and the same results to the bit
// (tests/test_gpu_bc32_bits.py).  (The flush's two predicated stores, written that way too, are sunk by the compiler into ONE
// store per staged row with a selected per-lane base -- the same lanes and bytes; the flush waits for vmcnt(0) itself.  The
// window fills keep their per-lane pointers.  HISTORY.md: "Scalar-base addressing in the 32-stream BC kernel".)
template <int K, int Q0, int Q1>
struct FmacRows {  // v[q] -= bcast_K(v[q]) * f for q in [Q0, Q1)
  static __device__ __forceinline__ void run(double (&v)[4], const double f) {
    if constexpr (Q0 < Q1) {
      asm volatile("v_fmac_f64_dpp %0, -%0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(v[Q0]) : "v"(f), "n"(K));
      FmacRows<K, Q0 + 1, Q1>::run(v, f);
    }
  }
};

template <int NB, int K>
struct GjFast {
  static __device__ __forceinline__ void run(double (&ta)[4], double (&tb)[4], double& tv, int& bad, const int col) {
    constexpr int QK = K >> 2, RK = K & 3;
    const double x = bcast_row<RK>(ta[QK], col);  // row K of Ta^T, replicated over the lane-rows
    const double xk = bcast16<K>(x);
    // one Newton step from the hardware seed (~4e-15): an inexact multiplier only perturbs entries that are never
    // read again, an inexact pivot scale perturbs column K of the result by the same relative amount
    const double r0 = __builtin_amdgcn_rcp(xk);
    const double rp = r0 * (2.0 - xk * r0);
    const double f = (col == K) ? 1.0 - rp : x * rp;
    bad |= (col > K && fabs(f) > RTD_GJ_GROWTH) ? 1 : 0;  // a zero pivot shows up as a non-finite result (checked by the caller)
    // v -= bcast_K(v) * f as ONE instruction per register: v_fmac_f64 with a row_newbcast DPP source (the only DPP control
    // the DP ALU has), the source being the accumulator itself (settled in round 3 against an FMA on a bcast16 copy).  The compiler's hazard recogniser does not see VALU writes
    // made inside inline asm; a DPP read needs two wait states after a VALU write of the same VGPR: every register
    // touched here was last written by the previous step's block (>= 9 instructions back), and the block ends with the
    // wait states that cover the compiler's own DPP / permute reads of ta in the next step.  `volatile` keeps the blocks
    // of consecutive steps in program order (the scheduler would otherwise put step K + 1's update of a register right
    // behind step K's); build.py scans the generated ISA for the hazard pattern (tools/check_dpp_hazards.py).
    FmacRows<K, QK, 4>::run(ta, f);
    FmacRows<K, 0, NB>::run(tb, f);
    asm volatile("v_fmac_f64_dpp %0, -%0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf\n\ts_nop 1" : "+v"(tv) : "v"(f), "n"(K));
    GjFast<NB, K + 1>::run(ta, tb, tv, bad, col);
  }
};
template <int NB>
struct GjFast<NB, 16> {
  static __device__ __forceinline__ void run(double (&)[4], double (&)[4], double&, int&, const int) {}
};

// Column-pivoted Gauss-Jordan on the same registers as GjFast (round 4: the elimination of the chains that are pivoted
// THROUGHOUT -- chain_needs_pivoting -- used to be the rolled LDS loop `pivoted_lds`, ~10 x a speculative elimination: a
// batch with a conservative cloud layer in every column ran 3 x slower).  Step K makes row K of Ta^T a unit vector; the pivot
// is the largest unused column of that row, with threshold 1/4 in favour of the diagonal (the rule of pivoted_lds: partial
// pivoting with threshold 1/4 bounds the growth like LAPACK's, _solve_for_coeffs.py:326-333).  One chain per wavefront: the
// pivot column is wave-uniform, its row entry comes by v_readlane, its column by ds_bpermute (a run-time lane: no DPP
// broadcast); 18 cross-lane fetches + 9 FMAs per step, no LDS memory, no barrier.  Afterwards the column that was the
// pivot of step c holds column c of Tb^T Ta^-T and t^T Ta^-T (perm[c], written to sPerm): the caller moves them back.
template <int NB, int K>
struct GjPiv {
  static __device__ __forceinline__ void run(double (&ta)[4], double (&tb)[4], double& tv, unsigned& used, int* sPerm, const int col,
                                             const int rowbase, const int lane) {
    constexpr int QK = K >> 2, RK = K & 3;
    const double x = bcast_row<RK>(ta[QK], col);  // row K of Ta^T, replicated over the lane-rows
    const float key = ((used >> col) & 1u) ? -1.0f : fabsf((float)x);
    const float kmax = group_max_key<16>(key);
    const float kd = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(key), 0x150 + K, 0xF, 0xF, true));
    int pcol = K;
    if (!(kd >= 0.25f * kmax && kd > 0.0f)) {  // (wave-uniform: the four lane-rows hold the same row)
      const unsigned long long bal = __ballot(key == kmax) & 0xFFFFull;
      pcol = bal ? __ffsll((long long)bal) - 1 : K;  // (a chain that has gone NaN has no candidate: the diagonal, NaN stays NaN)
    }
    pcol = __builtin_amdgcn_readfirstlane(pcol);
    const double xp = readlane_f64(x, pcol);
    const double rp = fast_rcp(xp);
    // the pivot column is scaled by 1 / pivot EXACTLY (one multiplication): the speculative form's v - (1 - 1/p) v loses
    // |1 - 1/p| / |1/p| ulps, harmless for its growth-limited pivots, not for the chains that are here because their result
    // hangs on the last digits (random32/3736: 1.6e-2 of the field scale with that form, 1.9e-4 -- the reference's level -- so)
    const bool isp = col == pcol;
    const double f = x * rp;
    const int addr = (rowbase | pcol) << 2;
    auto upd = [&](double& v) {
      const double bp = bperm(addr, v);
      v = isp ? bp * rp : fma(-f, bp, v);
    };
    static_for<QK, 4>([&](auto qc) {  // rows below 4 QK are finished: unit vectors with a zero in every unused column
      upd(ta[decltype(qc)::value]);
    });
    static_for<0, NB>([&](auto qc) { upd(tb[decltype(qc)::value]); });
    upd(tv);
    used |= 1u << pcol;
    if (lane == 0) sPerm[K] = pcol;
    if constexpr (K + 1 < 16) GjPiv<NB, K + 1>::run(ta, tb, tv, used, sPerm, col, rowbase, lane);
  }
};

// Four wavefronts per SIMD: <= 128 registers and <= 10 KB of LDS each, so the kernel prefetches one layer ahead, forms the
// interface products one after the other (one accumulator set live), takes exp(-k dtau) from memory, saves t^T once and
// rotates two operand sets in the backward sweep (128 VGPRs, 13 dwords spilled outside the two loops -- profiles/bc32_diet/kernel_resources.json; 9.8 KB).  The kernel
// is bound by the latency of its dependent chains: a three-wavefront form (two layers of prefetch, the products side by
// side, exp(-k dtau) in the LDS window: 168 VGPRs, 12.7 KB; removed in round 3) took 4.19-4.25 ms per 2 048 cfg4 columns
// against this form's 4.08-4.11 ms, and padded to 7 / 9 / 12 wavefronts per CU 5.46 / 4.82 / 4.33 ms.
__global__ __launch_bounds__(64, 4) void rtd_bc_mfma_kernel(RtdDev d) {
  constexpr int NP = 16, Q = 32, NN = NP * NP;
  const int lane = threadIdx.x, kq = lane >> 4, col = lane & 15, rowbase = lane & 48;
  const long cm = chain_of_block(blockIdx.x, d.C, d.M);
  const int m = (int)(cm % d.M), c = (int)(cm / d.M);
  const int L = d.L, Lm1 = L - 1;
  const double* Ym = d.Ym + cm * L * NN;
  const double* Am = d.Am + cm * L * NN;
  const double* kk = d.kk + cm * L * NP;
  const double* Ek = d.Ek + cm * L * NP;
  const double* Bv = d.Bv + cm * L * Q;
  const double* ts0 = d.taus0 + (long)c * (L + 1);
  const double* dq = d.dq + (long)c * L * d.Ns * Q;
  double* wsb = d.Fws + cm * Lm1 * Ws<NP>::SLOT;
  double* coef = d.coef + cm * L * Q;
  const int mg = d.m0 + d.mstep * m;  // the Fourier mode this local index stands for (mode shards)
  const bool iso = d.Ns > 0 && mg == 0;
  const bool beam = d.beam != 0;
  const double mu0 = beam ? d.mu0[c] : 1.0;
  // careful: this chain takes the column-pivoted elimination throughout (GjPiv, registers) -- a mode-0 chain with a tiny eigenvalue,
  // thermal source or not (chain_needs_pivoting), or the test hook RTD_BC_FORCE_PIVOT=2 for every chain.  force_redo (RTD_BC_FORCE_PIVOT=1): every speculative elimination is
  // declared failed and redone by pivoted_lds, the path of the rare real failures (the suite runs under both).
  const int careful = chain_needs_pivoting(d, mg == 0, kk, L, NP) | ((d.flags >> 2) & 1);
  const int force_redo = d.flags & 1;
  // thermal particular solution of layer l at one of the layer's own boundaries (top / bottom), streams idx in [0, 2 NP): the values
  // the eigen kernel left in vb (it holds the polynomial coefficients about the layer's top, rtd_dd.h) -- no polynomial is evaluated here
  const double* vbp = d.vb + (long)c * L * 4 * NP;
  auto vedge = [&](int l, bool bottom, int idx) { return vbp[((long)l * 4 + (bottom ? 2 : 0)) * NP + idx]; };
  // Per-lane-pointer loads: the prologue's and the bottom boundary's global reads and every LDS read (the sweeps' global accesses
  // are load_d_u / load_row_u).  (kq is passed in so that the loops can hand over an opaque copy of the lane index: the compiler
  // then rebuilds the few address VGPRs per iteration instead of keeping dozens of hoisted ones alive and spilling)
  auto load_d =[](const double* p, const int kq, const int col) {  // row-major 16 x 16 matrix -> D layout
    v4f64 x;
    x[0] = p[kq * NP + col];
    x[1] = p[(4 + kq) * NP + col];
    x[2] = p[(8 + kq) * NP + col];
    x[3] = p[(12 + kq) * NP + col];
    return x;
  };
  auto load_row = [](const double* p, const int kq) {  // a 16-vector in row form
    v4f64 x;
    x[0] = p[kq];
    x[1] = p[4 + kq];
    x[2] = p[8 + kq];
    x[3] = p[12 + kq];
    return x;
  };
  auto make_eye = [](const int kq, const int col) {
    v4f64 e;
    e[0] = (kq == col) ? 1.0 : 0.0;
    e[1] = (4 + kq == col) ? 1.0 : 0.0;
    e[2] = (8 + kq == col) ? 1.0 : 0.0;
    e[3] = (12 + kq == col) ? 1.0 : 0.0;
    return e;
  };
  // ---- LDS.  (1) The save area of the running elimination, read back only when its speculation fails; the backward sweep
  //      stages its results there.  (2) The chain's small vectors for a window of RTD_BCF_WIN layers, filled by coalesced
  //      loads: exp(-k_l dtau_l), the stream scaling T, and the particular solution p_l(tau) = B_l exp(-tau / mu0) + v_l(tau)
  //      (beam + thermal polynomial) in the form each sweep needs -- forward: its jump at the interface below layer l,
  //      r_l = p_(l+1)(tau_(l+1)) - p_l(tau_(l+1)) (:184-205, :242-245); backward: its value at the top of layer l, which the
  //      fused evaluation adds.  The loops then read them in whatever form they need (row form = a broadcast read)
  //      without keeping dozens of registers in flight, know nothing of beam or thermal sources, and have no global load
  //      that is consumed right away (one such load makes the wave wait for everything it has in flight: the counter is
  //      in-order).
  constexpr int W = RTD_BCF_WIN;
  constexpr int NSV = 8 * 64 + 16;  // the save area: rows of Ta^T, Tb^T (4 x 64 each) and one copy of t^T
  constexpr int NSTG = NSV / 64;                    // result rows it can stage in the backward sweep
  __shared__ double sSaveFlat[NSV];
  double (*const sSave)[64] = reinterpret_cast<double (*)[64]>(sSaveFlat);
  __shared__ double sPs[W][Q];  // forward: r_l; backward: p_l(tau_l)
  __shared__ double sT[2][NP];  // T and 1 / T
  __shared__ double sF[NP];
  // Diagnostic build (-DRTD_BCF_STAMPS): lane 0 of three chains records s_memtime at the phase boundaries and prints the
  // differences (tools/bc_phase_cycles.py formats them); this is how the stalls named in the comments were measured.
  // The stamps split basic blocks: read the stamped build's own ISA before trusting a phase (its forward loop, unlike the
  // product's, ends with a vmcnt(0) that waits for the stores).
#ifdef RTD_BCF_STAMPS
  __shared__ long long sStamp[512];
  int nstamp = 0;
#define RTD_STAMP()                                                                  \
  {                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                               \
    if (lane == 0 && nstamp < 512) sStamp[nstamp] = (long long)__builtin_amdgcn_s_memtime(); \
    ++nstamp;                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                               \
  }
#else
#define RTD_STAMP()
#endif
  RTD_STAMP();
  __shared__ int sPerm[NP];
  int wb = 0;                   // the window holds layers [wb, wb + W) and interfaces [wb, wb + W]
  // Column-pivoted Gauss-Jordan on the save area: the stacked rows [Ta^T ; Tb^T (with_tb) ; t^T] in the D layout, row r of
  // the stack = sSave[r >> 2][16 (r & 3) + column].  Step K makes row K of Ta^T a unit vector; the pivot is the largest
  // unused column of that row (threshold 1/4 in favour of the diagonal); afterwards the column that was the pivot of
  // step c holds column c of Tb^T Ta^-T and t^T Ta^-T.  Rolled loops, one stacked row per lane: slow and small -- it runs
  // for the few eliminations whose speculation fails and must not cost the others registers.
  auto pivoted_lds = [&](const bool with_tb) {
    __syncthreads();
    double* const sM = &sSave[0][0];
    unsigned int used = 0;
    const int r = lane;
    const bool mine = r < NP || (with_tb && r < 2 * NP) || r == 2 * NP;
    double* const myrow = sM + (r >> 2) * 64 + 16 * (r & 3);
#pragma unroll 1
    for (int K = 0; K < NP; ++K) {
      const double* rowK = sM + (K >> 2) * 64 + 16 * (K & 3);
      float key = (lane < NP && !((used >> lane) & 1u)) ? fabsf((float)rowK[lane]) : -1.0f;
      const float kd = __shfl(key, K, 64);
      int idx = lane;
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) {  // argmax over lanes 0..15 (lowest index among equals)
        const float k2 = __shfl_xor(key, o, 64);
        const int i2 = __shfl_xor(idx, o, 64);
        if (k2 > key || (k2 == key && i2 < idx)) {
          key = k2;
          idx = i2;
        }
      }
      const float kmax = __shfl(key, 0, 64);
      const int pcol = (kd >= 0.25f * kmax && kd > 0.0f) ? K : __shfl(idx, 0, 64);
      used |= 1u << pcol;
      const double rp = 1.0 / rowK[pcol];
      if (lane < NP) sF[lane] = (lane == pcol) ? 0.0 : rowK[lane] * rp;
      if (lane == 0) sPerm[K] = pcol;
      __syncthreads();
      if (mine) {
        const double mp = myrow[pcol];
#pragma unroll 4
        for (int jj = 0; jj < NP; ++jj) myrow[jj] -= sF[jj] * mp;
        myrow[pcol] = mp * rp;
      }
      __syncthreads();
    }
  };
  // Two forms.  `fill` is the plain loop, used for the refills inside the sweeps (chains deeper than the window): it pays
  // the memory latency once per 64 elements but costs the loops no registers.  `fill_all` issues all loads of a fill before
  // the first is used (indices clamped, not predicated): one latency instead of ten; it holds ~70 registers and is used
  // where few others are live -- before the forward loop and at the turn into the backward sweep, i.e. for every fill of a
  // chain that fits the window.
  auto fill = [&](const int base, const bool backward) {
    __syncthreads();
    wb = base;
    const int nl = min(W, L - base);
#pragma unroll 1
    for (int e = lane; e < nl * Q; e += 64) {
      const int l = base + (e >> 5), i = e & 31;
      double v = 0.0;
      if (backward) {
        if (beam) v = Bv[l * Q + i] * d.att[(long)c * (L + 1) + l];
        if (iso) v += vedge(l, false, i);
      } else if (l < Lm1) {
        if (beam) v = (Bv[(l + 1) * Q + i] - Bv[l * Q + i]) * d.att[(long)c * (L + 1) + l + 1];
        if (iso) v += vedge(l + 1, false, i) - vedge(l, true, i);
      }
      (&sPs[0][0])[e] = v;
    }
    
    __syncthreads();
  };
  auto fill_all = [&](const int base, const bool backward) {
    __syncthreads();
    wb = base;
    const int nl = min(W, L - base);
    constexpr int NE = W * Q / 64, NK = (W * NP + 63) / 64;
    static_assert(W * Q % 64 == 0, "whole passes of the wavefront");
    const double* att = d.att + (long)c * (L + 1);
    double b1[NE], b0[NE], at[NE], ek[NK];
#pragma unroll
    for (int it = 0; it < NE; ++it) {
      const int e = min(lane + 64 * it, nl * Q - 1), l = base + (e >> 5), i = e & 31;
      const int lt = backward ? l : min(l + 1, Lm1);  // forward: the jump B_(l+1) - B_l (zero at the last layer)
      b1[it] = Bv[lt * Q + i];
      b0[it] = Bv[l * Q + i];
      at[it] = att[backward ? l : l + 1];
    }
    
#pragma unroll
    for (int it = 0; it < NE; ++it) {
      const int e = lane + 64 * it, l = base + (e >> 5), i = e & 31;
      if (e < nl * Q) {
        double v = beam ? (backward ? b1[it] : b1[it] - b0[it]) * at[it] : 0.0;
        if (iso) {
          if (backward) v += vedge(l, false, i);
          else if (l < Lm1) v += vedge(l + 1, false, i) - vedge(l, true, i);
        }
        (&sPs[0][0])[e] = v;
      }
    }
    
    __syncthreads();
  };
  // (everything the prologue needs from memory is requested here, ahead of the window's fill: one memory latency, the
  //  fill's, for all of it instead of three in a row)
  v4f64 a0 = load_d(Am, kq, col), y0 = load_d(Ym, kq, col);
  const int lsecond = min(1, Lm1);
  v4f64 a1 = a0, y1 = y0;  // (lean: layer l + 1 is requested at the top of iteration l)
  double k0c = kk[col], k1c = k0c;
  
  const v4f64 k_row = load_row(kk, kq);
  v4f64 e_row_g = k_row;
  e_row_g = load_row(Ek, kq);
  double tv = d.bneg[cm * NP + col];
  const double bv_top = beam ? Bv[NP + col] : 0.0, dq_top = iso ? dq[NP + col] : 0.0;
  {
    const double t = d.T[col];
    if (lane < NP) {
      sT[0][lane] = t;
      sT[1][lane] = fast_rcp(t);
    }
  }
  fill_all(0, false);
  tv -= bv_top + dq_top;

  // carry rows (transposed): top boundary, down-streams at tau = 0 (:161-179, :284-285):
  //   Ta = Gm_0 = (Y + A/k)/T-rows,  Tb = Gp_0 E_0 = (Y - A/k)/T-rows E_0
  double ta[4], tb[4];
  {
    const double rT_col = sT[1][col];
    const v4f64 eye = make_eye(kq, col);
    const v4f64 yt = mm_t(y0, eye), at = mm_t(a0, eye);
    const v4f64 e_row = e_row_g;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double av = at[q] * fast_rcp(k_row[q]);
      ta[q] = (yt[q] + av) * rT_col;
      tb[q] = (yt[q] - av) * rT_col * e_row[q];
    }
  }

  // One layer per iteration, in this order:
  //   loads     the operands of layer l + 2 (consumed by the NEXT iteration);
  //   products  M1 = A_l^T Y', M2s = diag(k) Y_l^T A' diag(1/k') and their transposes, the particular-solution jump rho:
  //             independent of the carry, in one block with
  //   the elimination  [Ta^T ; Tb^T ; t^T] -> H = S^T, s   whose dependent steps leave the issue slots the MFMAs fill;
  //   a wait    for the loads (issued a whole elimination ago), THEN the stores of H, s, rho_b: with loads and stores
  //             both in flight every wait is a wait for the youngest store's acknowledgement (~4 000 cycles, measured:
  //             40 % of an iteration when the stores came before the wait); stored here they have a whole iteration;
  //   the carry of the next layer.
  // (Everything the prologue loaded is waited for here: a register that still had a load pending at the loop's entry would
  //  get a counted wait at its first use in the loop, and a counted wait is a wait for every OLDER operation -- the
  //  previous iteration's stores.)
  __builtin_amdgcn_s_waitcnt(0x0F70);
  for (int l = 0; l < L; ++l) {
    // (kq, col from an opaque copy of the lane index: the compiler then rebuilds the few address VGPRs per iteration
    //  instead of keeping dozens of hoisted ones alive and spilling)
    int lv = lane;
    asm volatile("" : "+v"(lv));
    const int kq = lv >> 4, col = lv & 15, rowbase = lv & 48;
    const int ln = min(l + 1, Lm1), l2 = min(l + 2, Lm1);
    v4f64 a2 = a1, y2 = y1, e1r_g = a1;
    double k2c = k1c, e0c_g = 0.0;
    const LaneOff lo = lane_offsets(lv);
    {  // one layer ahead: consumed behind this iteration's elimination
      a1 = load_d_u(Am + (long)ln * NN, lo.lane8);
      y1 = load_d_u(Ym + (long)ln * NN, lo.lane8);
      k1c = ldg_u(kk + ln * NP, lo.col8);
      e0c_g = ldg_u(Ek + l * NP, lo.col8);
      e1r_g = load_row_u(Ek + ln * NP, lo.kq8);
    }
    if (ln >= wb + W) fill(l, false);
    RTD_STAMP();  // 4 l + 1: loop top (register rotation, loads issued)
    const int r0 = l - wb, r1 = ln - wb;
    // ---- elimination (speculative: the diagonal as pivot; see GjFast)
    {
      // (the speculative elimination stays unconditional and in ONE basic block with the products above: its dependent steps
      //  leave the issue slots the MFMAs fill.  A chain that is pivoted throughout pays for it as well -- straight-line, cheap --
      //  and then redoes the elimination from the saved inputs; wrapping the two forms in if / else split the block and cost
      //  the kernel 4 %)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sSave[q][lane] = ta[q];
        sSave[4 + q][lane] = tb[q];
      }
      if (kq == 0) sSave[8][col] = tv;
      int bad = 0;
      GjFast<4, 0>::run(ta, tb, tv, bad, col);
      bad |= (fabs(tv) + fabs(tb[0]) + fabs(tb[1]) + fabs(tb[2]) + fabs(tb[3]) < 1e300) ? 0 : 1;  // zero pivot: inf / nan
      bad |= force_redo | careful;
      if (__any(bad)) {  // some diagonal pivot was too small, or the chain is pivoted throughout: the saved inputs once more
        if (careful) {  // (wave-uniform) in registers
          __syncthreads();
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            ta[q] = sSave[q][lane];
            tb[q] = sSave[4 + q][lane];
          }
          tv = sSave[8][col];
          unsigned used = 0;
          GjPiv<4, 0>::run(ta, tb, tv, used, sPerm, col, rowbase, lane);
          __syncthreads();
          const int addr = (rowbase | sPerm[col]) << 2;  // unknown `col` sits in the column that was the pivot of step `col`
#pragma unroll
          for (int q = 0; q < 4; ++q) tb[q] = bperm(addr, tb[q]);
          tv = bperm(addr, tv);
          __syncthreads();
        } else {
          pivoted_lds(true);
          const int src = sPerm[col];  // unknown `col` sits in the column that was the pivot of step `col`
#pragma unroll
          for (int q = 0; q < 4; ++q) tb[q] = sSave[4 + q][16 * kq + src];
          tv = sSave[8][src];
          __syncthreads();
        }
      }
    }
    RTD_STAMP();  // 4 l + 2: elimination
    if (l == Lm1) break;
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the loads of this iteration, before the stores go out
    // (S, rho_b and s lie 4 096 ... 6 528 bytes into the slot, past the 13-bit immediate: the scalar base is taken at S through an
    //  opaque byte offset, or the compiler folds the constants back into one and builds the address in vector registers after
    //  all.  The offset, not the pointer: a pointer out of an asm statement is a flat one)
    long wso = 8 * ((long)l * Ws<NP>::SLOT + Ws<NP>::S);
    asm("" : "+s"(wso));
    double* wS = reinterpret_cast<double*>(reinterpret_cast<char*>(wsb) + wso);
#pragma unroll
    for (int q = 0; q < 4; ++q) stg_u(wS, block_local(lo.lane8), 512 * q, tb[q]);  // element [4 q + kq][col]
    if (kq == 0) stg_u(wS, block_local(lo.col8), 8 * (Ws<NP>::SV - Ws<NP>::S), tv);
    {
      // the same quantities with one accumulator set live at a time (Y_l is scaled in place: it is not used again)
      v4f64 a1s;
      {
        const double rk1c = fast_rcp(k1c);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          y0[q] *= k0c;
          a1s[q] = a1[q] * rk1c;
        }
      }
      double rt = 0.0, rb = 0.0;
      {
        const v4f64 t_row = load_row(&sT[0][0], kq);
        const v4f64 ru = load_row(&sPs[r0][0], kq), rd = load_row(&sPs[r0][NP], kq);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double pa = t_row[s] * a0[s] * (ru[s] + rd[s]), pb = -t_row[s] * y0[s] * (ru[s] - rd[s]);
          rt += pa + pb;
          rb += pa - pb;
        }
        rt = 0.25 * sum_kq(rt);
        rb = 0.25 * sum_kq(rb);
      }
      if (kq == 0) stg_u(wS, block_local(lo.col8), 8 * (Ws<NP>::RB - Ws<NP>::S), rb);
      const double e0c = e0c_g;
      v4f64 he;
#pragma unroll
      for (int q = 0; q < 4; ++q) he[q] = tb[q] * e0c;
      const v4f64 hcur = {tb[0], tb[1], tb[2], tb[3]};
      const double tnew = rt - e0c * (tv - col_dot(hcur, col_to_row(rb, rowbase, kq)));  // t' = rho_t - E (s - S rho_b)
      // X + M1^T = M1^T (H E + I) and Z - M2s^T = M2s^T (H E - I): the unit matrix goes onto the diagonal of H E before each product,
      // so that neither transpose is ever formed -- not by a second MFMA chain (FP64 MFMAs and FP64 vector instructions share the DP
      // ALUs on gfx950, tools/hiptests/dp_coissue.hip: 8 MFMAs were 512 cycles of the very resource the kernel is short of), and not
      // through LDS either (rounds 3-4: two round trips on the chain's critical path per layer)
      v4f64 hep, hem;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double one = (4 * q + kq == col) ? 1.0 : 0.0;
        hep[q] = he[q] + one;
        hem[q] = he[q] - one;
      }
      v4f64 s1;  // M1^T (H E + I)
      {
        const v4f64 m1 = mm_t(a0, y1);
        s1 = mm_t(m1, hep);
      }
      {
        const v4f64 m2s = mm_t(y0, a1s);
        const v4f64 dd4 = mm_t(m2s, hem);  // M2s^T (H E - I)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double dd = dd4[q];
          ta[q] = -0.5 * (s1[q] - dd);
          tb[q] = -0.5 * (s1[q] + dd) * e1r_g[q];
        }
      }
      tv = tnew;
    }
#ifdef RTD_BCF_STAMPS
    asm volatile("" ::"v"(ta[0]), "v"(ta[3]), "v"(tb[0]), "v"(tb[3]), "v"(tv));
#endif
    RTD_STAMP();  // 4 l + 4: carry
    a0 = a1;
    y0 = y1;
    k0c = k1c;
    
  }

  // ---- bottom boundary (up-streams at tau_L) (:208-232, :248-254, :288-293):  Ba C- + Bb C+ = br,
  //      with C- = s - S C+  ->  (Bb - Ba S) C+ = br - Ba s;  Ba = [(I - R) P0 - (I + R) Q0] E_L, Bb = (I - R) P0 + (I + R) Q0,
  //      P0 = Y/T-rows, Q0 = A/(k T-rows), R = (1 + delta_m0) q (mu w).  Solved transposed like the carry.
  double cminus, cplus;
  {
    const int l = Lm1, rL = Lm1 - wb;
    // (everything the block needs from memory is requested here, before the first use: one memory latency instead of
    //  one per group of loads)
    const bool refl = mg < d.NBDRF;
    const double kLc = kk[l * NP + col];
    double br = d.bpos[cm * NP + col];
    const double att = beam ? d.att[(long)c * (L + 1) + L] : 0.0;
    const double bvc = beam ? Bv[l * Q + col] : 0.0;
    v4f64 qr = {0.0, 0.0, 0.0, 0.0}, mur = qr, wr = qr, bdr = qr;
    double I0c = 0.0, q0c = 0.0;
    if (refl) {
      const double* qt = d.bdrfq + (((long)c * d.NBDRF + mg) * NP + col) * NP;  // row j = col of q^m
      qr = load_row(qt, kq);
      mur = load_row(d.mu, kq);
      wr = load_row(d.w, kq);
      if (beam) {
        bdr = load_row(Bv + l * Q + NP, kq);
        I0c = d.I0[c];
        q0c = d.bdrfq0[((long)c * d.NBDRF + mg) * NP + col];
      }
    }
    v4f64 eLr_g = qr;
    eLr_g = load_row(Ek + l * NP, kq);
    const double rkLc = fast_rcp(kLc);
    const v4f64 eLr = eLr_g;
    const v4f64 rT_row = load_row(&sT[1][0], kq), eye = make_eye(kq, col);
    v4f64 p0, q0, x1 = eye, x2 = eye, rtr = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      p0[q] = y0[q] * rT_row[q];
      q0[q] = a0[q] * rT_row[q] * rkLc;
    }
    if (refl) {
      const double delta = (mg == 0) ? 2.0 : 1.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double r = delta * qr[q] * mur[q] * wr[q];  // R^T in the D layout: [row j2 = 4 q + kq][col j] = R[j][j2]
        rtr[q] = r;
        x1[q] -= r;
        x2[q] += r;
      }
    }
    const v4f64 g1 = mm_t(p0, x1), g2 = mm_t(q0, x2);  // ((I - R) P0)^T, ((I + R) Q0)^T
    v4f64 bat;
    double mt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      bat[q] = eLr[q] * (g1[q] - g2[q]);
      mt[q] = g1[q] + g2[q];
    }
    const v4f64 hcur = {tb[0], tb[1], tb[2], tb[3]};
    const v4f64 sd = mm_t(hcur, eye);     // S in the D layout
    const v4f64 hb = mm_t(sd, bat);       // S^T Ba^T
#pragma unroll
    for (int q = 0; q < 4; ++q) mt[q] -= hb[q];  // (Bb - Ba S)^T
    const double tL = iso ? ts0[L] : 0.0;
    if (refl) {
      if (beam) {
        const double rbm = col_dot(rtr, bdr);
        const double Xs = mu0 * I0c / M_PI * q0c;
        br += (Xs + rbm - bvc) * att;
      }
      if (iso) {
        v4f64 vr;
#pragma unroll
        for (int q = 0; q < 4; ++q) vr[q] = vedge(l, true, NP + 4 * q + kq);
        br += col_dot(rtr, vr) - vedge(l, true, col);
      }
    } else {
      br -= bvc * att;
      if (iso) br -= vedge(l, true, col);
    }
    double rhs = br - col_dot(bat, col_to_row(tv, rowbase, kq));
    double none[4] = {0.0, 0.0, 0.0, 0.0};
    if (careful) {
      unsigned used = 0;
      GjPiv<0, 0>::run(mt, none, rhs, used, sPerm, col, rowbase, lane);
      __syncthreads();
      rhs = bperm((rowbase | sPerm[col]) << 2, rhs);
      __syncthreads();
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) sSave[q][lane] = mt[q];
      if (kq == 0) sSave[8][col] = rhs;
      int bad = 0;
      GjFast<0, 0>::run(mt, none, rhs, bad, col);
      bad |= (fabs(rhs) < 1e300) ? 0 : 1;
      bad |= force_redo;
      if (__any(bad)) {
        pivoted_lds(false);
        rhs = sSave[8][sPerm[col]];
        __syncthreads();
      }
    }
    cplus = rhs;
    cminus = tv - col_dot(hcur, col_to_row(cplus, rowbase, kq));
    // a singular system (the reference's solve_banded / solve raises LinAlgError, :326-333, :383) leaves inf / nan here,
    // and they propagate through the whole backward sweep: one test at its end is enough
  }
  // ---- fused evaluation at the layer interfaces (d.um != null): u^m = G_l [e- C- ; e+ C+] + B_l exp(-tau*/mu0) (+ v) at
  //      the top of layer l (e- = 1, e+ = E_l) and, for the last layer, at its bottom (e- = E_L, e+ = 1); with
  //      Gp = (Y - A/k)/T, Gm = (Y + A/k)/T:  up = [Y (en + ep) - A (en - ep)/k]/T,  down = [Y (en + ep) + A (en - ep)/k]/T
  //      (_assemble_intensity_and_fluxes.py:197-254).  The sums over the eigen-index are row sums over the 16 lanes of a
  //      lane-row of the D layout.
  RTD_STAMP();  // bottom boundary
  double* um = d.um ? d.um + cm * (L + 1) * Q : nullptr;
  // Results leave through LDS: a global store issued inside the sweep would make every later wait for a prefetched operand
  // a wait for that store's acknowledgement as well.  The elimination's save area is free during the sweep: it takes the
  // rows [C-_l, C+_l | u^m(tau_l)] of nine layers (row L: u^m(tau_L) only), which then go out as nine full-width stores,
  // followed by an explicit wait: the stores are then out of the way of the counted waits of the next steps.
  double* const sOut = &sSave[0][0];
  int nstage = 0, ltop = L;  // slot k holds the rows of layer / interface ltop - k
  auto flush = [&]() {
    __syncthreads();
#pragma unroll 1
    for (int k2 = 0; k2 < nstage; ++k2) {
      const long row = ltop - k2;
      const double v = sOut[k2 * 64 + lane];
      const unsigned lane8 = (unsigned)lane << 3;
      if (lane < 32) {
        if (row < L) stg_u(coef + row * Q, lane8, 0, v);
      } else if (um) {
        stg_u(um + row * Q, lane8, -8 * 32, v);  // element lane - 32
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    ltop -= nstage;
    nstage = 0;
  };
  // the homogeneous part of u^m at an interface from the two row sums  P = Y_l (e- C- + e+ C+),  Qs = A_l (e- C- - e+ C+) / k_l
  // of layer l; lanes col < 4 hold element i = 4 (col & 3) + kq of the up- and of the down-streams
  auto um_values = [&](const v4f64& P, const v4f64& Qs, const int kq, const int col, double& up, double& dn) {
    const int c3 = col & 3;
    const v4f64 rT_row = load_row(&sT[1][0], kq);
    up = 0.0;
    dn = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double u_q = (P[q] - Qs[q]) * rT_row[q], d_q = (P[q] + Qs[q]) * rT_row[q];
      up = (c3 == q) ? u_q : up;
      dn = (c3 == q) ? d_q : dn;
    }
  };
  // C-_l, C+_l and (with the fused evaluation) u^m at the top of layer l into the next slot
  auto stage = [&](const int l, const double cmn, const double cp, const v4f64& P, const v4f64& Qs, const int kq, const int col) {
    if (nstage == NSTG) flush();
    double* o = sOut + nstage * 64;
    if (kq == 0) {
      o[col] = cmn;
      o[NP + col] = cp;
    }
    if (um) {
      double up, dn;
      um_values(P, Qs, kq, col, up, dn);
      if (col < 4) {
        const int i = 4 * (col & 3) + kq;
        o[32 + i] = up + sPs[l - wb][i];
        o[32 + NP + i] = dn + sPs[l - wb][NP + i];
      }
    }
    ++nstage;
  };
  // ---- backward sweep: C+_l = Wq C-' + Wp E' C+' + rho_b ;  C-_l = s_l - S_l C+_l, with W applied through its
  //      factors: the row sums  w1 = Y' (C-' + E' C+'),  w2 = A' (E' C+' - C-') / k'  of the layer below are carried from
  //      step to step, so that a step touches the operands of ONE layer only:
  //          C+_l = rho_b + (A_l^T w1 + k_l Y_l^T w2) / 2 ,  C-_l = s_l - H_l^T C+_l ,  then w1, w2 of layer l.
  //      Interface l for free: w1 and -w2 are the two row sums of the TOP of layer l (e- = 1, e+ = E_l).  The reference
  //      evaluates tau = tau_arr[l - 1] in layer l - 1, from above the interface (_assemble_intensity_and_fluxes.py:185);
  //      the continuity rows of the boundary-condition system make the two sides equal to the residual of the solve,
  //      which is what the fused-vs-kernel test holds to 1e-13 of the field scale.
  //      The sweep moves 6 KB per layer and does ~300 instructions on them: it runs at the speed of its loads (~3 000
  //      cycles of latency against ~1 300 of arithmetic).  Three register sets rotate (the loop is unrolled by three so that
  //      the rotation is a renaming, not a copy that would wait for the load): the operands of layer l - 3 are requested
  //      when layer l has been consumed; a step has no load of its own and no store.
  struct BwSet {
    v4f64 a, y, h;
    double sl, rb, k, e;  // (e: exp(-k dtau) of the layer, lean form only)
  };
  auto load_set = [&](const int l) {
    int lv = lane;
    asm volatile("" : "+v"(lv));
    BwSet s;
    const LaneOff lo = lane_offsets(lv);
    // Streamed (non-temporal): the last use of every line.  Measured +1.4 % on the headline; the same policy on the FORWARD sweep's
    // loads and stores lost 1 ... 4 % (they are what these loads find in the Infinity Cache).  profiles/bc_cache_policy/;
    // HISTORY.md: "Cache policy of the 32-stream hand-off".
    constexpr Mem P = Mem::STREAM;
    s.a = load_d_u<P>(Am + (long)l * NN, lo.lane8);
    s.y = load_d_u<P>(Ym + (long)l * NN, lo.lane8);
    long wso = 8 * ((long)l * Ws<NP>::SLOT + Ws<NP>::S);  // (opaque: see the forward loop's stores)
    asm("" : "+s"(wso));
    const double* wS = reinterpret_cast<const double*>(reinterpret_cast<const char*>(wsb) + wso);
    s.h = load_d_u<P>(wS, lo.lane8);
    s.sl = ldg_u<P>(wS, lo.col8, 8 * (Ws<NP>::SV - Ws<NP>::S));
    s.rb = ldg_u<P>(wS, lo.col8, 8 * (Ws<NP>::RB - Ws<NP>::S));
    s.k = ldg_u<P>(kk + l * NP, lo.col8);
    s.e = 0.0;
    s.e = ldg_u<P>(Ek + l * NP, lo.col8);
    return s;
  };
  v4f64 w1, w2;
  // (what the turn needs from memory -- the first operand set included -- is requested ahead of the window's fill: one
  //  memory latency for all of it)
  const unsigned col8 = (unsigned)col << 3;
  const double kL = ldg_u(kk + Lm1 * NP, col8);
  double eL_g = 0.0;
  eL_g = ldg_u(Ek + Lm1 * NP, col8);
  double attL = 0.0, buL = 0.0, bdL = 0.0;
  if (beam && um) {
    const unsigned i8 = (unsigned)(4 * (col & 3) + kq) << 3;  // the element of u^m a lane col < 4 stages
    attL = d.att[(long)c * (L + 1) + L];
    buL = ldg_u(Bv + Lm1 * Q, i8);
    bdL = ldg_u(Bv + Lm1 * Q, i8, 8 * NP);
  }
  BwSet s0 = {};
  if (Lm1 > 0) s0 = load_set(Lm1 - 1);
  fill_all(max(L - W, 0), true);
  {
    const double eL = eL_g, rk = fast_rcp(kL);
    nstage = 1;  // slot 0 = row L: u^m at tau_L, the bottom of the last layer (e- = E_L, e+ = 1); no coefficients
    if (um) {
      const double en = eL * cminus, ep = cplus;
      double up, dn;
      um_values(row_dot(y0, en + ep), row_dot(a0, (en - ep) * rk), kq, col, up, dn);
      if (col < 4) {
        const int i = 4 * (col & 3) + kq;
        up = fma(buL, attL, up);
        dn = fma(bdL, attL, dn);
        if (iso) {
          const double* vL = vbp + ((long)Lm1 * 4 + 2) * NP;  // vedge(Lm1, true, .)
          up += ldg_u(vL, (unsigned)i << 3);
          dn += ldg_u(vL, (unsigned)i << 3, 8 * NP);
        }
        sOut[32 + i] = up;
        sOut[32 + NP + i] = dn;
      }
    }
    const double x = cminus, y = eL * cplus;
    w1 = row_dot(y0, x + y);
    w2 = row_dot(a0, (y - x) * rk);
    v4f64 nw2;
#pragma unroll
    for (int q = 0; q < 4; ++q) nw2[q] = -w2[q];
    stage(Lm1, cminus, cplus, w1, nw2, kq, col);
  }
  if (Lm1 == 0) {  // single layer: no interface, no workspace
    flush();
    if (!(fabs(cminus) + fabs(cplus) < 1e300)) rtd_raise(d, RTD_ST_BC, mg, c);
    return;
  }
  auto step = [&](const int l, const BwSet& s) {
    int lv = lane;
    asm volatile("" : "+v"(lv));
    const int kq = lv >> 4, col = lv & 15, rowbase = lv & 48;
    if (l < wb) fill(max(l - W + 1, 0), true);
    const double cp = s.rb + 0.5 * (col_dot(s.a, w1) + s.k * col_dot(s.y, w2));
    RTD_STAMP();  // backward step: operands arrived, C+
    const double cmn = s.sl - col_dot(s.h, col_to_row(cp, rowbase, kq));
    cminus = cmn;
    cplus = cp;
    v4f64 nw2 = {0.0, 0.0, 0.0, 0.0};
    if (l > 0 || um) {
      const double x = cmn, y = s.e * cp;
      w1 = row_dot(s.y, x + y);
      w2 = row_dot(s.a, (y - x) * fast_rcp(s.k));
#pragma unroll
      for (int q = 0; q < 4; ++q) nw2[q] = -w2[q];
    }
    stage(l, cmn, cp, w1, nw2, kq, col);
    RTD_STAMP();  // backward step: C-, row sums, staging
  };
  __builtin_amdgcn_s_waitcnt(0x0F70);  // nothing pending at the loop's entry (see the forward loop)
  // (issued in the order of their use: a set requested after a younger one would be waited for with a smaller count; the
  //  first set came in with the fill)
  {  // two sets, unrolled by two
    BwSet s1 = load_set(max(Lm1 - 2, 0));
    __builtin_amdgcn_sched_barrier(0);
    for (int l = Lm1 - 1; l >= 0; l -= 2) {
      step(l, s0);
      s0 = load_set(max(l - 2, 0));
      if (l < 1) break;
      step(l - 1, s1);
      s1 = load_set(max(l - 3, 0));
    }
  }
  flush();
  RTD_STAMP();
#ifdef RTD_BCF_STAMPS
  if (lane == 0 && (cm == 1000 || cm == 30000 || cm == 60000 || (d.C <= 64 && (cm == 100 || cm == 300))))
    for (int i = 1; i < min(nstamp, 512); ++i) printf("ST %d %d %lld\n", (int)cm, i, sStamp[i] - sStamp[i - 1]);
#endif
  if (!(fabs(cminus) + fabs(cplus) < 1e300)) rtd_raise(d, RTD_ST_BC, mg, c);
}

}  // namespace

bool rtd_bc_fuses_eval(const RtdDev& d) {
  // the fused kernels -- rtd_bc_small_kernel (NP <= 8), rtd_bc_mfma_kernel (16) and rtd_bc_tile2_kernel (32 streams per hemisphere) --
  // write u^m at the interfaces themselves; a window in which the 64-stream kernel handed a chain to the row-per-lane kernels
  // (d.split_any) is evaluated by the evaluation kernel instead (rtd_launch_eval); the 66 ... 128-stream kernels (NP = 64) do not
  return d.NP <= 32;
}

void rtd_launch_bc(const RtdDev& d, hipStream_t s, int part) {
  // the fused kernels run in one of the two parts and leave the other empty
  const long nch = (long)d.C * d.M;
  switch (d.NP) {
    case 4:  // 2 ... 16 streams
    case 8:
      if (part == 1) rtd_launch_bc_small(d, s);
      break;
    case 16:  // 18 ... 32 streams
      if (part == 1) hipLaunchKernelGGL(rtd_bc_mfma_kernel, dim3((unsigned)nch), dim3(64), 0, s, d);
      break;
    case 32:  // 34 ... 64 streams: the fused kernel first (rtd_bc_tile2.hip); the chains it could not solve (singular carry block) raise
              // need_split and are solved by the pivoted row-per-lane kernels, which leave at once when none of their chains is flagged
      if (part == 0) {
        (void)hipMemsetAsync(d.need_split, 0, sizeof(int) * (size_t)nch, s);
        (void)hipMemsetAsync(d.split_any, 0, sizeof(int), s);
        rtd_launch_bc_tile2(d, s);
      } else {
        rtd_launch_bc_rows(d, s);
      }
      break;
    case 64:  // 66 ... 128 streams: four wavefronts per chain
      rtd_launch_bc_wide(d, s, part);
      break;
    default: break;
  }
}
