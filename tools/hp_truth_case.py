#!/usr/bin/env python3
"""High-precision (mpmath, 40 digits) arbitration of ANY parity case: when the HIP path and the float64 oracle (= the
reference's algorithm) differ by more than the north star's 1e-6, somebody has to say who is right.

This is the reference's mathematics -- SURVEY Appendix A, i.e. the equations oracle/disort_oracle.py restates -- carried
out in 40-digit arithmetic for every Fourier mode of one column and evaluated at the very points the parity test uses:

  * per (mode, layer) the reference's non-symmetric eigenproblem (alpha - beta)(alpha + beta) V = V k^2
    (_solve_for_gen_and_part_sols.py:179-198) with mpmath's general eigensolver, G = [[V+U, V-U],[V-U, V+U]],
    U = (alpha + beta) V / k; the reference's shortcut for layers without multiple scattering (:119, :162-168) is part of
    the model (decided on the float64 inputs exactly as the reference decides it) and is replicated;
  * the beam particular solution from the 2N x 2N system (A + I/mu0) B = X (:226-231);
  * the thermal particular solution v(tau) = G (sum_q b_q(K) tau^q) (G^-1 M^-1 1) (subroutines.py:746-862);
  * the reference's boundary-condition system, with BDRF surface terms and the Stamnes-Conklin scaling
    (_solve_for_coeffs.py:121-323), by Gaussian elimination with partial pivoting inside the band;
  * the evaluators (_assemble_intensity_and_fluxes.py:170-613): u^m(tau), the Fourier sum, u0, flux_up.

Nothing of the device's algorithm (symmetrisation, Cholesky, one-sided Jacobi, structured block elimination) is used.
The inputs of the hot path (delta-M scaling, quadrature, source rescale: oracle.prepare, float64) are common to all
three parties.  Nakajima-Tanaka corrections are post-processing and are left out (the cases are solved with NT_cor off).

Fixtures: tests/golden/hp/<family>_<seed>.npz = the evaluation points, u [Q, ntau, nphi], u0, flux_up of the truth and,
for the record, the oracle's distance to it.  Families: random32 / random64 / random (the seeded generators of
tests/test_gpu_random_parity.py), golden (a reference-captured case of tests/golden/ref by name), chain (a column of
tests/chain_cases.py, "<NQuad>_L<L>[_s<k>]": deep ill-conditioned chains of up to 41 layers; fields as a phase fixture) and phase (a column of
tests/phase_cases.py, "<NQuad>_<column>": phase functions beyond Henyey-Greenstein, six columns c0 ... c5 per stream count and the
six-layer column "deep" at 94 and 126 streams; these fixtures also carry both parts of flux_down) and thermal (a column of
tests/thermal_deep_cases.py, "<NQuad>_<name>": deep thermal source polynomials.  There the float64 coefficients of the source in the
absolute scaled depth are NOT a common input -- they cannot hold such a polynomial -- and the truth starts from the user's raw
s_poly_coeffs in exact arithmetic (thermal_inputs); mode 0 only, with the tau-derivative and the tau-antiderivative of u0 and the
fluxes, the source loss of the two float64 roads on the same inputs and the cancellation factor R).

Usage (build container; minutes per case on 6 processes):
    python3 tools/hp_truth_case.py random32 9 25          # family, seeds ...
    python3 tools/hp_truth_case.py random64 11
    python3 tools/hp_truth_case.py golden 8ARTS_A
    python3 tools/hp_truth_case.py synth cfg4_9 cfg5_0     # a column of a synthetic BASELINE config (cfg5: ~1.5 h)
    python3 tools/hp_truth_case.py phase 30_c3 94_deep    # columns of tests/phase_cases.py; "phase all": every one of the 80 (~15 min
                                                          # with HP_WORKERS=8: the 36 up to 128 streams of the first set ~7 min, the 44
                                                          # of the padded stream counts and the deep column ~7 min, 126_deep alone ~4)
    python3 tools/hp_truth_case.py phase all --skip-existing   # only the cases whose fixture is missing
    python3 tools/hp_truth_case.py chain 32_L21 64_L25_s3  # columns of tests/chain_cases.py; "chain all": every one of the 33 (~5 min with
                                                          # HP_WORKERS=8; a mode of 128_L9 is the longest single job, ~2.5 min)
    python3 tools/hp_truth_case.py chain all --skip-existing
    python3 tools/hp_truth_case.py fed chain 96_L9_s2 dump.npz   # the 40-digit BC solve and evaluation fed with a device plan's exported
                                                          # G, K, B (run_fed): separates the eigen stage from the elimination
    python3 tools/hp_truth_case.py thermal 6_d13 32_d16    # columns of tests/thermal_deep_cases.py; "thermal all": the 93 (~4 min, HP_WORKERS=8)
    python3 tools/hp_truth_case.py --near-conservative    # every random32 / random64 seed with an omega > 1 - 1e-5 layer
"""
import multiprocessing
import os
import sys
import time
import warnings

import numpy as np
import mpmath as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "pythonic-disort_amd"), os.path.join(ROOT, "tools")]
from oracle import disort_oracle as O  # noqa: E402  (host-side preparation only: delta-M scaling, quadrature, tables)
import nt_truth  # noqa: E402

mp.mp.dps = 40
OUT = os.path.join(ROOT, "tests", "golden", "hp")
WORKERS = int(os.environ.get("HP_WORKERS", "6"))


def mpf(x):
    return mp.mpf(float(x))


def banded_solve(rows, rhs, kl):
    """Gaussian elimination with partial pivoting on a banded system in mpmath numbers.  rows[i] is a dict
    {column: value} of row i; fill stays inside [i - kl, i + 2 kl] as in LAPACK's dgbsv."""
    return [x[0] for x in banded_solve_multi(rows, [[v] for v in rhs], kl)]


def banded_solve_multi(rows, rhs, kl):
    """``banded_solve`` for several right-hand sides at once: rhs[i] is the list of row i's right-hand sides (one elimination,
    the same arithmetic per right-hand side) -> x[i] the list of solutions."""
    n = len(rows)
    K = len(rhs[0])
    zero = mp.mpf(0)
    for c in range(n):
        piv, best = c, abs(rows[c].get(c, zero))
        for r in range(c + 1, min(n, c + kl + 1)):
            v = abs(rows[r].get(c, zero))
            if v > best:
                piv, best = r, v
        if piv != c:
            rows[c], rows[piv] = rows[piv], rows[c]
            rhs[c], rhs[piv] = rhs[piv], rhs[c]
        prow, pv = rows[c], rows[c][c]
        tail = [(k, a) for k, a in prow.items() if k > c]
        for r in range(c + 1, min(n, c + kl + 1)):
            v = rows[r].pop(c, None)
            if v is None or v == 0:
                continue
            f = v / pv
            rr = rows[r]
            for k, a in tail:
                rr[k] = rr.get(k, zero) - f * a
            rc, rr = rhs[c], rhs[r]
            rhs[r] = [rr[q] - f * rc[q] for q in range(K)]
    x = [None] * n
    for c in range(n - 1, -1, -1):
        s = list(rhs[c])
        for k, a in rows[c].items():
            if k > c:
                xk = x[k]
                for q in range(K):
                    s[q] -= a * xk[q]
        x[c] = [v / rows[c][c] for v in s]
    return x


def solve_mode(args):
    """u^m at the points (ts_pts: delta-scaled optical depths, l_pts: their layers) -> float64 [Q, npts], BEFORE the
    rescale factor.  Mirrors oracle.gen_and_part_sols / solve_for_coeffs / Solution._um, in 40 digits.

    The thermal family (p["s_loc"], mode 0 only): K columns that differ in their thermal source alone, as K right-hand sides of one
    elimination.  p["s_loc"][k][l] are the source coefficients of column k about the TOP of layer l in the scaled depth, formed in
    exact arithmetic from the user's raw polynomials (``thermal_inputs``) -- p["s_s"], the float64 coefficients in the absolute
    scaled depth, is not read -- and the particular solution is evaluated in the local variable (its construction is translation
    invariant).  Layers with the same scaled inputs share one decomposition.  -> dict(u [K, 3, Q, npts]: value, d/dtau and the
    antiderivative in tau as the reference's closures define them (_assemble_intensity_and_fluxes.py:170-260: the rates on the
    exponentials, the polynomial of the ABSOLUTE scaled depth differentiated or integrated from tau* = 0, each over / times
    scale_tau), term = the largest single term |G_ij b_q x^q z_j| of the particular solutions at the points, [K])."""
    p, m, ts_pts, l_pts = args
    s_loc = p.get("s_loc")
    K = len(s_loc) if s_loc is not None else 1
    mp.mp.dps = 40
    L, N, P = p["L"], p["N"], p["P"]
    Q = 2 * N
    mu = [mpf(x) for x in p["mu"]]
    w = [mpf(x) for x in p["W"]]
    beam, iso = bool(p["beam"]), bool(p["iso"]) and m == 0
    mu0 = mpf(p["mu0"])
    ts = [mpf(x) for x in p["tau_s0"]]
    one, zero = mp.mpf(1), mp.mpf(0)

    def leg(x):
        # sqrt((l-m)!/(l+m)!) P_l^m(x) up to the common sign (-1)^m, which cancels in every product: the reference's poch
        # factor (:96) split over both factors.  Normalised three-term recurrence in 40-digit arithmetic (mpmath's legenp
        # sums a hypergeometric series that does not converge at degree ~60, order ~40).
        out = [zero] * P
        if m >= P:
            return out
        v = one
        for jj in range(1, m + 1):
            v = v * mp.sqrt(mp.mpf(2 * jj - 1) / (2 * jj)) * mp.sqrt(1 - x * x)
        out[m] = v
        if m + 1 < P:
            out[m + 1] = mp.sqrt(2 * m + 1) * x * v
        for ell in range(m + 1, P - 1):
            out[ell + 1] = ((2 * ell + 1) * x * out[ell] - mp.sqrt(mp.mpf((ell + m) * (ell - m))) * out[ell - 1]) \
                / mp.sqrt(mp.mpf((ell + 1 - m) * (ell + 1 + m)))
        return out
    Y = [leg(x) for x in mu]
    Y0 = leg(-mu0) if beam else None
    Gs, Ks, Bs, Zs = [], [], [], []
    seen = {}
    fed = p.get("fed")  # G [M, L, Q, Q], K, B [M, L, Q] of a device plan (Plan.tensors): the eigen stage is then the device's
    for l in range(L):
        if fed is not None:
            assert not iso, "fed tensors: beam and boundary sources only"
            Gs.append(mp.matrix([[mpf(x) for x in row] for row in fed["G"][m][l]]))
            Ks.append([mpf(x) for x in fed["K"][m][l]])
            Bs.append([mpf(x) for x in fed["B"][m][l]])
            continue
        c64 = 0.5 * p["omega_s"][l] * p["wleg"][l, m:]
        same = seen.setdefault((float(p["omega_s"][l]), np.asarray(p["wleg"][l], float).tobytes()), l)
        if same != l:  # a layer with these very inputs has been decomposed
            Gs.append(Gs[same])
            Ks.append(Ks[same])
            Bs.append(Bs[same])
            if iso:
                Zs.append(Zs[same])
            continue
        if not np.any(np.abs(c64) > 1e-8):  # the reference's shortcut (:119, :162-168), decided on the float64 inputs
            G = mp.zeros(Q)
            for i in range(N):
                G[i, N + i] = G[N + i, i] = one
            Gs.append(G)
            Ks.append([-1 / x for x in mu] + [1 / x for x in mu])
            Bs.append([zero] * Q)
            if iso:  # G_inv = trivial (:168): z = trivial [1/mu; -1/mu]
                Zs.append([-1 / x for x in mu] + [1 / x for x in mu])
            continue
        om = mpf(p["omega_s"][l])
        wl = [mpf(x) for x in p["wleg"][l]]
        sgn = [(-1) ** (ell - m) for ell in range(P)]
        al, be = mp.zeros(N), mp.zeros(N)
        for i in range(N):
            for j in range(N):
                sp = sm = zero
                for ell in range(m, P):
                    t = om / 2 * wl[ell] * Y[i][ell] * Y[j][ell]
                    sp += t
                    sm += t * sgn[ell]
                al[i, j] = (sp * w[j] - (1 if i == j else 0)) / mu[i]
                be[i, j] = sm * w[j] / mu[i]
        ev, V = mp.eig((al - be) * (al + be))
        k = [mp.sqrt(mp.re(e)) for e in ev]
        V = V.apply(mp.re)
        U = (al + be) * V
        for j in range(N):
            for i in range(N):
                U[i, j] /= k[j]
        G = mp.zeros(Q)
        for i in range(N):
            for j in range(N):
                G[i, j] = G[N + i, N + j] = V[i, j] + U[i, j]
                G[i, N + j] = G[N + i, j] = V[i, j] - U[i, j]
        Gs.append(G)
        Ks.append([-x for x in k] + k)
        if beam:
            A = mp.zeros(Q)
            for i in range(N):
                for j in range(N):
                    A[i, j], A[i, N + j], A[N + i, j], A[N + i, N + j] = -al[i, j], -be[i, j], be[i, j], al[i, j]
            X = mp.zeros(Q, 1)
            for i in range(N):
                xp = xm = zero
                for ell in range(m, P):
                    t = mpf(p["I0_4pi"]) * (1 if m == 0 else 2) * om * wl[ell] * Y0[ell] * Y[i][ell]
                    xp += t
                    xm += t * sgn[ell]
                X[i], X[N + i] = xp / mu[i], -xm / mu[i]
            Bs.append(list(mp.lu_solve(A + mp.eye(Q) / mu0, X)))
        else:
            Bs.append([zero] * Q)
        if iso:  # z = G^-1 [1/mu; -1/mu]  (_assemble_intensity_and_fluxes.py:124)
            rhs = mp.matrix([1 / x for x in mu] + [-1 / x for x in mu])
            Zs.append(list(mp.lu_solve(G, rhs)))

    Ns = p["Ns"]

    def vth(l, t):  # thermal particular solution at delta-scaled tau t in layer l (subroutines.py:822-862)
        s_row = [mpf(x) for x in p["s_s"][l]]
        poly = [zero] * Q
        for j in range(Q):
            kk = Ks[l][j]
            acc = zero
            for q in range(Ns):
                bq = zero
                for jj in range(q, Ns):
                    bq += mp.factorial(jj) / mp.factorial(q) * s_row[jj] / kk ** (jj - q + 1)
                acc += bq * t**q
            poly[j] = acc * Zs[l][j]
        return [sum(Gs[l][i, j] * poly[j] for j in range(Q)) for i in range(Q)]

    bq_cache = {}

    def bq_local(k, l):  # [Q][Ns]: b_q(K_j) z_j of column k's source about the top of layer l
        if (k, l) not in bq_cache:
            row = s_loc[k][l]
            fact = [mp.factorial(q) for q in range(Ns)]
            bq_cache[k, l] = [[sum(fact[jj] / fact[q] * row[jj] / Ks[l][j] ** (jj - q + 1) for jj in range(q, Ns)) * Zs[l][j]
                               for q in range(Ns)] for j in range(Q)]
        return bq_cache[k, l]

    def poly_local(k, l, t, order=0):  # [Q]: sum_q b_q z_j x^q at x = t - ts[l], its d/dtau or its antiderivative from tau* = 0
        x, sc = t - ts[l], mpf(p["scale_tau"][l])
        out = []
        for row in bq_local(k, l):
            if order == 0:
                out.append(sum(b * x**q for q, b in enumerate(row)))
            elif order == 1:
                out.append(sc * sum(q * b * x ** (q - 1) for q, b in enumerate(row) if q))
            else:
                out.append(sum(b * (x ** (q + 1) - (-ts[l]) ** (q + 1)) / (q + 1) for q, b in enumerate(row)) / sc)
        return out

    def vth_local(l, t):  # [Q][K]
        cols = []
        for k in range(K):
            pl = poly_local(k, l, t)
            cols.append([sum(Gs[l][i, j] * pl[j] for j in range(Q)) for i in range(Q)])
        return [[cols[k][i] for k in range(K)] for i in range(Q)]

    def expo(l, j, t):  # every exponential referenced to the boundary of its layer where it is <= 1
        kk = Ks[l][j]
        return mp.e ** (kk * (t - (ts[l + 1] if kk > 0 else ts[l])))

    has_bdrf = len(p["bdrf"]) > m
    if has_bdrf:  # _solve_for_coeffs.py:121-134
        R = [[(2 if m == 0 else 1) * mpf(p["bdrf"][m][0][i, j]) * mu[j] * w[j] for j in range(N)] for i in range(N)]
        Xs = [mu0 * mpf(p["I0_4pi"]) * 4 * mpf(p["bdrf"][m][1][i]) for i in range(N)]
    n = Q * L
    rows, rhs = [dict() for _ in range(n)], [None] * n
    r = 0

    def vthK(l, t):  # [Q][K]
        return vth_local(l, t) if s_loc is not None else [[v] for v in vth(l, t)]
    v_top = vthK(0, ts[0]) if iso else None
    for i in range(N):  # top boundary: downward streams
        for j in range(Q):
            rows[r][j] = Gs[0][N + i, j] * expo(0, j, ts[0])
        v = mpf(p["b_neg"][i, m]) - Bs[0][N + i] * mp.e ** (-ts[0] / mu0)
        rhs[r] = [v - v_top[N + i][k] for k in range(K)] if iso else [v]
        r += 1
    for l in range(L - 1):
        t = ts[l + 1]
        if iso:
            va, vb = vthK(l, t), vthK(l + 1, t)
        for i in range(Q):
            for j in range(Q):
                rows[r][l * Q + j] = Gs[l][i, j] * expo(l, j, t)
                rows[r][(l + 1) * Q + j] = -Gs[l + 1][i, j] * expo(l + 1, j, t)
            v = (Bs[l + 1][i] - Bs[l][i]) * mp.e ** (-t / mu0)
            rhs[r] = [v + (vb[i][k] - va[i][k]) for k in range(K)] if iso else [v]
            r += 1
    tb = ts[L]
    vb = vthK(L - 1, tb) if iso else [[zero]] * Q
    att = mp.e ** (-tb / mu0) if beam else zero
    GL, BL = Gs[L - 1], Bs[L - 1]
    for i in range(N):  # bottom boundary: upward streams; surface reflection (:288-293, :232, :246-252)
        for j in range(Q):
            g = GL[i, j]
            if has_bdrf:
                g = g - sum(R[i][q] * GL[N + q, j] for q in range(N))
            rows[r][(L - 1) * Q + j] = g * expo(L - 1, j, tb)
        vs = []
        for k in range(len(vb[0])):
            v = mpf(p["b_pos"][i, m]) - BL[i] * att - vb[i][k]
            if has_bdrf:
                v += sum(R[i][q] * (BL[N + q] * att + vb[N + q][k]) for q in range(N))
                if beam:
                    v += Xs[i] * att
            vs.append(v)
        rhs[r] = vs
        r += 1
    CK = banded_solve_multi(rows, rhs, 3 * N - 1)
    if s_loc is not None:
        out = np.zeros((K, 3, Q, len(ts_pts)))
        term = [zero] * K
        gmax = {}
        for ti, (t64, l) in enumerate(zip(ts_pts, l_pts)):
            t, l = mpf(t64), int(l)
            sc = mpf(p["scale_tau"][l])
            x = t - ts[l]
            if id(Gs[l]) not in gmax:
                gmax[id(Gs[l])] = [max(abs(Gs[l][i, j]) for i in range(Q)) for j in range(Q)]
            for k in range(K):
                if iso:
                    term[k] = max([term[k]] + [gmax[id(Gs[l])][j] * abs(b * x**q) for j, row in enumerate(bq_local(k, l))
                                               for q, b in enumerate(row)])
                for oi, order in enumerate((0, 1, -1)):
                    e = [expo(l, j, t) * CK[l * Q + j][k] * (1 if order == 0 else (sc * Ks[l][j]) ** order) for j in range(Q)]
                    if iso:
                        e = [a + b for a, b in zip(e, poly_local(k, l, t, order))]
                    bt = (mp.e ** (-t / mu0) * (1 if order == 0 else (-sc / mu0) ** order)) if beam else zero
                    for i in range(Q):
                        out[k, oi, i, ti] = float(Bs[l][i] * bt + sum(Gs[l][i, j] * e[j] for j in range(Q)))
        return dict(u=out, term=np.array([float(v) for v in term]))
    Cc = [v[0] for v in CK]
    out = np.zeros((Q, len(ts_pts)))
    for ti, (t64, l) in enumerate(zip(ts_pts, l_pts)):
        t = mpf(t64)
        l = int(l)
        ex = [expo(l, j, t) * Cc[l * Q + j] for j in range(Q)]
        bt = mp.e ** (-t / mu0) if beam else zero
        vv = vth(l, t) if iso else None
        for i in range(Q):
            v = Bs[l][i] * bt
            for j in range(Q):
                v += Gs[l][i, j] * ex[j]
            if iso:
                v += vv[i]
            out[i, ti] = float(v)
    return out


def _mode_jobs(kw, tau):
    """(prepared inputs, one solve_mode job per Fourier mode) of a case at the optical depths tau."""
    kw = dict(kw)
    kw.pop("NT_cor", None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = O.prepare(**kw)
    if not p["beam"]:
        p["mu0"] = 1.0  # no beam: every beam term carries the factor I0 = 0
    _, l_pts, ts_pts = O.Solution._locate(type("S", (), {"p": p})(), tau)
    return p, [(p, m, ts_pts, l_pts) for m in range(p["M"])]


def _from_modes(p, um, phi):
    um = np.stack(um)  # [M, Q, ntau]
    u0 = p["rescale"] * um[0]
    fup = p["rescale"] * 2 * np.pi * (p["mu"] * p["W"]) @ um[0][:p["N"]]
    if p["only_flux"]:
        return None, u0, fup
    cosm = np.cos(np.arange(p["M"])[:, None] * (p["phi0"] - np.atleast_1d(np.asarray(phi, float)))[None, :])
    return p["rescale"] * np.einsum("mit,mp->itp", um, cosm), u0, fup


def truth(kw, tau, phi, parallel=True):
    """(u [Q, ntau, nphi] or None when only_flux, u0 [Q, ntau], flux_up [ntau]) of the 40-digit solution at optical depths
    tau and azimuths phi, in the units of the inputs.  parallel: one process per Fourier mode."""
    p, jobs = _mode_jobs(kw, tau)
    if parallel and p["M"] > 1:
        with multiprocessing.Pool(min(WORKERS, p["M"])) as pool:
            um = pool.map(solve_mode, jobs, chunksize=1)
    else:
        um = [solve_mode(j) for j in jobs]
    return _from_modes(p, um, phi)


def flux_down_of(kw, tau, u0):
    """(diffuse, direct) of flux_down from the truth's u0 as the reference forms them (_assemble_intensity_and_fluxes.py:568-601):
    the quadrature sum over the downward streams plus the delta-scaled direct beam minus the unscaled one, and the unscaled direct
    beam in closed form.  Sums of positive terms and two exponentials: benign in float64."""
    kw = dict(kw)
    kw.pop("NT_cor", None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = O.prepare(**kw)
    tau, l_pts, ts_pts = O.Solution._locate(type("S", (), {"p": p})(), tau)
    direct = direct_s = np.zeros(len(tau))
    if p["beam"]:
        direct = p["rescale"] * p["I0"] * p["mu0"] * np.exp(-tau / p["mu0"])
        direct_s = p["rescale"] * p["I0"] * p["mu0"] * np.exp(-ts_pts / p["mu0"])
    return 2 * np.pi * (p["mu"] * p["W"]) @ u0[p["N"]:] + direct_s - direct, direct


def case_of(family, key):
    """(kwargs, tau, phi) of a random case exactly as its parity test builds them."""
    import test_gpu_random_parity as T
    seed = int(key)
    kw = {"random": T.make_case, "random32": T.make_case_many_streams, "random64": T.make_case_64_streams,
          "random128": T.make_case_128_streams}[family](seed)
    tau, phi = T.eval_points(family, seed, kw)
    return kw, tau, phi


def case_synth(key):
    """A column of a synthetic BASELINE config, "cfg4_<i>" or "cfg5_<i>", at the points of its reference-computed golden
    (tests/golden/synth/<cfg>.npz); the tabulated BDRF modes of cfg5 become callables on the quadrature grid."""
    from pydisort_amd import synthetic
    name, col = key.rsplit("_", 1)
    col = int(col)
    if name == "cfg4cloud":  # cfg4 with a conservative cloud layer in every column (bench.py's all-cloud leg): own points
        cfg = synthetic.cfg4_cloud_columns(col + 1)
        kw = synthetic.column_kwargs(cfg, col)
        t = np.concatenate(([0.0], cfg["tau_arr"][col]))
        return kw, np.sort(np.concatenate((t, 0.5 * (t[1:] + t[:-1])))), np.array([0.0, np.pi / 2, np.pi, 2.5])
    cfg = {"cfg4": synthetic.cfg4_columns, "cfg5": synthetic.cfg5_columns}[name](col + 1)
    kw = synthetic.column_kwargs(cfg, col)
    if "bdrf_q" in cfg:
        q, q0 = cfg["bdrf_q"][col], cfg["bdrf_q0"][col]
        kw["BDRF_Fourier_modes"] = [(lambda mu, nmup, m=m: q0[m][:, None] if len(np.atleast_1d(nmup)) == 1 else q[m])
                                    for m in range(q.shape[0])]
    z = np.load(os.path.join(ROOT, "tests", "golden", "synth", name + ".npz"))
    return kw, z[f"c{col}.tau_pts"], z["phi"]


def _nt_correction(kw, tau, phi):
    """The Nakajima-Tanaka terms the reference adds to u when NT_cor is on (pydisort.py:375-698): closed forms of the INPUTS
    (optical depths, phase-function moments, beam), independent of the solved coefficients -- evaluated in 40 digits by
    tools/nt_truth.py, which shares no code with oracle/.  (The committed golden_4a / 4b / 5a / 5b fixtures predate it: their NT
    part is the float64 oracle's u(NT_cor=True) - u(NT_cor=False); tests/test_nt_truth_cpu.py holds that difference against the
    40-digit terms at the same points.)"""
    return nt_truth.correction(kw, tau, phi)["value"]


def _golden_call(job):
    kw, tau, phi, parallel = job
    u, u0, fup = truth(kw, tau, phi, parallel=parallel)
    return u, fup


def run_golden(test_id):
    """A reference-captured case (tests/golden/ref/<test_id>.npz): the truth of the FIRST plain `u(tau, phi)` evaluation
    of every captured pydisort call, stored as c<i>.u with the shape the reference returned (squeezed axes); calls made with
    the Nakajima-Tanaka corrections on get the (input-only, 40-digit: tools/nt_truth.py) correction terms added: c<i>.nt = 1 and
    c<i>.nt_provenance."""
    import goldens
    calls = goldens.load(test_id)
    jobs, meta = [], []
    for ci, call in enumerate(calls):
        for ev in call["evals"]:
            if ev["name"] == "u" and not ev["kwargs"] and len(ev["args"]) == 2:
                kw = {k: v for k, v in call["kwargs"].items() if k != "autograd_compatible"}
                jobs.append([kw, np.atleast_1d(ev["args"][0]), np.atleast_1d(ev["args"][1]), False])
                meta.append((ci, np.shape(ev["out"]), ev["out"], goldens.nt_is_active(kw)))
                break
    t0 = time.time()
    if len(jobs) < WORKERS:  # few calls: the Fourier modes of a call side by side instead of the calls
        for j in jobs:
            j[3] = True
        outs = [_golden_call(j) for j in jobs]
    else:
        with multiprocessing.Pool(WORKERS) as pool:
            outs = pool.map(_golden_call, jobs, chunksize=1)
    res, worst, worst_scale = {}, 0.0, 0.0
    for (ci, shape, ref_out, nt), (u, fup), job in zip(meta, outs, jobs):
        u = u.reshape(shape)
        if nt:
            u = u + np.asarray(_nt_correction(job[0], job[1], job[2])).reshape(shape)
            res[f"c{ci}.nt"] = np.array(1)
            res[f"c{ci}.nt_provenance"] = np.array(nt_truth.PROVENANCE)
        res[f"c{ci}.u"] = u
        res[f"c{ci}.flux_up"] = fup
        big = np.abs(u) > 1e-8 * np.max(np.abs(u))
        worst = max(worst, float(np.max(np.abs(ref_out - u)[big] / np.abs(u)[big])))
        worst_scale = max(worst_scale, float(np.max(np.abs(ref_out - u)) / np.max(np.abs(u))))
    res["reference_u_pointwise_rel"] = worst
    res["reference_u_scale_rel"] = worst_scale
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"golden_{test_id}.npz"), **res)
    print(f"golden/{test_id}: {len(jobs)} calls, {time.time() - t0:.0f} s; the reference's own float64 result vs truth: "
          f"{worst_scale:.2e} of the scale, {worst:.2e} pointwise", flush=True)


def case_phase(key):
    """A column of tests/phase_cases.py, "<NQuad>_<column>", at its own points."""
    import phase_cases
    kw = phase_cases.case(key)
    return (kw,) + tuple(phase_cases.points(kw))


def thermal_inputs(kw):
    """(prepared inputs of the hot path WITHOUT the float64 source polynomials' say, the source coefficients about the top of each
    layer in the scaled depth as 40-digit numbers [L][Ns], divided by the rescale factor): formed from the RAW s_poly_coeffs,
    tau_arr, omega and the float64 scale_tau in exact rational arithmetic (tests/thermal_deep_cases.py: exact_local_scaled)."""
    import thermal_deep_cases as TD
    kw = dict(kw)
    kw.pop("NT_cor", None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = O.prepare(**kw)
    if not p["beam"]:
        p["mu0"] = 1.0
    exact, _ = TD.exact_local_scaled(kw)
    res = mpf(p["rescale"])
    return p, [[mp.mpf(b.numerator) / mp.mpf(b.denominator) / res for b in row] for row in exact]


def solve_thermal(job):
    """Mode 0 of the columns `kws` of ONE atmosphere (they differ in s_poly_coeffs only) at the optical depths tau ->
    per column dict(u0 [3, Q, ntau]: value, d/dtau, antiderivative; flux_up, flux_down_diffuse [3, ntau]; R)."""
    kws, tau = job
    mp.mp.dps = 40
    prepared = [thermal_inputs(kw) for kw in kws]
    p = dict(prepared[0][0])
    Ns = max(len(s[0]) for _, s in prepared)
    zero = mp.mpf(0)
    # one rescale factor for the common elimination: every column's source in the units of the first column's factor
    p["s_loc"] = [[list(row) + [zero] * (Ns - len(row)) for row in
                   [[b * mpf(q["rescale"]) / mpf(p["rescale"]) for b in r] for r in s]] for q, s in prepared]
    p["Ns"], p["iso"] = Ns, True
    _, l_pts, ts_pts = O.Solution._locate(type("S", (), {"p": p})(), tau)
    sol = solve_mode((p, 0, ts_pts, l_pts))
    N, wts = p["N"], 2 * np.pi * (p["mu"] * p["W"])
    out = []
    for k in range(len(kws)):
        u0 = p["rescale"] * sol["u"][k]
        out.append(dict(u0=u0, flux_up=np.einsum("i,oit->ot", wts, u0[:, :N]), flux_down_diffuse=np.einsum("i,oit->ot", wts, u0[:, N:]),
                        R=p["rescale"] * sol["term"][k] / np.max(np.abs(u0[0]))))
    return out


def _thermal_losses(kw):
    """Source error, over the layer's largest source value, of the two float64 roads on these inputs: the substitution
    tau* = scale tau + shift of the reference's front end (then shifted exactly to the layer's top), and the plain-Horner Taylor
    shift of the raw polynomial."""
    import thermal_deep_cases as TD
    from fractions import Fraction
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = O.prepare(**kw)
    exact, width = TD.exact_local_scaled(kw)
    res = Fraction(float(p["rescale"]))
    sub = [[b * res for b in TD.local_exact(p["s_s"][l], p["tau_s0"][l])] for l in range(p["L"])]
    tau = np.atleast_1d(kw["tau_arr"])
    top = np.concatenate(([0.0], tau[:-1]))
    a = np.atleast_2d(kw["s_poly_coeffs"])
    raw_exact = [TD.local_exact(a[l], top[l]) for l in range(p["L"])]
    horner = [TD.horner_shift(a[l], float(top[l])) for l in range(p["L"])]
    thick = [Fraction(float(tau[l])) - Fraction(float(top[l])) for l in range(p["L"])]
    return TD.source_error(sub, exact, width)[0], TD.source_error(horner, raw_exact, thick)[0]


def run_thermal(keys):
    """The columns of tests/thermal_deep_cases.py: the columns of one atmosphere (stream count; delta-M, its twin or the thin one)
    are the right-hand sides of one elimination; the atmospheres go through one pool, the largest first."""
    import thermal_deep_cases as TD
    t0 = time.time()
    groups = {}
    for key in keys:
        q, name = key.split("_")
        groups.setdefault((int(q), "thin" if name == "thin" else name[0]), []).append(key)
    order = sorted(groups, key=lambda g: -g[0] ** 3 * TD.layer_count(g[0]))
    jobs = [([TD.case(k) for k in groups[g]], TD.points(TD.case(groups[g][0]))) for g in order]
    with multiprocessing.Pool(WORKERS) as pool:
        sols = pool.map(solve_thermal, jobs, chunksize=1)
    os.makedirs(OUT, exist_ok=True)
    for g, (kws, tau), sol in zip(order, jobs, sols):
        for key, kw, s in zip(groups[g], kws, sol):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref = O.pydisort(**kw)
            sub, horner = _thermal_losses(kw)
            res = dict(tau=tau, u0=s["u0"][0], flux_up=s["flux_up"][0], flux_down_diffuse=s["flux_down_diffuse"][0],
                       flux_down_direct=np.zeros(len(tau)), R=s["R"], loss_substitution=sub, loss_horner=horner,
                       oracle_u0_scale_rel=np.max(np.abs(ref[3](tau) - s["u0"][0])) / np.max(np.abs(s["u0"][0])))
            for oi, order_name in ((1, "derivative"), (2, "antiderivative")):
                for qn in ("u0", "flux_up", "flux_down_diffuse"):
                    res[f"{order_name}.{qn}"] = s[qn][oi]
            np.savez_compressed(TD.fixture_path(key), **res)
            print(f"thermal/{key}: {time.time() - t0:.0f} s; R {float(s['R']):.1e}, loss substitution {sub:.1e} horner {horner:.1e}, "
                  f"oracle vs truth u0 {float(res['oracle_u0_scale_rel']):.2e}", flush=True)


def _record(family, key, kw, tau, phi, u, u0, fup, seconds):
    kwo = dict(kw)
    kwo.pop("NT_cor", None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = O.pydisort(**kwo)
    res = dict(tau=tau, phi=phi, u0=u0, flux_up=fup, oracle_u0_scale_rel=np.max(np.abs(ref[3](tau) - u0)) / np.max(np.abs(u0)))
    if u is not None:
        ou = ref[4](tau, phi)
        res.update(u=u, oracle_u_scale_rel=np.max(np.abs(ou - u)) / np.max(np.abs(u)))
        big = np.abs(u) > 1e-8 * np.max(np.abs(u))
        res["oracle_u_pointwise_rel"] = np.max(np.abs(ou - u)[big] / np.abs(u)[big])
    if family in ("phase", "chain"):
        res["flux_down_diffuse"], res["flux_down_direct"] = flux_down_of(kw, tau, u0)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"{family}_{key}.npz"), **res)
    print(f"{family}/{key}: NQuad {kw['NQuad']}, {len(np.atleast_1d(kw['tau_arr']))} layers, {seconds:.0f} s; oracle vs truth: "
          + ", ".join(f"{k[7:]} {float(v):.2e}" for k, v in res.items() if k.startswith("oracle_")), flush=True)


def run(family, key):
    kw, tau, phi = case_synth(key) if family == "synth" else case_of(family, key)
    t0 = time.time()
    u, u0, fup = truth(kw, tau, phi)
    _record(family, key, kw, tau, phi, u, u0, fup, time.time() - t0)


def case_chain(key):
    """A column of tests/chain_cases.py, "<NQuad>_L<L>" or "<NQuad>_L<L>_s<k>", at its own points."""
    import chain_cases
    kw = chain_cases.case(key)
    return (kw,) + tuple(chain_cases.points(kw))


def run_phase(keys, family="phase"):
    """The cases of tests/phase_cases.py (or, family "chain", of tests/chain_cases.py): the Fourier modes of ALL of them through one
    pool, the largest first (a case has three modes only, so case by case the workers would idle)."""
    t0 = time.time()
    cases = {key: (case_chain if family == "chain" else case_phase)(key) for key in keys}
    prepared = {key: _mode_jobs(kw, tau) for key, (kw, tau, phi) in cases.items()}
    # the cost of a mode: the banded elimination, ~ NQuad^3 per layer
    order = sorted(keys, key=lambda k: -cases[k][0]["NQuad"] ** 3 * len(cases[k][0]["tau_arr"]))
    flat = [(key, job) for key in order for job in prepared[key][1]]
    with multiprocessing.Pool(WORKERS) as pool:
        ums = pool.map(solve_mode, [job for _, job in flat], chunksize=1)
    for key in order:
        kw, tau, phi = cases[key]
        u, u0, fup = _from_modes(prepared[key][0], [um for (k, _), um in zip(flat, ums) if k == key], phi)
        _record(family, key, kw, tau, phi, u, u0, fup, time.time() - t0)


def run_fed(family, key, dump):
    """Who owns a distance from the truth: the 40-digit boundary-condition solve and evaluation fed with the tensors G, K, B that a
    device plan exported (Plan.tensors of the one-column solve, saved with np.savez beside the device's own u, u0, flux_up at the
    case's points).  fed <-> truth is what the eigen stage's float64 tensors cost, device <-> fed what elimination and evaluation
    add (10_c0, the deep chains).  Prints both per quantity and the point of the worst pointwise figure."""
    kw, tau, phi = (case_chain if family == "chain" else case_phase)(key)
    z = np.load(dump)
    t0 = time.time()
    p, jobs = _mode_jobs(kw, tau)
    p["fed"] = dict(G=z["G"], K=z["K"], B=z["B"])
    with multiprocessing.Pool(min(WORKERS, p["M"])) as pool:
        um = pool.map(solve_mode, jobs, chunksize=1)
    fed = dict(zip(("u", "u0", "flux_up"), _from_modes(p, um, phi)))
    truth = np.load(os.path.join(OUT, f"{family}_{key}.npz"))
    np.savez_compressed(os.path.splitext(dump)[0] + "_fed.npz", **fed)

    def dist(a, b):
        scale = np.max(np.abs(b))
        big = np.abs(b) > 1e-8 * scale
        rel = np.where(big, np.abs(a - b) / np.where(big, np.abs(b), 1.0), 0.0)
        at = np.unravel_index(np.argmax(rel), rel.shape)
        return (f"{np.max(np.abs(a - b)) / scale:.2e} of the scale, {rel[at]:.2e} pointwise at {tuple(int(i) for i in at)} "
                f"(|value| {abs(b[at]) / scale:.1e} of the scale, |error| {abs(a[at] - b[at]) / scale:.1e})")
    print(f"fed {family}/{key}: {time.time() - t0:.0f} s")
    for k in ("u", "u0", "flux_up"):
        print(f"  {k}: fed    <-> truth: {dist(fed[k], truth[k])}")
        print(f"  {k}: device <-> truth: {dist(z[k], truth[k])}")
        print(f"  {k}: device <-> fed:   {dist(z[k], fed[k])}", flush=True)


def near_conservative_seeds():
    import test_gpu_random_parity as T
    out = []
    for family, make, n in (("random32", T.make_case_many_streams, 40), ("random64", T.make_case_64_streams, 12)):
        for seed in range(n):
            if np.any(make(seed)["omega_arr"] > 1 - 1e-5):
                out.append((family, str(seed)))
    return out


if __name__ == "__main__":
    if sys.argv[1:2] == ["fed"]:
        run_fed(*sys.argv[2:5])
        sys.exit(0)
    if "--near-conservative" in sys.argv:
        todo = near_conservative_seeds()
        if "--list" in sys.argv:
            print(todo)
            sys.exit(0)
    else:
        todo = [(sys.argv[1], k) for k in sys.argv[2:] if not k.startswith("--")]
    if ("phase", "all") in todo:
        import phase_cases
        todo = [t for t in todo if t != ("phase", "all")] + [("phase", k) for k in phase_cases.keys() + [phase_cases.NEGATIVE]]
    if ("chain", "all") in todo:
        import chain_cases
        todo = [t for t in todo if t != ("chain", "all")] + [("chain", k) for k in chain_cases.keys()]
    if "--skip-existing" in sys.argv:
        todo = [(f, k) for f, k in todo if f == "golden" or not os.path.exists(os.path.join(OUT, f"{f}_{k}.npz"))]
    if ("thermal", "all") in todo:
        import thermal_deep_cases
        todo = [t for t in todo if t != ("thermal", "all")] + [("thermal", k) for k in thermal_deep_cases.keys()]
        if "--skip-existing" in sys.argv:
            todo = [(f, k) for f, k in todo if f != "thermal" or not os.path.exists(thermal_deep_cases.fixture_path(k))]
    phase = [k for f, k in todo if f == "phase"]
    if phase:
        run_phase(phase)
    chain = [k for f, k in todo if f == "chain"]
    if chain:
        run_phase(chain, "chain")
    thermal = [k for f, k in todo if f == "thermal"]
    if thermal:
        run_thermal(thermal)
    for family, key in todo:
        if family in ("phase", "chain", "thermal"):
            continue
        if family == "golden":
            run_golden(key)
            continue
        run(family, key)
