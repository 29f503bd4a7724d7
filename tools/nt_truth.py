#!/usr/bin/env python3
"""40-digit arbiter of the Nakajima-Tanaka intensity corrections (TMS + IMS), independent of oracle/ and of the package.

The corrections are closed forms of the INPUTS of one ``pydisort`` call: no eigenproblem, no linear solve.  This module
evaluates them in mpmath at 40 digits from the reference's equations (pydisort.py:409-479 the in-layer TMS terms, :489-589
the contributions of the other layers, :601-638 IMS), written as attenuation differences over layer segments instead of the
reference's cumulative sums with ``expm1`` branches:

    upward stream mu at scaled depth t* in layer l:   E(t) = exp(-t/mu0 - (t - t*)/mu),
        in-layer  E(t*) - E(t_{l+1}),   layer r > l:  g_r (E(t_r) - E(t_{r+1}))
    downward stream:                                  D(t) = exp(-t/mu0 - (t* - t)/mu),
        in-layer  D(t*) - D(t_l),       layer r < l:  g_r (D(t_{r+1}) - D(t_r))

with g_r = 1 for the value, +-mu / scale_tau[r] for the reference's tau-antiderivative (:513-515, :524, :570) and
+-scale_tau[l] / mu for the tau-derivative (every term is an exponential of t*, d t*/d tau = scale_tau[l]).  As in the reference
every layer's contribution carries mathscr_B of the layer that CONTAINS the point (:541, :584), the layer of a point is
``argmax(tau <= tau_arr)`` (an interface belongs to the layer that ends there) and the IMS averages are weighted with the
cumulative ``tau_arr`` (:601-610).  The tau-derivative has no counterpart in the reference: it is d/d tau of the value within
the point's layer.

The quadrature nodes are the zeros of P_N mapped to (0, 1), refined by Newton's method in 40 digits and rounded to float64:
like every other float64 input they are then taken as exact.  Everything else stays in 40 digits until the result is rounded.

    truth = nt_truth.correction(kw, tau, phi)   # -> dict(value=, antiderivative=, derivative=), each [NQuad, ntau, nphi]

in the units of ``I0`` (the correction is linear in I0: no rescale factor enters).
"""
import numpy as np
import mpmath as mp

DPS = 40
ORDERS = ("value", "antiderivative", "derivative")
PROVENANCE = "40-digit closed form (tools/nt_truth.py)"


def quadrature_nodes(N):
    """Zeros of P_N on (-1, 1) mapped to (0, 1), ascending, as float64 (Newton in 40 digits from numpy's zeros)."""
    with mp.workdps(DPS):
        out = []
        for x0 in np.polynomial.legendre.leggauss(int(N))[0]:
            x = mp.mpf(float(x0))
            for _ in range(4):
                pm1, p = mp.mpf(1), x
                for ell in range(1, N):
                    pm1, p = p, ((2 * ell + 1) * x * p - ell * pm1) / (ell + 1)
                x = x - p * (x * x - 1) / (N * (x * p - pm1))  # P_N' = N (x P_N - P_{N-1}) / (x^2 - 1)
            out.append(float((x + 1) / 2))
    return np.array(out)


def _legendre_values(n, x):
    out = [mp.mpf(1), x][:n]
    for ell in range(1, n - 1):
        out.append(((2 * ell + 1) * x * out[ell] - ell * out[ell - 1]) / (ell + 1))
    return out


def _dot(c, p):
    s = mp.mpf(0)
    for a, b in zip(c, p):
        s += a * b
    return s


def correction(kw, tau, phi):
    """kw: the keyword arguments of one pydisort call (tau_arr, omega_arr, NQuad, Leg_coeffs_all, mu0, I0, phi0, f_arr and
    optionally NLeg; anything else is ignored: the corrections do not depend on it).  tau [ntau], phi [nphi]: the points."""
    with mp.workdps(DPS):
        return _correction(kw, tau, phi)


def _correction(kw, tau, phi):
    F = lambda v: mp.mpf(float(v))  # noqa: E731
    tau_arr = np.atleast_1d(np.asarray(kw["tau_arr"], float))
    L = len(tau_arr)
    omega64 = np.broadcast_to(np.asarray(kw["omega_arr"], float), (L,))
    f64 = np.broadcast_to(np.asarray(kw.get("f_arr", 0), float), (L,))
    leg64 = np.atleast_2d(np.asarray(kw["Leg_coeffs_all"], float))
    NQuad = int(kw["NQuad"])
    N = NQuad // 2
    NLeg = NQuad if kw.get("NLeg") is None else int(kw["NLeg"])
    nall = leg64.shape[1]
    if not (np.any(f64 > 0) and NLeg < nall and np.any(omega64 > 0) and float(kw["I0"]) > 0):
        raise ValueError("the Nakajima-Tanaka corrections are not active for these inputs (pydisort.py:375)")
    tau = np.atleast_1d(np.asarray(tau, float))
    phi = np.atleast_1d(np.asarray(phi, float))
    lay = [int(np.argmax(t <= tau_arr)) for t in tau]

    mu = [F(x) for x in quadrature_nodes(N)]
    mu0, phi0, I0_4pi = F(kw["mu0"]), F(kw["phi0"]), F(kw["I0"]) / (4 * mp.pi)
    ta = [F(x) for x in tau_arr]
    om = [F(x) for x in omega64]
    f = [F(x) for x in f64]
    leg = [[F(x) for x in row] for row in leg64]
    one = mp.mpf(1)
    sc = [one - om[r] * f[r] for r in range(L)]  # :318-323
    ts0 = [mp.mpf(0)]
    for r in range(L):
        ts0.append(ts0[r] + sc[r] * (ta[r] - (ta[r - 1] if r else 0)))
    # per layer: the coefficients of  p_true / (1 - f) - p_trun  (:428-449), times omega* I0 / 4 pi
    coef = {}
    for l in set(lay):
        oms = (one - f[l]) / sc[l] * om[l]
        c = [(2 * k + 1) * leg[l][k] / (one - f[l]) for k in range(nall)]
        for k in range(NLeg):
            c[k] -= (2 * k + 1) * (leg[l][k] - f[l]) / (one - f[l])
        coef[l] = [oms * I0_4pi * v for v in c]
    # IMS constants (:601-611)
    sum1 = sum(om[r] * ta[r] for r in range(L))
    omega_avg = sum1 / sum(ta)
    sum2 = sum(f[r] * om[r] * ta[r] for r in range(L))
    f_avg = sum2 / sum1
    ravg = []
    for k in range(nall):
        ravg.append(sum((f[r] if k < NLeg else leg[r][k]) * om[r] * ta[r] for r in range(L)) / sum2)
    of = omega_avg * f_avg
    smu0 = mu0 / (one - of)
    ims_coef = [I0_4pi * of**2 / (one - of) * (2 * k + 1) * (2 * ravg[k] - ravg[k] ** 2) for k in range(nall)]

    s0 = mp.sqrt(one - mu0 * mu0)
    out = {o: np.zeros((NQuad, len(tau), len(phi))) for o in ORDERS}
    for i in range(N):
        m = mu[i]
        si = mp.sqrt(one - m * m)
        x = one / m - one / smu0
        for p in range(len(phi)):
            cs = mp.cos(phi0 - F(phi[p]))
            # cosine of the angle between the stream (+-mu, phi) and the beam (-mu0, phi0)  (subroutines.py:85-112)
            P_up = _legendre_values(nall, -mu0 * m + s0 * si * cs)
            P_dn = _legendre_values(nall, mu0 * m + s0 * si * cs)
            ims_series = _dot(ims_coef, P_dn)
            B = {l: (mu0 / (mu0 + m) * _dot(c, P_up), mu0 / (mu0 - m) * _dot(c, P_dn)) for l, c in coef.items()}
            for t in range(len(tau)):
                l = lay[t]
                tt = F(tau[t])
                ts = ts0[l + 1] - (ta[l] - tt) * sc[l]  # :419-421
                att = mp.exp(-ts / mu0)
                E = lambda v: mp.exp(-v / mu0 - (v - ts) / m)  # noqa: E731
                D = lambda v: mp.exp(-v / mu0 - (ts - v) / m)  # noqa: E731
                eb, et = E(ts0[l + 1]), D(ts0[l])
                rate = sc[l] / m
                up = dict(value=att - eb, antiderivative=att / (-sc[l] / mu0) - eb / rate,
                          derivative=att * (-sc[l] / mu0) - eb * rate)
                dn = dict(value=att - et, antiderivative=att / (-sc[l] / mu0) + et / rate,
                          derivative=att * (-sc[l] / mu0) + et * rate)
                for r in range(l + 1, L):
                    seg = E(ts0[r]) - E(ts0[r + 1])
                    up["value"] += seg
                    up["antiderivative"] += seg * m / sc[r]
                    up["derivative"] += seg * rate
                for r in range(l):
                    seg = D(ts0[r + 1]) - D(ts0[r])
                    dn["value"] += seg
                    dn["antiderivative"] -= seg * m / sc[r]
                    dn["derivative"] -= seg * rate
                e0, e1 = mp.exp(-tt / smu0), mp.exp(-tt / m)
                chi = dict(value=((tt - one / x) * e0 + e1 / x) / (m * smu0 * x),  # :625-628
                           antiderivative=((smu0 - x * smu0 * (smu0 + tt)) * e0 - m * e1) / (m * smu0 * x * x),  # :619-623
                           derivative=((one - (tt - one / x) / smu0) * e0 - e1 / (m * x)) / (m * smu0 * x))
                for o in ORDERS:
                    out[o][i, t, p] = float(B[l][0] * up[o])
                    out[o][N + i, t, p] = float(B[l][1] * dn[o] + ims_series * chi[o])
    return out
