#!/usr/bin/env python3
"""40-digit arbiter of the Nakajima-Tanaka corrections (TMS + IMS) at ARBITRARY polar-angle cosines: tools/nt_truth.py evaluates
them at the quadrature nodes only; this is the same closed form of the inputs of one ``pydisort`` call (pydisort.py:409-638) with
the stream's cosine left free.  It shares no code with oracle/ or the package (only nt_truth's node finder and Legendre helper).

A viewing angle routinely is a special value of the formulas as the reference writes them: mu = -mu0 makes mu0 / (mu0 - |mu|)
infinite against a vanishing attenuation difference, |mu| = the IMS scaled mu0 makes chi 0 / 0.  Two forms are therefore given:

    form="divided" (the truth)   every such quotient is written as a divided difference with its limit taken explicitly:
        mu0 / (mu0 - a) (e^{-D/mu0} - e^{-D/a}) = (D / a) phi1(z) e^{-D/mu0},  z = D (1/a - 1/mu0),  phi1(z) = (1 - e^{-z}) / z,  phi1(0) = 1
        chi = e^{-tau/s} tau^2 psi2(tau x) / (a s),  x = 1/a - 1/s,  psi2(z) = (e^{-z} - 1 + z) / z^2,  psi2(0) = 1/2
      and the tau-derivative / -antiderivative follow from these (the comments at each line).  psi2 takes its series below |z| = 1e-8,
      where the closed form would spend 16 of the working digits; above it spends at most 8.
    form="plain"                 the reference's quotients as they stand (nt_truth's, with mu free): raises ZeroDivisionError at
      mu = -mu0.  It is what the divided form is checked against: at the nodes the two agree to 1e-30 and reproduce tests/golden/nt,
      and at mu = -mu0 the divided form agrees to 1e-25 with the mean of the plain form at -mu0 (1 +- 2^-60) in 80 digits
      (tests/test_nt_view_truth_cpu.py).

    truth = nt_view_truth.correction(kw, mu, tau, phi)   # -> dict(value=, antiderivative=, derivative=), each [nmu, ntau, nphi]

in the units of ``I0``.  mu > 0 looks up (TMS only), mu < 0 down (TMS + IMS); mu = 0 is refused.  ``terms`` returns the unrounded
mpmath numbers and takes mpmath angles.
"""
import numpy as np
import mpmath as mp

import nt_truth

DPS = 40
ORDERS = nt_truth.ORDERS
PROVENANCE = "40-digit closed form at the angles (tools/nt_view_truth.py)"


def _phi1(z):
    return mp.mpf(1) if z == 0 else -mp.expm1(-z) / z


def _psi2(z):
    if z == 0:
        return mp.mpf(1) / 2
    if abs(z) < mp.mpf("1e-8"):  # sum_k (-z)^k / (k + 2)!: the term k = 10 is below 1e-80 / 12!
        return sum((-z) ** k / mp.factorial(k + 2) for k in range(10))
    return (mp.expm1(-z) + z) / (z * z)


def terms(kw, mu, tau, phi, form="divided", dps=DPS):
    """-> {order: [nmu][ntau][nphi] of mpf}.  mu may hold floats or mpf (each is taken as exact)."""
    if form not in ("divided", "plain"):
        raise ValueError(form)
    with mp.workdps(dps):
        return _terms(kw, mu, tau, phi, form == "divided")


def correction(kw, mu, tau, phi):
    """The truth rounded to float64 -> {order: array [nmu, ntau, nphi]}."""
    t = terms(kw, np.atleast_1d(np.asarray(mu, float)), tau, phi)
    return {o: np.array([[[float(v) for v in row] for row in plane] for plane in t[o]]) for o in ORDERS}


def _terms(kw, mu, tau, phi, divided):
    F = lambda v: v if isinstance(v, mp.mpf) else mp.mpf(float(v))  # noqa: E731
    tau_arr = np.atleast_1d(np.asarray(kw["tau_arr"], float))
    L = len(tau_arr)
    omega64 = np.broadcast_to(np.asarray(kw["omega_arr"], float), (L,))
    f64 = np.broadcast_to(np.asarray(kw.get("f_arr", 0), float), (L,))
    leg64 = np.atleast_2d(np.asarray(kw["Leg_coeffs_all"], float))
    NQuad = int(kw["NQuad"])
    NLeg = NQuad if kw.get("NLeg") is None else int(kw["NLeg"])
    nall = leg64.shape[1]
    if not (np.any(f64 > 0) and NLeg < nall and np.any(omega64 > 0) and float(kw["I0"]) > 0):
        raise ValueError("the Nakajima-Tanaka corrections are not active for these inputs (pydisort.py:375)")
    tau = np.atleast_1d(np.asarray(tau, float))
    phi = np.atleast_1d(np.asarray(phi, float))
    lay = [int(np.argmax(t <= tau_arr)) for t in tau]
    mus = [F(m) for m in mu]
    if any(m == 0 or abs(m) > 1 for m in mus):
        raise ValueError("mu must be non-zero and within [-1, 1]")

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
    coef = {}  # per layer: the coefficients of  p_true / (1 - f) - p_trun  (:428-449), times omega* I0 / 4 pi
    for l in set(lay):
        oms = (one - f[l]) / sc[l] * om[l]
        c = [(2 * k + 1) * leg[l][k] / (one - f[l]) for k in range(nall)]
        for k in range(NLeg):
            c[k] -= (2 * k + 1) * (leg[l][k] - f[l]) / (one - f[l])
        coef[l] = [oms * I0_4pi * v for v in c]
    sum1 = sum(om[r] * ta[r] for r in range(L))  # IMS constants (:601-611)
    omega_avg = sum1 / sum(ta)
    sum2 = sum(f[r] * om[r] * ta[r] for r in range(L))
    f_avg = sum2 / sum1
    ravg = [sum((f[r] if k < NLeg else leg[r][k]) * om[r] * ta[r] for r in range(L)) / sum2 for k in range(nall)]
    of = omega_avg * f_avg
    smu0 = mu0 / (one - of)
    ims_coef = [I0_4pi * of**2 / (one - of) * (2 * k + 1) * (2 * ravg[k] - ravg[k] ** 2) for k in range(nall)]

    s0 = mp.sqrt(one - mu0 * mu0)
    out = {o: [[[None] * len(phi) for _ in tau] for _ in mus] for o in ORDERS}
    for i, m in enumerate(mus):
        up, a = m > 0, abs(m)
        si = mp.sqrt(one - a * a)
        for p in range(len(phi)):
            # cosine of the angle between the direction (m, phi) and the beam (-mu0, phi0)  (subroutines.py:85-112)
            P = nt_truth._legendre_values(nall, -mu0 * m + s0 * si * mp.cos(phi0 - F(phi[p])))
            ims_series = mp.mpf(0) if up else nt_truth._dot(ims_coef, P)
            series = {l: nt_truth._dot(c, P) for l, c in coef.items()}
            for t in range(len(tau)):
                l = lay[t]
                tt = F(tau[t])
                ts = ts0[l + 1] - (ta[l] - tt) * sc[l]  # :419-421
                if up:
                    fac = _up(a, mu0, ts, ts0, sc, l, L)
                elif divided:
                    fac = _down_divided(a, mu0, ts, ts0, sc, l)
                else:
                    fac = _down_plain(a, mu0, ts, ts0, sc, l)
                chi = dict.fromkeys(ORDERS, mp.mpf(0)) if up else (_chi_divided if divided else _chi_plain)(a, smu0, tt)
                for o in ORDERS:
                    out[o][i][t][p] = series[l] * fac[o] + ims_series * chi[o]
    return out


def _up(m, mu0, ts, ts0, sc, l, L):
    """mu0 / (mu0 + m) times the attenuation differences of an upward stream: nothing is special here."""
    att = mp.exp(-ts / mu0)
    E = lambda v: mp.exp(-v / mu0 - (v - ts) / m)  # noqa: E731
    eb, rate = E(ts0[l + 1]), sc[l] / m
    up = dict(value=att - eb, antiderivative=att / (-sc[l] / mu0) - eb / rate, derivative=att * (-sc[l] / mu0) - eb * rate)
    for r in range(l + 1, L):
        seg = E(ts0[r]) - E(ts0[r + 1])
        up["value"] += seg
        up["antiderivative"] += seg * m / sc[r]
        up["derivative"] += seg * rate
    return {o: mu0 / (mu0 + m) * v for o, v in up.items()}


def _down_plain(m, mu0, ts, ts0, sc, l):
    att = mp.exp(-ts / mu0)
    D = lambda v: mp.exp(-v / mu0 - (ts - v) / m)  # noqa: E731
    et, rate = D(ts0[l]), sc[l] / m
    dn = dict(value=att - et, antiderivative=att / (-sc[l] / mu0) + et / rate, derivative=att * (-sc[l] / mu0) + et * rate)
    for r in range(l):
        seg = D(ts0[r + 1]) - D(ts0[r])
        dn["value"] += seg
        dn["antiderivative"] -= seg * m / sc[r]
        dn["derivative"] -= seg * rate
    return {o: mu0 / (mu0 - m) * v for o, v in dn.items()}  # ZeroDivisionError at m = mu0


def _down_divided(m, mu0, ts, ts0, sc, l):
    def H(top, depth):
        """mu0 / (mu0 - m) (e^{-(top + depth)/mu0} - e^{-top/mu0 - depth/m}): the attenuation difference over a segment of scaled
        thickness `depth` whose top lies at `top`, as seen from the segment's bottom."""
        z = depth * (1 / m - 1 / mu0)
        return (depth / m) * _phi1(z) * mp.exp(-(top + depth) / mu0)

    att = mp.exp(-ts / mu0)
    et = mp.exp(-ts0[l] / mu0 - (ts - ts0[l]) / m)
    h = H(ts0[l], ts - ts0[l])
    dn = dict(value=h,
              # mu0 / (mu0 - m) (-mu0 att + m et) / sc:  -mu0 att + m et = -m (att - et) - (mu0 - m) att
              antiderivative=-(m * h + mu0 * att) / sc[l],
              # mu0 / (mu0 - m) (-att / mu0 + et / m) sc:  the bracket = (att - et) (-1 / mu0) + et (1 / m - 1 / mu0)
              derivative=sc[l] * (et / m - h / mu0))
    for r in range(l):
        seg = H(ts0[r], ts0[r + 1] - ts0[r]) * mp.exp(-(ts - ts0[r + 1]) / m)
        dn["value"] += seg
        dn["antiderivative"] -= seg * m / sc[r]
        dn["derivative"] -= seg * sc[l] / m
    return dn


def _chi_plain(m, smu0, tt):
    one = mp.mpf(1)
    x = one / m - one / smu0
    e0, e1 = mp.exp(-tt / smu0), mp.exp(-tt / m)
    return dict(value=((tt - one / x) * e0 + e1 / x) / (m * smu0 * x),  # :625-628
                antiderivative=((smu0 - x * smu0 * (smu0 + tt)) * e0 - m * e1) / (m * smu0 * x * x),  # :619-623
                derivative=((one - (tt - one / x) / smu0) * e0 - e1 / (m * x)) / (m * smu0 * x))


def _chi_divided(m, smu0, tt):
    z = tt * (1 / m - 1 / smu0)
    e0 = mp.exp(-tt / smu0)
    psi, ph = e0 * _psi2(z), e0 * _phi1(z)
    return dict(value=tt * tt * psi / (m * smu0),
                # (:619-623) e0 (smu0 - x smu0 (smu0 + tau)) - m e1 with m = smu0 / (1 + x smu0), collected in powers of x
                antiderivative=-(tt * tt * psi / smu0 + e0 * (smu0 + tt)),
                # d/dtau of the value: e0' = -e0 / smu0,  d(z^2 psi2)/dz = 1 - e^{-z} = z phi1
                derivative=(-tt * tt * psi / smu0 + tt * ph) / (m * smu0))
