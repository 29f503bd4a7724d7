"""Exact values and derived error bounds of the device-formed Nakajima-Tanaka inputs (csrc/rtd_nt_prep.h), shared by
tests/test_nt_prep_cpu.py (the routines on the host) and tests/test_gpu_nt_device.py (the kernels, through Plan.get_nt).

Every float64 input is taken as exact (fractions.Fraction), pi is the float64 M_PI the code multiplies by.  With u = 2^-53 and
gamma_n = n u / (1 - n u) the bounds follow from the loops AS WRITTEN in rtd_nt_ims_lane (a fused multiply-add only removes a
rounding, so they hold with and without contraction):

 r_k   num^ = sum_l resid_l w_l (1 + th_l): one rounding for w_l = omega_l tau_l, one for the product, at most L - 1 additions, so
       |th_l| <= gamma_{L+1} and |num^ - num| <= gamma_{L+1} A_k with A_k = sum_l |resid_l w_l|.  den^ = D (1 + th), D = sum f w,
       |th| <= gamma_{L+1} (all terms >= 0).  One division.  Hence
           |r^ - r| <= [gamma_{L+1} A (1 + u) + |num| (u + gamma_{L+1})] / (D (1 - gamma_{L+1})) <= gamma_{2L+4} A_k / D =: dr
       (|num| <= A_k).
 coef  h(r) = 2 r - r^2, h(r^) - h(r) = (r^ - r)(2 - r^ - r): at most dr (2 |1 - r| + dr).  Evaluating h(r^) rounds r^ r^, the
       difference and the product with 2k + 1 (2 r^ and 2k + 1 are exact): at most gamma_3 (r^2 + |h|) <= gamma_4 (2 |r| + 2 r^2)
       in terms of the exact r.  Hence  |coef^ - coef| <= (2k + 1) [dr (2 |1 - r| + dr) + gamma_4 (2 |r| + 2 r^2)].
 par   of = (sw / st)(sfw / sw): the rounded sw divides out EXACTLY, what remains is sfw (gamma_{L+1}), st (gamma_{L-1}), two
       divisions and one product: |of^ - of| <= gamma_{2L+3} of.  1 - of^ then carries gamma_{2L+3} of / (1 - of) + u relative, and
           scaled mu0 = mu0 / (1 - of):                    relative error <= gamma_{2L+6} / (1 - of)
           amplitude = I0 / (4 pi) (of of) / (1 - of):     2 gamma_{2L+3} + gamma_{2L+3} of / (1 - of) + 5 u <= 2 gamma_{2L+6} / (1 - of)
       (first order; the tests assert that gamma_{2L+6} / (1 - of) < 2^-30, where the second-order terms are below one part in 2^30
       of the bound and the step from 2L+5 to 2L+6 covers them).
 wfull (2k + 1) g is one rounding of an exact product: the correctly rounded value, bit for bit.
 mix   t_s = omega_s dtau_s (one rounding), sca = sum t_s (S - 1 additions, terms >= 0), num = sum t_s leg_s (one more rounding each),
       one division: |g^ - g| <= gamma_{2S+3} sum_s |t_s leg_s| / sca, by the argument of r_k.  Moment 0 is exactly 1, a layer
       without a scatterer exactly (1, 0, ...).
A column with D = 0 has ims_coef = 0, amplitude 0, scaled mu0 = mu0, all exact."""
import math
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
F = lambda v: Fraction(float(v))  # noqa: E731
PI = Fraction(math.pi)


NLEG, NALL = 8, 12


def columns(L, seed, C=4):
    """C columns of L layers, NALL moments of which NLEG are used; high moments of both signs; the last column has f = 0 everywhere."""
    rng = np.random.default_rng([77, L, seed])
    tau = np.cumsum(rng.uniform(0.05, 2.0, (C, L)), axis=1)
    omega = rng.uniform(0.05, 0.999, (C, L))
    leg = rng.uniform(0.2, 0.95, (C, L, 1)) ** np.arange(NALL)[None, None, :]
    leg[:, :, NLEG:] *= rng.choice([-1.0, 1.0], (C, L, NALL - NLEG)) * rng.uniform(0.1, 1.0, (C, L, NALL - NLEG))
    f = np.abs(leg[:, :, NLEG]).copy()
    f[-1] = 0.0
    return dict(tau=tau, omega=omega, f=f, leg=leg, mu0=rng.uniform(0.2, 1.0, C), I0=rng.uniform(0.3, 3.0, C))


def gamma(n):
    return n * U / (1 - n * U)


def exact_ims(tau, omega, f, leg, nleg, mu0, I0):
    """One column: tau, omega, f [L], leg [L][nleg_all] -> (coef [nleg_all], par [2], coef bounds, par bounds), all Fractions."""
    L, nall = len(tau), len(leg[0])
    w = [F(omega[l]) * F(tau[l]) for l in range(L)]
    sw, st = sum(w), sum(F(t) for t in tau)
    D = sum(F(f[l]) * w[l] for l in range(L))
    if D == 0:
        return [Fraction(0)] * nall, [F(mu0), Fraction(0)], [Fraction(0)] * nall, [Fraction(0), Fraction(0)]
    coef, cb = [], []
    for k in range(nall):
        terms = [(F(f[l]) if k < nleg else F(leg[l][k])) * w[l] for l in range(L)]
        r, A = sum(terms) / D, sum(abs(t) for t in terms)
        dr = gamma(2 * L + 4) * A / D
        coef.append((2 * k + 1) * (2 * r - r * r))
        cb.append((2 * k + 1) * (dr * (2 * abs(1 - r) + dr) + gamma(4) * (2 * abs(r) + 2 * r * r)))
    of = (sw / st) * (D / sw)
    rel = gamma(2 * L + 6) / (1 - of)
    assert rel < Fraction(1, 2 ** 30)
    par = [F(mu0) / (1 - of), F(I0) / (4 * PI) * of * of / (1 - of)]
    return coef, par, cb, [rel * abs(par[0]), 2 * rel * abs(par[1])]


def hold_ims(got_coef, got_par, tau, omega, f, leg, nleg, mu0, I0):
    """Asserts one column against its exact values; returns the worst error over bound (0 where the bound is 0 and met)."""
    coef, par, cb, pb = exact_ims(tau, omega, f, leg, nleg, mu0, I0)
    worst = 0.0
    for got, want, bound in list(zip(got_coef, coef, cb)) + list(zip(got_par, par, pb)):
        err = abs(F(got) - want)
        assert err <= bound, (float(got), float(want), float(err), float(bound))
        if bound > 0:
            worst = max(worst, float(err / bound))
    return worst


def hold_wfull(got, leg):
    """got [L][nleg_all] == the correctly rounded (2k + 1) leg, bit for bit."""
    for l, row in enumerate(leg):
        for k, g in enumerate(row):
            assert float(got[l][k]) == float((2 * k + 1) * F(g)), (l, k)


def exact_mix(dt, om, lspec, k):
    """One (profile, layer): dt, om [S], lspec [S][nleg_all] -> (moment k, bound)."""
    S = len(dt)
    t = [F(om[s]) * F(dt[s]) for s in range(S)]
    sca = sum(t)
    if k == 0:
        return Fraction(1), Fraction(0)
    if sca == 0:
        return Fraction(0), Fraction(0)
    terms = [t[s] * F(lspec[s][k]) for s in range(S)]
    return sum(terms) / sca, gamma(2 * S + 3) * sum(abs(v) for v in terms) / sca
