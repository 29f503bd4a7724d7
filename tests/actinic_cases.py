"""The cases of the actinic-flux fixtures (tests/golden/actinic/*.npz) and the test-side truth of the actinic fluxes, shared by
the maker (tests/golden/make_actinic_goldens.py), the CPU test that pins the truth to the reference (tests/test_actinic_cpu.py) and
the GPU tests (tests/test_gpu_actinic.py).

Truth: the CPU oracle's u0 (value, tau-antiderivative, tau-derivative) and the closed forms of include/rtd.h
(rtd_plan_fetch_actinic) in NumPy, with the CALLER's I0:

    act_up           = 2 pi sum_{i<N} w_i u0_i
    act_down_diffuse = 2 pi sum_{i<N} w_i u0_{N+i} + R
    act_down_direct  = D
    value:          R = I0 e^(-tau*/mu0) - I0 e^(-tau/mu0)                       D = I0 e^(-tau/mu0)
    antiderivative: R = I0 e^(-tau*/mu0) / (-sc/mu0) - I0 e^(-tau/mu0) (-mu0)    D = I0 e^(-tau/mu0) (-mu0)
    derivative:     R = I0 e^(-tau*/mu0) (-sc/mu0) - I0 e^(-tau/mu0) / (-mu0)    D = I0 e^(-tau/mu0) / (-mu0)

The reference (generate_diff_act_flux_funcs, subroutines.py:258-318) forms R with the I0 it has divided by its rescale factor and
does not multiply back; in every fixture but "rescaled" the largest source is I0 = 1 (or there is no beam), so the two agree."""
import os
import warnings
from math import pi

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "actinic")
ORDERS = (0, -1, 1)  # value, tau-antiderivative, tau-derivative
KEYS = ("flux_act_up", "flux_act_down_diffuse", "flux_act_down_direct")


def hg_column(L, NQuad, g=0.75, delta_m=True, seed=0, **extra):
    """A Henyey-Greenstein column: NLeg = NQuad of NQuad + 3 moments, f_arr = moment NLeg (or 0 in every layer)."""
    rng = np.random.default_rng(1000 * L + NQuad + seed)
    nleg_all = NQuad + 3
    leg = np.tile(g ** np.arange(nleg_all), (L, 1))
    kw = dict(tau_arr=np.cumsum(rng.uniform(0.2, 0.9, L)), omega_arr=rng.uniform(0.6, 0.97, L), NQuad=NQuad, Leg_coeffs_all=leg,
              mu0=float(rng.uniform(0.35, 0.9)), I0=1.0, phi0=0.0, NLeg=NQuad, f_arr=np.full(L, g ** NQuad if delta_m else 0.0),
              only_flux=True)
    kw.update(extra)
    return kw


def cases():
    """name -> keyword arguments of the one-column ``pydisort`` (the reference's, the oracle's and this project's alike)."""
    return {
        "L1_q6": hg_column(1, 6),
        "L3_q16": hg_column(3, 16),
        "L6_q34": hg_column(6, 34),
        "L6_q6": hg_column(6, 6, g=0.6),
        "L3_q16_no_deltam": hg_column(3, 16, delta_m=False),
        "L3_q16_thermal": hg_column(3, 16, seed=1, s_poly_coeffs=np.array([[0.30, 0.10], [0.42, 0.05], [0.20, 0.12]])),
        "L3_q16_lambert": hg_column(3, 16, seed=2, BDRF_Fourier_modes=[0.35]),
        "L3_q6_no_beam": hg_column(3, 6, seed=3, I0=0.0, b_neg=1.0, b_pos=0.4),
        "rescaled": hg_column(3, 16, seed=4, I0=2.5, b_pos=0.1),
    }


# Fixtures that hold values only, because the reference's own u0 antiderivative is not one there:
#  * thermal: the antiderivative of the thermal particular solution divides by the whole scale_tau array instead of the point's
#    layer (subroutines.py:815) and does not evaluate for several layers;
#  * no beam: the antiderivative branch of u0 is taken only when there is a beam source (_assemble_intensity_and_fluxes.py:382),
#    so without one the closure returns the VALUE whatever the flag says.
VALUE_ONLY = ("L3_q16_thermal", "L3_q6_no_beam")
RESCALED = ("rescaled",)  # the cases whose rescale factor is not 1: the reference's R is low by R (1 - 1 / rescale) there


def points(kw):
    """tau = 0, every interface, the middle of every layer, the bottom."""
    edges = np.concatenate(([0.0], np.asarray(kw["tau_arr"], float)))
    return np.sort(np.concatenate((edges, 0.5 * (edges[:-1] + edges[1:]))))


def reclassification(p, I0, tau, order):
    """(R, D) of the closed forms above for the oracle's prepared column p (oracle.disort_oracle.prepare) and the caller's I0."""
    tau = np.atleast_1d(np.asarray(tau, float))
    if not I0 > 0:
        return np.zeros(len(tau)), np.zeros(len(tau))
    l = np.argmax(tau[:, None] <= p["tau"][None, :], axis=1)
    sc, mu0 = p["scale_tau"][l], p["mu0"]
    ts = p["tau_s0"][1:][l] - (p["tau"][l] - tau) * sc
    es, ed = I0 * np.exp(-ts / mu0), I0 * np.exp(-tau / mu0)
    if order < 0:
        es, ed = es / (-sc / mu0), ed * (-mu0)
    elif order > 0:
        es, ed = es * (-sc / mu0), ed / (-mu0)
    return es - ed, ed


def truth(kw, tau, order=0, sol=None):
    """The three actinic fluxes of one column at tau [ntau >= 2] -> dict of [ntau] arrays; `sol`: an oracle Solution of kw to
    reuse."""
    if sol is None:
        sol = solve(kw)
    p, N = sol.p, sol.p["N"]
    x = np.asarray(sol.u0(tau, order < 0, is_derivative_wrt_tau=order > 0), float).reshape(2 * N, -1)
    R, D = reclassification(p, float(kw["I0"]), tau, order)
    return dict(flux_act_up=2 * pi * (p["W"] @ x[:N]), flux_act_down_diffuse=2 * pi * (p["W"] @ x[N:]) + R, flux_act_down_direct=D)


def solve(kw):
    """The oracle's Solution of one column."""
    from oracle import disort_oracle as O
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return O.Solution(O.prepare(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}))


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
