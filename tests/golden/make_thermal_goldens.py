#!/usr/bin/env python3
"""Generator of tests/golden/thermal/*.npz: thermal problems stated by temperatures, solved by the REFERENCE.

Run with the reference package on PYTHONPATH (its src/ directory) and PYTHONDONTWRITEBYTECODE=1:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference>/src python tests/golden/make_thermal_goldens.py

Each case builds s_poly_coeffs, b_pos and b_neg with the reference's own helpers (generate_s_poly_coeffs,
blackbody_contrib_to_BCs with epsrel=1e-13 passed through to SciPy's quadrature; the emissivity of case 9c as its test states
it, 1 - albedo), calls the reference's pydisort and stores
  * the temperature-level description: TEMPER, WVNMLO, WVNMHI, BTEMP, TTEMP, TEMIS, and what the caller adds to the boundary
    terms on top of the emission (b_pos_add, b_neg_add);
  * every other argument of pydisort as arrays (the BDRF as the tabulated zeroth mode q0 on the quadrature grid and at mu0);
  * u, u0 and the three fluxes at all interfaces plus the mid-layers, phi in {0, pi/2, pi, 2.5}.
Data only; tests/test_gpu_thermal_batch.py feeds the first two groups to pydisort_batch(thermal=...) and compares with the third.
"""
import os
from math import pi

import numpy as np
import PythonicDISORT
from PythonicDISORT.subroutines import blackbody_contrib_to_BCs, generate_s_poly_coeffs

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "thermal")
EPS = dict(epsrel=1e-13)
PHI = np.array([0.0, pi / 2, pi, 2.5])


def cases():
    # TP7a (pydisotest/7_test.py:15): one layer, 16 streams, no beam, no boundary emission
    yield "7a", dict(tau_arr=np.array([1.0]), omega_arr=np.array([0.1]), NQuad=16, Leg=0.05 ** np.arange(17)[None, :],
                     mu0=0.0, I0=0.0, phi0=0.0, f_arr=np.array([0.0]), TEMPER=np.array([200.0, 300.0]), WVNMLO=300.0, WVNMHI=800.0,
                     BTEMP=None, TTEMP=None, TEMIS=1.0, b_pos_add=0.0, b_neg_add=0.0, albedo=None)
    # TP7c (:173) without the Nakajima-Tanaka corrections: beam, delta-M scaling, both boundaries emit, b_neg + 100
    leg = 0.8 ** np.arange(24)
    yield "7c", dict(tau_arr=np.array([1.0]), omega_arr=np.array([0.5]), NQuad=12, Leg=leg[None, :], mu0=0.5, I0=200.0, phi0=0.0,
                     f_arr=np.array([leg[12]]), TEMPER=np.array([300.0, 200.0]), WVNMLO=0.0, WVNMHI=80000.0, BTEMP=320.0,
                     TTEMP=100.0, TEMIS=1.0, b_pos_add=0.0, b_neg_add=100.0, albedo=None)
    # TP9c (pydisotest/9_test.py:171): six layers, 8 streams, beam, Lambertian surface of albedo 0.5, b_neg + 1
    layer = np.arange(1.0, 7.0)
    yield "9c", dict(tau_arr=np.cumsum(layer), omega_arr=np.linspace(0.65, 0.9, 6), NQuad=8,
                     Leg=(layer[:, None] / 7.0) ** np.arange(9)[None, :], mu0=0.5, I0=pi, phi0=0.0,
                     f_arr=np.zeros(6), TEMPER=600.0 + np.arange(7) * 10.0, WVNMLO=999.0, WVNMHI=1000.0, BTEMP=700.0, TTEMP=550.0,
                     TEMIS=1.0, b_pos_add=0.0, b_neg_add=1.0, albedo=0.5)


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, c in cases():
        N = c["NQuad"] // 2
        band = (c["WVNMLO"], c["WVNMHI"])
        s_poly = generate_s_poly_coeffs(c["tau_arr"], c["TEMPER"], *band, **EPS)
        emis = 1.0 if c["albedo"] is None else 1.0 - c["albedo"]
        b_pos = c["b_pos_add"] + (0.0 if c["BTEMP"] is None else emis * float(blackbody_contrib_to_BCs(c["BTEMP"], *band, **EPS)))
        b_neg = c["b_neg_add"] + (0.0 if c["TTEMP"] is None else c["TEMIS"] * float(blackbody_contrib_to_BCs(c["TTEMP"], *band, **EPS)))
        modes = [] if c["albedo"] is None else [lambda mu, neg_mup, a=c["albedo"]: np.full((len(mu), len(neg_mup)), a)]
        mu_arr, flux_up, flux_down, u0, u = PythonicDISORT.pydisort(
            c["tau_arr"], c["omega_arr"], c["NQuad"], c["Leg"] if len(c["tau_arr"]) > 1 else c["Leg"][0], c["mu0"], c["I0"], c["phi0"],
            b_pos=b_pos, b_neg=b_neg, s_poly_coeffs=s_poly, f_arr=c["f_arr"] if len(c["tau_arr"]) > 1 else c["f_arr"][0],
            BDRF_Fourier_modes=modes)
        levels = np.concatenate(([0.0], c["tau_arr"]))
        tau = np.sort(np.concatenate((levels, 0.5 * (levels[1:] + levels[:-1]))))
        fdn = flux_down(tau)
        nan = float("nan")
        np.savez(os.path.join(OUT, name + ".npz"),
                 tau_arr=c["tau_arr"], omega_arr=c["omega_arr"], NQuad=c["NQuad"], Leg_coeffs_all=c["Leg"], mu0=c["mu0"], I0=c["I0"],
                 phi0=c["phi0"], f_arr=c["f_arr"], b_pos_add=c["b_pos_add"], b_neg_add=c["b_neg_add"],
                 bdrf_q=np.zeros((0, N, N)) if c["albedo"] is None else np.full((1, N, N), c["albedo"]),
                 bdrf_q0=np.zeros((0, N)) if c["albedo"] is None else np.full((1, N), c["albedo"]),
                 TEMPER=c["TEMPER"], WVNMLO=c["WVNMLO"], WVNMHI=c["WVNMHI"], BTEMP=nan if c["BTEMP"] is None else c["BTEMP"],
                 TTEMP=nan if c["TTEMP"] is None else c["TTEMP"], TEMIS=c["TEMIS"],
                 ref_s_poly_coeffs=s_poly, ref_b_pos=b_pos, ref_b_neg=b_neg,
                 tau=tau, phi=PHI, mu_arr=mu_arr, u=u(tau, PHI), u0=u0(tau), flux_up=flux_up(tau), flux_down_diffuse=fdn[0],
                 flux_down_direct=fdn[1])
        print(name, "u", u(tau, PHI).shape, "max", float(np.max(np.abs(u(tau, PHI)))))


if __name__ == "__main__":
    main()
