#!/usr/bin/env python3
"""Lambertian surfaces of the REFERENCE, solved directly and as the two parts of the adding formula (needs the reference importable:
maker only).

Per case of tests/lambert_cases.py: for each albedo A of lambert_cases.ALBEDOS the reference's own DIRECT solve with
``BDRF_Fourier_modes=[A]`` and ``b_pos=(1 - A) E``; its solve over a BLACK surface (the case as stated); and its solve of the same
layers without a source, LIT FROM BELOW by unit isotropic intensity (``b_pos=1``, ``I0=0``, ``only_flux=True``).  Each is
evaluated at four depths (0, an interior point, an interface, the bottom) and two azimuths:
  values            u, u0, flux_up, both parts of flux_down, and ``subroutines.interpolate`` of u and u0 at three angles;
  antiderivatives   flux_up and both parts of flux_down (lambert_cases.fields_of).
The reference has these two tau-orders only (it leaves derivatives to autograd), and its u0 and u return the VALUE for
``is_antiderivative_wrt_tau=True`` when there is no beam source (_assemble_intensity_and_fluxes.py: the branch is taken only with
a beam), which is the lit-from-below solve: the antiderivatives of the intensities are therefore not stored.  Its antiderivative of
a thermal source's particular solution evaluates only for as many depths as layers, so the thermal case is stored as values only
(lambert_cases.VALUE_ONLY).  It does not take several depths at once in the antiderivative of flux_down either: everything is
evaluated depth by depth.  tests/test_lambert_cpu.py holds all three tau-orders of every field against the oracle.
Stored: the inputs that identify the case, the points, E, and one array per tau-order and field, "<order>.<field>", whose leading
axis runs over the solves lambert_cases.SOLVES = (black, below, direct0 ... direct3: one per albedo); the lit-from-below solve is
azimuth-independent, its u and u_mu are its u0 and u0_mu repeated over phi.
Output: tests/golden/lambert/<case>.npz (data only).

Usage:  PYTHONDONTWRITEBYTECODE=1 PYTHONICDISORT_SRC=<reference checkout>/src python3 tests/golden/make_lambert_goldens.py [case ...]
"""
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (os.environ.get("PYTHONICDISORT_SRC"), os.path.dirname(HERE), ROOT) if p]
import PythonicDISORT  # noqa: E402
from PythonicDISORT import subroutines  # noqa: E402
import lambert_cases as LC  # noqa: E402


def evaluate(res, tau, mu, into, prefix, orders):
    """The fields of one solve, in the tau-orders `orders`, into the store."""
    flux_up, flux_down, u0 = res[1], res[2], res[3]
    u = res[4] if len(res) > 4 else None
    nphi = len(LC.PHI)
    for order in orders:
        antider = order == "antider"
        key = f"{prefix}.{order}."
        into[key + "flux_up"] = np.array([float(flux_up(t, antider)) for t in tau])
        down = [flux_down(t, antider) for t in tau]
        into[key + "flux_down_diffuse"] = np.array([float(np.squeeze(d[0])) for d in down])
        into[key + "flux_down_direct"] = np.array([float(np.squeeze(d[1])) for d in down])
        if antider:
            continue
        u0_at = subroutines.interpolate(u0)
        into[key + "u0"] = np.stack([np.asarray(u0(t), float).reshape(-1) for t in tau], axis=1)
        into[key + "u0_mu"] = np.stack([np.asarray(u0_at(mu, t), float).reshape(len(mu)) for t in tau], axis=1)
        if u is not None:
            u_at = subroutines.interpolate(u)
            into[key + "u"] = np.stack([np.asarray(u(t, LC.PHI), float).reshape(-1, nphi) for t in tau], axis=1)
            into[key + "u_mu"] = np.stack([np.asarray(u_at(mu, t, LC.PHI), float).reshape(len(mu), nphi) for t in tau], axis=1)
        else:
            into[key + "u"] = np.repeat(into[key + "u0"][..., None], nphi, axis=-1)
            into[key + "u_mu"] = np.repeat(into[key + "u0_mu"][..., None], nphi, axis=-1)


def solve(kw):
    kw = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PythonicDISORT.pydisort(**kw)


def make_case(name, kw, E):
    tau, mu = LC.points(kw), LC.view_mu(kw["NQuad"])
    store = dict(tau=tau, mu=mu, phi=LC.PHI, albedos=np.array(LC.ALBEDOS), E=np.array(E), tau_arr=np.asarray(kw["tau_arr"], float),
                 omega_arr=np.asarray(kw["omega_arr"], float), NQuad=np.array(kw["NQuad"]))
    parts, orders = {}, LC.orders_of(name)
    evaluate(solve(kw), tau, mu, parts, "black", orders)
    evaluate(solve(LC.below_kwargs(kw)), tau, mu, parts, "below", orders)
    for i, A in enumerate(LC.ALBEDOS):
        evaluate(solve(dict(kw, BDRF_Fourier_modes=[A], b_pos=(1.0 - A) * E)), tau, mu, parts, f"direct{i}", orders)
    for order in orders:
        for field in LC.fields_of(order) + ("flux_down_direct",):
            store[f"{order}.{field}"] = np.stack([parts[f"{solve_}.{order}.{field}"] for solve_ in LC.SOLVES])
    path = os.path.join(LC.GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **store)
    F, s = LC.terms(store)
    print(f"{name:16s} F {F:.6f} s {s:.6f} 1/(1-s) {1 / (1 - s):.3f}  {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    os.makedirs(LC.GOLDEN_DIR, exist_ok=True)
    todo = LC.cases()
    for case in (sys.argv[1:] or todo):
        make_case(case, *todo[case])
