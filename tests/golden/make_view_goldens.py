#!/usr/bin/env python3
"""Radiances at user polar angles of the REFERENCE (needs the reference importable: maker only).

Per case of tests/view_cases.py: one ``pydisort`` call of the reference, its ``subroutines.interpolate(u)(mu, tau, phi)`` and
``interpolate(u0)(mu, tau)`` (subroutines.py:614-705) at the angles view_cases.mu_list (1, a node, the float next above a node,
0.37, +0.0, -0.62, a negated node, -1), at tau = 0, every interface and two interior depths, and two azimuths, as values and as
tau-antiderivatives.  Stored: the inputs that identify the case (tau_arr, omega_arr, mu0, I0, f_arr, NQuad), the points (mu, tau,
phi), and u_mu [nmu, ntau, nphi], u0_mu [nmu, ntau] with the suffix ".antider" for the antiderivatives (not for
view_cases.VALUE_ONLY).  Output: tests/golden/view/<case>.npz (data only).

Usage:  PYTHONDONTWRITEBYTECODE=1 PYTHONICDISORT_SRC=<reference checkout>/src python3 tests/golden/make_view_goldens.py [case ...]
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
import view_cases as V  # noqa: E402


def make_case(name, kw):
    kw = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    tau, mu = V.points(kw), V.mu_list(V.nodes(kw["NQuad"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = PythonicDISORT.pydisort(**kw)
    u_at, u0_at = subroutines.interpolate(res[4]), subroutines.interpolate(res[3])
    store = dict(mu=mu, tau=tau, phi=V.PHI, tau_arr=np.asarray(kw["tau_arr"], float), omega_arr=np.asarray(kw["omega_arr"], float),
                 f_arr=np.asarray(kw["f_arr"], float), mu0=np.array(kw["mu0"]), I0=np.array(kw["I0"]), NQuad=np.array(kw["NQuad"]))
    for suffix, antider in (("", False), (".antider", True)):
        if antider and name in V.VALUE_ONLY:
            continue
        store["u_mu" + suffix] = np.asarray(u_at(mu, tau, V.PHI, antider), float).reshape(len(mu), len(tau), len(V.PHI))
        store["u0_mu" + suffix] = np.asarray(u0_at(mu, tau, antider), float).reshape(len(mu), len(tau))
    np.savez_compressed(os.path.join(V.GOLDEN_DIR, name + ".npz"), **store)
    print(f"{name:20s} {len(mu)} angles x {len(tau)} depths  max u_mu {np.max(np.abs(store['u_mu'])):.4f}", flush=True)


if __name__ == "__main__":
    os.makedirs(V.GOLDEN_DIR, exist_ok=True)
    todo = V.cases()
    for case in (sys.argv[1:] or todo):
        make_case(case, todo[case])
