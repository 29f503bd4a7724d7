#!/usr/bin/env python3
"""Actinic fluxes of the REFERENCE (needs the reference importable: maker only).

Per case of tests/actinic_cases.py: one ``pydisort`` call of the reference, its ``generate_diff_act_flux_funcs(u0)``
(subroutines.py:258-318) evaluated at tau = 0, every interface, the middle of every layer and the bottom, as values and as
tau-antiderivatives.  Stored: the inputs that identify the case (tau_arr, omega_arr, mu0, I0, f_arr), the points, and
flux_act_up / flux_act_down_diffuse [ntau] with the suffix ".antider" for the antiderivatives (not for actinic_cases.VALUE_ONLY).
Output: tests/golden/actinic/<case>.npz (data only).

Usage:  PYTHONDONTWRITEBYTECODE=1 PYTHONICDISORT_SRC=<reference checkout>/src python3 tests/golden/make_actinic_goldens.py [case ...]
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
import actinic_cases as A  # noqa: E402


def make_case(name, kw):
    kw = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    tau = A.points(kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = PythonicDISORT.pydisort(**kw)
    up, down = subroutines.generate_diff_act_flux_funcs(res[3])
    store = dict(tau=tau, tau_arr=np.asarray(kw["tau_arr"], float), omega_arr=np.asarray(kw["omega_arr"], float),
                 f_arr=np.asarray(kw["f_arr"], float), mu0=np.array(kw["mu0"]), I0=np.array(kw["I0"]), NQuad=np.array(kw["NQuad"]))
    for suffix, antider in (("", False), (".antider", True)):
        if antider and name in A.VALUE_ONLY:
            continue
        store["flux_act_up" + suffix] = np.asarray(up(tau, antider), float).reshape(len(tau))
        store["flux_act_down_diffuse" + suffix] = np.asarray(down(tau, antider), float).reshape(len(tau))
    np.savez_compressed(os.path.join(A.GOLDEN_DIR, name + ".npz"), **store)
    print(f"{name:20s} {len(tau):3d} points  max act_up {np.max(np.abs(store['flux_act_up'])):.4f}", flush=True)


if __name__ == "__main__":
    os.makedirs(A.GOLDEN_DIR, exist_ok=True)
    todo = A.cases()
    for case in (sys.argv[1:] or todo):
        make_case(case, todo[case])
