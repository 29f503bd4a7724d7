#!/usr/bin/env python3
"""tau-derivatives of the REFERENCE's closures by finite differences (needs the reference importable: maker only).

The reference has no derivative evaluator (it leaves that to autograd), so the fixtures differentiate its own closures
u, u0, flux_up, flux_down with the sixth-order central stencil

    (f(t+3h) - 9 f(t+2h) + 45 f(t+h) - 45 f(t-h) + 9 f(t-2h) - f(t-3h)) / 60h

at two steps, h and h/2.  Stored per case and quantity: the h/2 result D and fd_uncertainty = max|D_h - D_{h/2}| / max|D_{h/2}|
(the absolute max|D_h - D_{h/2}| with `<q>.abs` = 1 when the derivative is identically zero).  h is halved per case while the
discrepancy keeps shrinking; a quantity enters a fixture only with fd_uncertainty <= 5e-9 (deriv_cases.CAP).
Points: three per layer -- mid-layer and 4 h0 inside each end (h0 = 1e-4, the largest step used), so no stencil reaches an
interface; a layer thinner than 8 h0 is left out (at most 10 % of a case's points may be).  phi: deriv_cases.PHI.
One-sided fixtures (deriv_cases.ONE_SIDED): seven-point sixth-order one-sided differences, backward at every interface
tau_arr[l] (the layer that ends there), forward at tau = 0; cap 1e-6.
Output: tests/golden/deriv/<case>.npz, tests/golden/deriv/onesided_<case>.npz (data only).

Usage:  PYTHONDONTWRITEBYTECODE=1 PYTHONICDISORT_SRC=<reference checkout>/src python3 tests/golden/make_derivative_goldens.py [case ...]
"""
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (os.environ.get("PYTHONICDISORT_SRC"), os.path.dirname(HERE), os.path.join(ROOT, "pythonic-disort_amd")) if p]
import PythonicDISORT  # noqa: E402
import deriv_cases as D  # noqa: E402

H0 = 1e-4
CENTRAL = ((3, 1.0), (2, -9.0), (1, 45.0), (-1, -45.0), (-2, 9.0), (-3, -1.0))  # / 60 h
FORWARD = (-49 / 20, 6.0, -15 / 2, 20 / 3, -15 / 4, 6 / 5, -1 / 6)               # f(t + k h), k = 0 ... 6, / h
MAX_HALVINGS = 4


def solve(name):
    kw = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in D.case_kwargs(name).items()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PythonicDISORT.pydisort(**kw), np.atleast_1d(np.asarray(kw["tau_arr"], float))


def central(res, tau, h):
    acc = None
    for k, c in CENTRAL:
        f = D.evaluate(res, tau + k * h, D.PHI)
        acc = {q: c * v for q, v in f.items()} if acc is None else {q: acc[q] + c * v for q, v in f.items()}
    return {q: v / (60 * h) for q, v in acc.items()}


def one_sided(res, tau, sign, h):
    """sign +1: forward difference (points tau + k h), -1: backward (tau - k h)."""
    acc = None
    for k, c in enumerate(FORWARD):
        f = D.evaluate(res, tau + sign * k * h, D.PHI)
        acc = {q: c * v for q, v in f.items()} if acc is None else {q: acc[q] + c * v for q, v in f.items()}
    return {q: sign * v / h for q, v in acc.items()}


def refine(diff, cap, label):
    """diff(h) -> dict of arrays.  Per quantity: the result at the smallest h/2 whose discrepancy against h still shrank."""
    best = {}
    prev, h = diff(H0), H0
    for _ in range(MAX_HALVINGS):
        cur = diff(h / 2)
        improved = False
        for q in cur:
            scale = float(np.max(np.abs(cur[q])))
            gap = float(np.max(np.abs(prev[q] - cur[q])))
            unc, is_abs = (gap / scale, 0) if scale > 0 else (gap, 1)
            if q not in best or unc < best[q][1]:
                best[q] = (cur[q], unc, is_abs, h / 2)
                improved = True
        prev, h = cur, h / 2
        if not improved:
            break
    store = {}
    for q, (val, unc, is_abs, hh) in best.items():
        print(f"  {label:22s} {q:18s} fd_uncertainty {unc:.2e} (h/2 = {hh:.2e}){' ABS' if is_abs else ''}"
              f"{'' if unc <= cap else '  NOT ADMITTED'}", flush=True)
        if unc <= cap:
            store.update({q: val, q + ".unc": np.array(unc), q + ".abs": np.array(is_abs), q + ".h_half": np.array(hh)})
    return store


def make_case(name):
    res, tau_arr = solve(name)
    edges = np.concatenate(([0.0], tau_arr))
    pts, skipped = [], 0
    for lo, hi in zip(edges[:-1], edges[1:]):
        if hi - lo < 8 * H0:
            skipped += 3
            continue
        pts += [lo + 4 * H0, 0.5 * (lo + hi), hi - 4 * H0]
    assert 10 * skipped <= 3 * len(tau_arr), (name, skipped)
    tau = np.array(pts)
    store = refine(lambda h: central(res, tau, h), D.CAP, name)
    store.update(tau=tau, phi=D.PHI, tau_arr=tau_arr, npoints=np.array(len(tau)), nskipped=np.array(skipped), h0=np.array(H0))
    np.savez_compressed(os.path.join(D.DERIV_DIR, name + ".npz"), **store)
    if name in D.ONE_SIDED:
        assert np.all(np.diff(edges) > 8 * H0)
        lower, top = tau_arr, np.array([0.0])
        back = refine(lambda h: one_sided(res, lower, -1, h), D.CAP_ONE_SIDED, name + " backward")
        fwd = refine(lambda h: one_sided(res, top, +1, h), D.CAP_ONE_SIDED, name + " forward")
        store = dict(tau=np.concatenate((top, lower)), phi=D.PHI, tau_arr=tau_arr)
        for q in D.QUANTITIES:
            if q in back and q in fwd:
                ax = 1 if q in ("u", "u0") else 0  # the tau axis
                store[q] = np.concatenate((fwd[q], back[q]), axis=ax)
                # each side against its own scale; the larger of the two is what the fixture is good to
                store[q + ".unc"] = np.array(max(float(fwd[q + ".unc"]), float(back[q + ".unc"])))
                store[q + ".abs"] = np.array(max(int(fwd[q + ".abs"]), int(back[q + ".abs"])))
        np.savez_compressed(os.path.join(D.DERIV_DIR, "onesided_" + name + ".npz"), **store)


if __name__ == "__main__":
    os.makedirs(D.DERIV_DIR, exist_ok=True)
    for case in (sys.argv[1:] or D.CASES):
        print(case, flush=True)
        make_case(case)
