"""Both tau-orders of every evaluator -- the derivative (``is_derivative_wrt_tau``) and the antiderivative
(``is_antiderivative_wrt_tau``) of u, u0, flux_up and both parts of flux_down -- swept over the random families of
tests/test_gpu_random_parity.py (60 + 40 + 12 + 10 seeds) and the edge cases of tests/test_gpu_parity.py, against the CPU oracle's
closed forms (oracle/disort_oracle.py, oracle/nt_oracle.py; its analytic derivative is pinned on the CPU by
tests/test_oracle_tau_derivative.py).  Run with ``-m gpu`` on an MI355X.

Points: ``eval_points`` of the value sweeps -- 0, every interface, the bottom and random interior points; NT corrections where the
case has them; u left out for only_flux.  No seed is left out: a seed with a layer at omega > 1 - 1e-5 (24 of the 40 32-stream
seeds, 3 of the 12 64-stream ones), where the oracle's own float64 is off and the 40-digit fixtures hold values only, runs as its
twin with omega_arr = minimum(omega_arr, 0.999), whose values are first held to the tolerances of the family's well-conditioned
seeds (deriv_cases.sweep_case).

Metric, per quantity of a case and order: the largest difference over the largest magnitude of the oracle's (deriv_cases.hold's).
A quantity the oracle has below ZERO = 1e-12 of the case's flux scale (the largest magnitude among its three fluxes at that
order) is zero to rounding -- identically zero without a beam or without scattering, or the 1e-17 a linear solve leaves under a
non-scattering layer -- and is held absolutely on that scale.  Pointwise errors are recorded, not held.

Tolerance: ten times the worst measured on an MI355X per family and order, MEASURED_WORST below; the ceilings are conditions, not
measurements (derivative 1e-7: a dropped q, scale_tau, 1/mu or sign is 1e-2 or more on these inputs; antiderivative 2e-8 up to
64 streams and 1e-7 above: what tools/fuzz_batch.py holds), and every tolerance is asserted to lie under its ceiling.

Measured (1 262 quantities of 131 cases and two orders; profiles/tau_derivative_parity_report.json, tau_orders/...), worst
scale-relative error, derivative / antiderivative: random 4.6e-12 / 3.9e-12, random32 2.1e-10 / 1.4e-11, random64 1.7e-9 /
4.5e-11, random128 3.6e-10 / 5.0e-10, edge cases 1.4e-11 / 3.0e-11, the seven-column batch with corrections 4.5e-13.  The 27 twins'
values: at most 8.7e-11 (32 streams) and 1.18e-9 (64 streams) of the scale, 2.5e-8 pointwise.  Pointwise, recorded only: up to
6.1e-7 (the derivative of u of random32/25's twin, at points 1e-8 of the largest).
"""
import warnings

import numpy as np
import pytest

import deriv_cases as D
import goldens
from test_gpu_parity import EDGE_CASES
from test_gpu_random_parity import eval_points, oracle_solution

pytestmark = pytest.mark.gpu

ORDERS = {"derivative": dict(is_derivative_wrt_tau=True), "antiderivative": dict(is_antiderivative_wrt_tau=True)}
ZERO = 1e-12
TWIN_VALUE_TOL = {"random32": (1e-9, 1e-6), "random64": (2e-9, 1e-6)}  # of the families' well-conditioned seeds
# (family, order) -> the worst scale-relative error against the oracle over the family's cases and quantities, MI355X
MEASURED_WORST = {
    ("random", "derivative"): 4.58e-12,       # seed 43, u0
    ("random", "antiderivative"): 3.94e-12,   # seed 43, u0
    ("random32", "derivative"): 2.05e-10,     # twin of seed 25, u0
    ("random32", "antiderivative"): 1.42e-11, # twin of seed 38, u
    # (64 streams: the oracle's own roundoff is ~1e-9, test_random_64_stream_case_matches_oracle; seed 11's twin has 1.07e-9 in its values)
    ("random64", "derivative"): 1.71e-9,      # twin of seed 11, u
    ("random64", "antiderivative"): 4.47e-11, # twin of seed 11, u
    ("random128", "derivative"): 3.58e-10,    # seed 5, u
    ("random128", "antiderivative"): 4.97e-10,  # seed 3, u0
    ("edge", "derivative"): 1.45e-11,         # padded_30, u0
    ("edge", "antiderivative"): 3.0e-11,      # max_streams_64, u0
    ("batch_nt", "derivative"): 4.52e-13,     # column 3
}
TOL = {k: 10 * v for k, v in MEASURED_WORST.items()}


def ceiling(order, nquad):
    if order == "derivative":
        return 1e-7
    return 2e-8 if nquad <= 64 else 1e-7


def test_every_tolerance_lies_under_its_ceiling():
    for (family, order), tol in TOL.items():
        assert tol <= ceiling(order, 66 if family == "random128" else 64) * (1 + 1e-12), (family, order, tol)


@pytest.fixture(scope="module")
def amd():
    import pydisort_amd
    from pydisort_amd import _engine
    assert _engine.device_count() >= 1, "no HIP device visible"
    return pydisort_amd


def _compare(label, family, got, want):
    """Both dicts as deriv_cases.evaluate returns them, per order -> records and asserts every quantity."""
    from conftest import record_parity
    for order in ORDERS:
        tol = TOL[family, order]
        flux_scale = max(float(np.max(np.abs(want[order][q]))) for q in D.FLUXES)
        for q in D.QUANTITIES:
            if q not in want[order]:
                continue
            g, w = got[order][q], want[order][q]
            assert g.shape == w.shape, (label, order, q, g.shape, w.shape)
            assert np.all(np.isfinite(g)) and np.all(np.isfinite(w)), (label, order, q)
            if float(np.max(np.abs(w))) > ZERO * flux_scale:
                err, pw = goldens.max_rel_err(g, w)
            else:
                err, pw = float(np.max(np.abs(g - w))) / flux_scale, 0.0
            print(f"tau-order {label:22s} {order:14s} {q:18s} scale-rel {err:.3e} pointwise {pw:.3e} tol {tol:.1e}")
            record_parity(f"tau_orders/{label}/{order}/{q}", err, pw, tol, None, against="oracle, analytic")


def _sweep(amd, family, label, kw, tau, phi, ref, value_tol=None):
    from conftest import record_parity
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = amd.pydisort(**kw)
    assert len(res) == len(ref) == (4 if kw.get("only_flux") else 5)
    if value_tol is not None:  # a twin is a new atmosphere: its values first, at what the family's well-conditioned seeds are held to
        a, b = goldens.max_rel_err(res[4](tau, phi), ref[4](tau, phi))
        record_parity(f"tau_orders/{label}/values", a, b, *value_tol)
    got = {order: D.evaluate(res, tau, phi, **flag) for order, flag in ORDERS.items()}
    want = {order: D.evaluate(ref, tau, phi, **flag) for order, flag in ORDERS.items()}
    _compare(label, family, got, want)


@pytest.mark.parametrize("family,seed", [(f, s) for f, n in D.SWEEP_FAMILIES for s in range(n)])
def test_both_orders_of_a_random_case_against_the_oracle(amd, family, seed):
    kw, twin = D.sweep_case(family, seed)
    tau, phi = eval_points(family, seed, kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = oracle_solution(family, seed, kw, tau)  # (fails for a seed the oracle cannot solve: none is listed as rejected)
    _sweep(amd, family, f"{family}/{seed}" + ("/twin" if twin else ""), kw, tau, phi, ref, TWIN_VALUE_TOL[family] if twin else None)


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_both_orders_of_an_edge_case_against_the_oracle(amd, name):
    from oracle import disort_oracle as O
    kw = EDGE_CASES[name]
    tau, phi = eval_points("edge", list(EDGE_CASES).index(name), kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = O.pydisort(**kw)
    _sweep(amd, "edge", "edge/" + name, kw, tau, phi, ref)


def test_batch_derivative_with_corrections_in_six_layers_against_the_oracle(amd):
    """Seven columns with their own mu0 and layers, Nakajima-Tanaka corrections active in all six layers (17 moments given, 16
    used), through ``pydisort_batch``: d/dtau of u of every column at the mid-layer points and at 0 and the interfaces."""
    from conftest import record_parity
    from oracle import disort_oracle as O
    from pydisort_amd import synthetic
    C = 7
    cfg = dict(synthetic.cfg4_columns(C, L=6, NQuad=16), NLeg=16, NT_cor=True)
    edges = np.concatenate((np.zeros((C, 1)), cfg["tau_arr"]), axis=1)
    tau = np.concatenate((0.5 * (edges[:, 1:] + edges[:, :-1]), edges), axis=1)
    _, sol = amd.pydisort_batch(**cfg)
    got = sol.u(tau, D.PHI, is_derivative_wrt_tau=True)
    tol = TOL["batch_nt", "derivative"]
    for c in range(C):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = O.pydisort(**dict(synthetic.column_kwargs(cfg, c), NLeg=16, NT_cor=True))
        want = ref[4](tau[c], D.PHI, is_derivative_wrt_tau=True)
        assert not np.array_equal(want, O.Solution(O.prepare(**dict(synthetic.column_kwargs(cfg, c), NLeg=16))).u(
            tau[c], D.PHI, is_derivative_wrt_tau=True))  # (the corrections are in it)
        err, pw = goldens.max_rel_err(got[c], want)
        print(f"tau-order batch_nt/column{c} derivative u scale-rel {err:.3e} pointwise {pw:.3e} tol {tol:.1e}")
        record_parity(f"tau_orders/batch_nt/column{c}/derivative/u", err, pw, tol, None, against="oracle, analytic")
