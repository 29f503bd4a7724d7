"""The oracle's analytic tau-derivative (oracle/disort_oracle.py, oracle/nt_oracle.py: ``is_derivative_wrt_tau=True``), pinned
on the CPU before the GPU sweeps of tests/test_gpu_random_orders.py hold the kernels against it.

Two references, both independent of the code under test:
  * the finite-difference fixtures made from the reference (tests/golden/deriv), under the rule the kernels are held by
    (deriv_cases.hold with TOL and CEILING of tests/test_gpu_tau_derivative.py; one-sided: ten times the fixture's own
    uncertainty, no floor, no ceiling);
  * sixth-order central differences of the oracle's OWN values (which are pinned to the reference's), on every seed of the four
    random families and every edge case, held to deriv_cases.CAP = 5e-9 -- the admission cap of such a stencil.
Measured: fixtures at most 4.8e-11 of the scale (cfg5_0 u0; every quantity within 9.2 x its fd_uncertainty), one-sided at most
5.0e-10 (fd_uncertainty 4.4e-10); own differences at most 1.3e-9 over the 122 seeds, the 27 twins and the edge cases (flux_up
of random32/15, a seed with a layer at omega = 1 - 1e-6; 3.5e-10 in the thin column random/34; 3.0e-10 and less elsewhere).
"""
import warnings

import numpy as np
import pytest

import deriv_cases as D
import goldens
from test_gpu_parity import EDGE_CASES
from test_gpu_tau_derivative import CEILING, TOL

H, HALVINGS = 1e-2, 10  # the steps tried: H / 2 ... H / 1024 (the fixtures' 1e-4 / 2 ... / 16 lie in that range)
CENTRAL = ((3, 1.0), (2, -9.0), (1, 45.0), (-1, -45.0), (-2, 9.0), (-3, -1.0))  # / 60 h


def _oracle(kw):
    from oracle import disort_oracle as O
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return O.pydisort(**kw)


@pytest.mark.parametrize("name", D.CASES)
def test_analytic_derivative_against_the_differentiated_reference(name):
    z = D.load(name)
    res = _oracle(D.case_kwargs(name))
    D.hold("oracle/" + name, D.evaluate(res, z["tau"], z["phi"], is_derivative_wrt_tau=True), z, TOL, CEILING)


@pytest.mark.parametrize("name", D.ONE_SIDED)
def test_interfaces_take_the_layer_that_ends_there_and_tau_0_the_right_derivative(name):
    z = D.load(name, one_sided=True)
    res = _oracle(D.case_kwargs(name))
    D.hold("oracle/one_sided/" + name, D.evaluate(res, z["tau"], z["phi"], is_derivative_wrt_tau=True), z, 0.0, None)


def _interior(kw, tau):
    """The points of tau more than 1e-3 of the column's depth from every interface (0 and the bottom included)."""
    tau_arr = np.atleast_1d(np.asarray(kw["tau_arr"], float))
    edges = np.concatenate(([0.0], tau_arr))
    return tau[np.min(np.abs(tau[:, None] - edges[None, :]), axis=1) > 1e-3 * tau_arr[-1]]


def _central(res, tau, h):
    acc = None
    for k, c in CENTRAL:
        f = D.evaluate(res[:4], tau + k * h, None)
        acc = {q: c * v for q, v in f.items()} if acc is None else {q: acc[q] + c * v for q, v in f.items()}
    return {q: v / (60 * h) for q, v in acc.items()}


def _own_differences(label, kw, tau):
    """d/dtau of u0, flux_up and both parts of flux_down, analytic, against the central differences of the oracle's own values.
    The step is chosen as the fixtures' maker chooses it, by the differences alone: per point the largest that keeps the stencil
    inside the layer (a quarter of the distance to the nearest interface, at most H), halved HALVINGS times, and per point and
    quantity the result that moved least from the step before it; the analytic derivative has no part in the choice.
    u0 is held on its own scale.  The three fluxes are held on the case's flux scale, the largest derivative among them: a
    difference of values f at step h cannot resolve a derivative below eps |f| / h, and in a thin column the diffuse fluxes hardly
    change (random/34: depth 1.2e-3, flux_down_diffuse 0.0713 with derivative 7e-4, h <= 1.2e-6 at the point nearest the top: the
    differences are good to 7e-12 absolutely, 9.7e-9 of that derivative and 4e-12 of the direct beam's 1.77), or are the 1e-17
    a linear solve leaves where they are zero (random32/2: under a non-scattering layer 26 deep).  A dropped factor in a flux
    is an error of its own size in one of the three, so of at least the smallest flux's share of that scale."""
    res = _oracle(kw)  # (a seed the oracle cannot solve raises here: the test fails, no seed is skipped)
    edges = np.concatenate(([0.0], np.atleast_1d(np.asarray(kw["tau_arr"], float))))
    h = np.minimum(H, 0.25 * np.min(np.abs(tau[:, None] - edges[None, :]), axis=1))
    got = D.evaluate(res[:4], tau, None, is_derivative_wrt_tau=True)
    best, gap, prev = {}, {}, _central(res, tau, h)
    for _ in range(HALVINGS):
        h = h / 2
        cur = _central(res, tau, h)
        for q in cur:
            g = np.max(np.abs(prev[q] - cur[q]).reshape(-1, len(tau)), axis=0)
            if q not in best:
                best[q], gap[q] = cur[q].copy(), g
            else:
                better = g < gap[q]
                best[q][..., better] = cur[q][..., better]
                gap[q] = np.where(better, g, gap[q])
        prev = cur
    flux_scale = max(float(np.max(np.abs(best[q]))) for q in D.FLUXES)
    for q, fd in best.items():
        assert np.all(np.isfinite(got[q])), (label, q)
        if q == "u0":
            err = goldens.max_rel_err(got[q], fd)[0]
        else:
            err = float(np.max(np.abs(got[q] - fd))) / flux_scale
        print(f"oracle derivative vs own differences {label:24s} {q:18s} {err:.3e}")
        assert err < D.CAP, (label, q, err)


SEEDS = [(f, s) for f, n in D.SWEEP_FAMILIES for s in range(n)]
TWINS = [(f, s) for f, s in SEEDS if D.sweep_case(f, s)[1]]


@pytest.mark.parametrize("family,seed", SEEDS)
def test_analytic_derivative_against_differences_of_the_oracles_own_values(family, seed):
    from test_gpu_random_parity import eval_points
    kw = D.random_case(family, seed)
    tau = _interior(kw, eval_points(family, seed, kw)[0])
    assert len(tau) > 0, (family, seed, "no interior point")
    _own_differences(f"{family}/{seed}", kw, tau)


def test_the_near_conservative_seeds_are_the_ones_counted():
    """24 of the 40 32-stream seeds and 3 of the 12 64-stream seeds have a layer at omega > 1 - 1e-5, none elsewhere."""
    assert len(SEEDS) == 122
    assert {f: sum(1 for g, _ in TWINS if g == f) for f, _ in D.SWEEP_FAMILIES} == {"random": 0, "random32": 24, "random64": 3, "random128": 0}


@pytest.mark.parametrize("family,seed", TWINS)
def test_twin_of_a_near_conservative_seed(family, seed):
    """The atmosphere the GPU sweeps run instead (omega capped at 0.999): the oracle solves it, and its derivative holds as above."""
    from test_gpu_random_parity import eval_points
    kw, twin = D.sweep_case(family, seed)
    assert twin and np.max(kw["omega_arr"]) == 0.999
    tau = _interior(kw, eval_points(family, seed, kw)[0])
    assert len(tau) > 0, (family, seed, "no interior point")
    _own_differences(f"{family}/{seed}/twin", kw, tau)


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_edge_case_derivative_against_differences_of_the_oracles_own_values(name):
    from test_gpu_random_parity import eval_points
    kw = EDGE_CASES[name]
    tau = _interior(kw, eval_points("edge", list(EDGE_CASES).index(name), kw)[0])
    assert len(tau) > 0, (name, "no interior point")
    _own_differences("edge/" + name, kw, tau)


def test_both_orders_together_are_refused_and_the_flag_is_keyword_only():
    import inspect
    from oracle import disort_oracle as O, nt_oracle
    kw = D.case_kwargs("nt_L6_q16")
    sol = O.Solution(O.prepare(**kw))
    tau, phi = np.array([0.3, 0.9]), np.array([0.0, 1.0])
    for fn in (sol.u, sol.u0, sol.flux_up, sol.flux_down, nt_oracle.corrected_u(sol)):
        p = inspect.signature(fn).parameters["is_derivative_wrt_tau"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
        args = (tau, phi) if "phi" in inspect.signature(fn).parameters else (tau,)
        with pytest.raises(ValueError):
            fn(*args, True, is_derivative_wrt_tau=True)
    # the corrections are part of the derivative
    assert nt_oracle.nt_active(sol.p)
    assert not np.array_equal(nt_oracle.corrected_u(sol)(tau, phi, is_derivative_wrt_tau=True), sol.u(tau, phi, is_derivative_wrt_tau=True))
