"""tau-derivatives of u, u0 and the fluxes evaluated on the device (``is_derivative_wrt_tau=True``, bit 2 of
rtd_plan_evaluate's flag word, rtd_plan_set_eval_order) -- run with ``-m gpu`` on an MI355X.

Reference: the reference's own closures differentiated by sixth-order finite differences at two steps (tests/golden/deriv,
tests/golden/make_derivative_goldens.py); every fixture quantity carries its fd_uncertainty (<= 5e-9, one-sided <= 1e-6).

Tolerance, scale-relative (max |d| / max |reference derivative| per quantity), per quantity of a case:
    min(CEILING, max(TOL, 10 x fd_uncertainty))
CEILING = 1e-7 is a condition, not a measurement: a missing scale_tau, 1/mu0 or sign is an O(1) error, 1e-7 cannot hide one.
TOL = ten times the worst scale-relative error measured over the cases on an MI355X: MEASURED_WORST below.  Measured (113
quantities of 20 case runs): 4.9e-11 at worst (cfg5_0 u0; cfg4 3.6e-11, 9corrections 4.2e-11, 6h flux_up 4.3e-11, the one-layer
catalogue cases 1e-13 ... 1e-11) -- every figure within a factor of three of its fixture's own fd_uncertainty (at most 5.7e-11), so
what is measured is the finite-difference error of the fixtures, not the kernels'.  Pointwise (over the points above 1e-8 of the
scale) the worst is 2.8e-6 (cfg5_0 u0, at derivatives 1e-5 of the largest); recorded, not held.  One-sided fixtures: 8.7e-12 ...
5.0e-10 at fd_uncertainty 6.2e-12 ... 1.0e-9.
The nine cases added for what those left out (deriv_cases.NT_MULTILAYER, RANDOM: corrections in several layers, thermal polynomials
of degree 2, 6 and 66 ... 112 streams, 40 modes, vector b_pos, only_flux; 44 quantities, fd_uncertainty 4.4e-14 ... 8.0e-11): 1.0e-13
... 1.2e-10 (random128_6 flux_up at fd_uncertainty 7.3e-11; random_29 8.6e-11 at 8.0e-11; nt_L6_q16 3.2e-12, random_3 3.9e-12,
random_24 3.9e-11, random_31 7.7e-12, random_49 4.6e-12, random128_1 1.2e-11, random128_4 3.2e-11) -- again the fixtures' own error,
so TOL stays what the first 18 cases gave; one-sided nt_L6_q16 7.0e-12 ... 2.1e-11, random_24 1.4e-11 ... 3.3e-10 (fd_uncertainty
up to 4.0e-10).  The oracle's analytic derivative, held by the same rule in tests/test_oracle_tau_derivative.py, is what the
sweeps of tests/test_gpu_random_orders.py compare with, at every seed and interface.
A quantity whose reference derivative is identically zero (no diffuse downward flux without scattering; no direct beam) is held
absolutely, at the same tolerance times the largest derivative scale among the case's fluxes.
"""
import ctypes
import warnings

import numpy as np
import pytest

import deriv_cases as D

pytestmark = pytest.mark.gpu

CEILING = 1e-7
MEASURED_WORST = 4.88e-11  # cfg5_0 u0 (64 streams, 50 layers); its fixture's fd_uncertainty is 2.3e-11
TOL = 10 * MEASURED_WORST


@pytest.fixture(scope="module")
def amd():
    import pydisort_amd
    from pydisort_amd import _engine
    assert _engine.device_count() >= 1, "no HIP device visible"
    return pydisort_amd


def _solve(amd, name, **extra):
    kw = dict(D.case_kwargs(name), **extra)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return amd.pydisort(**kw)


def _hold(label, got, z, tol_floor=TOL, ceiling=CEILING, factor=10.0):
    """Records and asserts every quantity of `got` (dict as deriv_cases.evaluate returns) against the fixture z: the rule is
    deriv_cases.hold, shared with the oracle's own test (tests/test_oracle_tau_derivative.py)."""
    from conftest import record_parity

    def record(label, q, err, pw, tol, unc):
        record_parity(f"tau_derivative/{label}/{q}", err, pw, tol, None, against="reference, 6th-order FD", fd_uncertainty=unc)

    D.hold(label, got, z, tol_floor, ceiling, factor, record)


@pytest.mark.parametrize("name", D.CASES)
def test_closure_derivatives_against_the_differentiated_reference(amd, name):
    """Every fixture case through ``pydisort``: d/dtau of u (with its NT corrections where the case has them), u0, flux_up,
    flux_down (diffuse, direct) at three points per layer and three azimuths."""
    z = D.load(name)
    res = _solve(amd, name)
    _hold(name, D.evaluate(res, z["tau"], z["phi"], is_derivative_wrt_tau=True), z)


@pytest.mark.parametrize("name", ("cfg4_0", "cfg4_2", "cfg5_0"))
def test_batch_derivatives_against_the_differentiated_reference(amd, name):
    """The multi-layer synthetic columns inside a larger batch (other columns behind them), through ``pydisort_batch``; the
    other columns are evaluated at their own mid-layer points in the same call."""
    z = D.load(name)
    cfg, col = D.batch_config(name)
    _, sol = amd.pydisort_batch(**cfg)
    C = cfg["tau_arr"].shape[0]
    tau = np.empty((C, len(z["tau"])))
    for c in range(C):  # the same relative positions in every column's own layers
        edges = np.concatenate(([0.0], cfg["tau_arr"][c]))
        own = np.concatenate(([0.0], z["tau_arr"]))
        l = np.searchsorted(z["tau_arr"], z["tau"])
        tau[c] = edges[l] + (z["tau"] - own[l]) / (own[l + 1] - own[l]) * (edges[l + 1] - edges[l])
    tau[col] = z["tau"]
    fd = sol.flux_down(tau, is_derivative_wrt_tau=True)
    got = {"u": sol.u(tau, z["phi"], is_derivative_wrt_tau=True)[col], "u0": sol.u0(tau, is_derivative_wrt_tau=True)[col],
           "flux_up": sol.flux_up(tau, is_derivative_wrt_tau=True)[col], "flux_down_diffuse": fd[0][col],
           "flux_down_direct": fd[1][col]}
    _hold("batch/" + name, got, z)
    # batch and per-column results are the same bits (a column's closure values do not depend on the batch it was solved in)
    one = D.evaluate(_solve(amd, name), z["tau"], z["phi"], is_derivative_wrt_tau=True)
    for q in D.QUANTITIES:
        assert np.array_equal(one[q], got[q]), q


@pytest.mark.parametrize("name", D.ONE_SIDED)
def test_interfaces_take_the_layer_that_ends_there_and_tau_0_the_right_derivative(amd, name):
    """argmax(tau <= tau_arr): at tau = tau_arr[l] the derivative is the one-sided one from above (backward differences of the
    reference inside layer l), at tau = 0 the right derivative (forward differences).  Tolerance 10 x the fixture's own
    uncertainty (one-sided stencils lose about two digits: fd_uncertainty 6e-12 ... 1e-9; measured errors 9e-12 ... 5e-10)."""
    z = D.load(name, one_sided=True)
    res = _solve(amd, name)
    _hold("one_sided/" + name, D.evaluate(res, z["tau"], z["phi"], is_derivative_wrt_tau=True), z, tol_floor=0.0, ceiling=None)
    # ... and it is NOT the derivative from below: across an interior interface the two sides differ by far more than that
    if len(z["tau_arr"]) > 1:
        below = D.evaluate(res, z["tau_arr"][:-1] + 1e-9, z["phi"], is_derivative_wrt_tau=True)["u0"]
        assert np.max(np.abs(below - z["u0"][:, 1:-1])) > 1e-6 * np.max(np.abs(z["u0"]))


def test_direct_beam_identity(amd):
    """d(flux_down_direct)/dtau = -flux_down_direct / mu0, to rounding (1e-13 relative)."""
    for name in ("9c", "cfg4_0", "cfg2_q32", "4c"):
        kw = D.case_kwargs(name)
        res = _solve(amd, name)
        tau = np.concatenate(([0.0], D.load(name)["tau"], np.atleast_1d(kw["tau_arr"])))
        val = res[2](tau)[1]
        der = res[2](tau, is_derivative_wrt_tau=True)[1]
        assert np.all(val > 0)
        assert np.max(np.abs(der + val / kw["mu0"]) / (val / kw["mu0"])) < 1e-13


def _all(sol, tau, phi, **kw):
    fd = sol.flux_down(tau, **kw)
    return dict(u=sol.u(tau, phi, **kw), u0=sol.u0(tau, **kw), flux_up=sol.flux_up(tau, **kw), flux_down_diffuse=fd[0],
                flux_down_direct=fd[1])


@pytest.mark.parametrize("nt", (False, True))
def test_retained_lean_and_resolving_plans_give_the_one_window_bits(amd, nt):
    from pydisort_amd import synthetic
    C = 7
    cfg = synthetic.cfg4_columns(C, L=6, NQuad=16)
    if nt:
        cfg = dict(cfg, NLeg=16, NT_cor=True)  # (17 moments given: one more than used)
    edges = np.concatenate((np.zeros((C, 1)), cfg["tau_arr"]), axis=1)
    tau = np.concatenate((0.5 * (edges[:, 1:] + edges[:, :-1]), edges), axis=1)
    phi = np.array([0.0, 1.0, 2.5])
    _, one = amd.pydisort_batch(**cfg)
    assert one.plan.windows()[1] == 1
    want = _all(one, tau, phi, is_derivative_wrt_tau=True)
    assert np.all(np.isfinite(want["u"])) and np.max(np.abs(want["u"])) > 0
    for kw in (dict(retain="full"), dict(retain="lean"), dict(retain=False)):
        _, sol = amd.pydisort_batch(work_columns=3, **kw, **cfg)
        assert sol.plan.windows()[1] == 3 and sol.plan.retained_form() == (kw["retain"] or None)
        got = _all(sol, tau, phi, is_derivative_wrt_tau=True)
        for q in want:
            assert np.array_equal(got[q], want[q]), (kw, q)
    if nt:  # the corrections are part of the derivative: without them u differs
        _, plain = amd.pydisort_batch(**dict(cfg, NT_cor=False))
        assert not np.array_equal(plain.u(tau, phi, is_derivative_wrt_tau=True), want["u"])


@pytest.mark.parametrize("G", (2, 3))
def test_mode_shard_partial_derivatives_add_up(amd, G):
    from pydisort_amd import synthetic
    cfg = synthetic.cfg4_columns(3, L=6, NQuad=16)
    edges = np.concatenate((np.zeros((3, 1)), cfg["tau_arr"]), axis=1)
    tau = np.concatenate((0.5 * (edges[:, 1:] + edges[:, :-1]), edges), axis=1)
    phi = np.array([0.0, 1.0, 2.5])
    _, full = amd.pydisort_batch(**cfg)
    want = _all(full, tau, phi, is_derivative_wrt_tau=True)
    acc = None
    for r in range(G):
        _, part = amd.pydisort_batch(mode_shard=(r, G), **cfg)
        got = _all(part, tau, phi, is_derivative_wrt_tau=True)
        acc = got if acc is None else {q: acc[q] + got[q] for q in got}
    for q in want:
        assert np.max(np.abs(acc[q] - want[q])) <= 1e-12 * np.max(np.abs(want[q])), q


def test_streamed_form_returns_every_order(amd):
    """solve_columns_streamed(..., tau_order): +1 the derivatives and -1 the antiderivatives of the BatchSolution evaluators
    (1e-12 of the scale: the streamed form prepares its inputs on the device, the batch in NumPy); 0 is the call without the
    argument, bit for bit -- also at the interfaces, where the run path takes the fused evaluation."""
    from pydisort_amd import synthetic
    C = 50
    cfg = synthetic.cfg4_columns(C, L=6, NQuad=16)
    edges = np.concatenate((np.zeros((C, 1)), cfg["tau_arr"]), axis=1)
    mids = 0.5 * (edges[:, 1:] + edges[:, :-1])
    phi = np.array([0.0, 2.0])
    _, sol = amd.pydisort_batch(**cfg)
    for order, kw in ((1, dict(is_derivative_wrt_tau=True)), (-1, dict(is_antiderivative_wrt_tau=True))):
        for tau in (mids, edges):
            want = _all(sol, tau, phi, **kw)
            got = amd.solve_columns_streamed(cfg, tau, phi, chunk_columns=16, tau_order=order)
            for q in want:
                assert np.max(np.abs(got[q] - want[q])) <= 1e-12 * np.max(np.abs(want[q])), (order, q)
    for tau in (mids, edges):
        a = amd.solve_columns_streamed(cfg, tau, phi, chunk_columns=16)
        b = amd.solve_columns_streamed(cfg, tau, phi, chunk_columns=16, tau_order=0)
        for q in a:
            assert np.array_equal(a[q], b[q]), q
    # the stored-points path of a plan driven by hand: the order holds for run() + fetch() and goes back to 0
    _, sol2 = amd.pydisort_batch(_defer_solve=True, **cfg)
    plan = sol2.plan
    plan.set_eval_points(edges, phi)
    plan.run()
    v0 = plan.fetch()
    plan.set_eval_order(1)
    plan.run()
    d1 = plan.fetch()
    plan.set_eval_order(0)
    plan.run()
    v1 = plan.fetch()
    want = _all(sol, edges, phi, is_derivative_wrt_tau=True)
    for q in want:
        assert np.array_equal(v0[q], v1[q]) and np.array_equal(d1[q], want[q]), q
    with pytest.raises(ValueError):
        plan.set_eval_order(2)
    with pytest.raises(ValueError):
        amd.solve_columns_streamed(cfg, mids, phi, tau_order=2)


def test_actinic_flux_helpers_pass_the_keyword_through(amd):
    """generate_diff_act_flux_funcs: d/dtau of the diffuse actinic fluxes, reclassification term included, against central
    differences of the same functions' values (delta-M scaled case: the reclassification term is not zero)."""
    from pydisort_amd import subroutines
    res = _solve(amd, "cfg4_0")
    up, down = subroutines.generate_diff_act_flux_funcs(res[3])
    tau = D.load("cfg4_0")["tau"]
    h = 1e-4
    for f in (up, down):
        fd = sum(c * f(tau + k * h) for k, c in ((3, 1.0), (2, -9.0), (1, 45.0), (-1, -45.0), (-2, 9.0), (-3, -1.0))) / (60 * h)
        got = f(tau, is_derivative_wrt_tau=True)
        assert np.max(np.abs(got - fd)) < 1e-8 * np.max(np.abs(fd))
    rec = res[3](tau, _return_act_dscale_for_reclass=True, is_derivative_wrt_tau=True)[1]
    assert np.max(np.abs(rec)) > 0


def test_error_paths(amd):
    from pydisort_amd import _lib
    res = _solve(amd, "9c")
    tau, phi = np.array([0.1, 0.5]), np.array([0.0])
    for call in (lambda: res[4](tau, phi, True, is_derivative_wrt_tau=True),
                 lambda: res[3](tau, True, is_derivative_wrt_tau=True),
                 lambda: res[1](tau, is_antiderivative_wrt_tau=True, is_derivative_wrt_tau=True),
                 lambda: res[2](tau, True, is_derivative_wrt_tau=True),
                 lambda: res[4](tau, phi, return_Fourier_error=True, is_derivative_wrt_tau=True)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="tau input outside the tau range"):
        res[4](np.array([1e9]), phi, is_derivative_wrt_tau=True)
    with pytest.raises(ValueError, match="tau input outside the tau range"):
        res[1](np.array([-0.1]), is_derivative_wrt_tau=True)
    with pytest.raises(NotImplementedError):
        _solve(amd, "9c", autograd_compatible=True)
    # the C ABI itself: bits 0 and 2 together are RTD_ERR_ARG (1); the tau range is reported as before (3)
    plan = res[1].__self__.plan
    lib = _lib.load()
    t = np.ascontiguousarray(tau[None])
    fu = np.empty((1, 2))
    args = (plan._h, 2, _lib.dptr(t), 0, None)
    rest = (None, None, _lib.dptr(fu), None, None, None)
    assert lib.rtd_plan_evaluate(*args, 1 | 4, *rest) == 1
    assert lib.rtd_plan_evaluate(*args, 4, *rest) == 0
    assert np.array_equal(fu[0], res[1](tau, is_derivative_wrt_tau=True))
    bad = np.array([[0.1, 1e9]])
    assert lib.rtd_plan_evaluate(plan._h, 2, _lib.dptr(bad), 0, None, 4, *rest) == _lib.RTD_ERR_TAU_RANGE
    assert lib.rtd_plan_set_eval_order(plan._h, ctypes.c_int32(3)) == 1
    with pytest.raises(ValueError):
        plan.evaluate(t, None, antiderivative=True, derivative=True)
