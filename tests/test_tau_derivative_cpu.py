"""Host-side checks of the tau-derivative feature (no GPU): the public signatures, the C ABI declaration and its binding,
and the finite-difference fixtures of tests/golden/deriv (made by tests/golden/make_derivative_goldens.py from the reference)."""
import inspect
import os
import re

import numpy as np
import pytest

import deriv_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kwonly_false(fn, name):
    p = inspect.signature(fn).parameters[name]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, (fn, p)


def test_the_eight_evaluators_take_the_keyword_only_derivative_flag():
    """Keyword-only, so that the positional order stays the reference's (_assemble_intensity_and_fluxes.py:170, :334, :446, :527)."""
    from pydisort_amd.batch import BatchSolution
    from pydisort_amd.pydisort import _Closures
    for cls in (_Closures, BatchSolution):
        for name in ("u", "u0", "flux_up", "flux_down"):
            _kwonly_false(getattr(cls, name), "is_derivative_wrt_tau")
    pos = [n for n, p in inspect.signature(_Closures.u).parameters.items() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert pos == ["self", "tau", "phi", "is_antiderivative_wrt_tau", "return_Fourier_error", "return_tau_arr"]
    pos = [n for n, p in inspect.signature(_Closures.u0).parameters.items() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert pos == ["self", "tau", "is_antiderivative_wrt_tau", "return_tau_arr", "_return_act_dscale_for_reclass"]


def test_streamed_form_plan_and_helpers_carry_the_new_parameters():
    from pydisort_amd import subroutines
    from pydisort_amd._engine import Plan
    from pydisort_amd.batch import solve_columns_streamed
    p = inspect.signature(solve_columns_streamed).parameters["tau_order"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0
    assert inspect.signature(Plan.evaluate).parameters["derivative"].default is False
    assert list(inspect.signature(Plan.set_eval_order).parameters) == ["self", "order"]
    seen = []

    def u0(tau, is_antiderivative_wrt_tau=False, return_tau_arr=False, _return_act_dscale_for_reclass=False, *,
           is_derivative_wrt_tau=False):
        seen.append(is_derivative_wrt_tau)
        val = np.ones((4, np.size(tau)))
        return (val, 0.5) if _return_act_dscale_for_reclass else val

    up, down = subroutines.generate_diff_act_flux_funcs(u0)
    for f in (up, down):
        _kwonly_false(f, "is_derivative_wrt_tau")
        del seen[:]
        f(0.1, is_derivative_wrt_tau=True)
        assert seen == [True]
        del seen[:]
        f(0.1)
        assert seen == [False]


def test_both_orders_together_are_refused_on_the_host():
    """The flag pair is rejected before any device call (the plan is never touched)."""
    from pydisort_amd.batch import BatchSolution
    from pydisort_amd.pydisort import _Closures
    for cls in (_Closures, BatchSolution):
        with pytest.raises(ValueError):
            cls._order(True, True)
    with pytest.raises(ValueError):
        _Closures._order(False, True, True)  # with return_Fourier_error
    assert _Closures._order(False, True) is True and _Closures._order(True, False) is False


def test_header_declares_and_binding_binds_the_eval_order():
    from pydisort_amd import _lib
    with open(os.path.join(ROOT, "include", "rtd.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+rtd_plan_set_eval_order\s*\(\s*rtd_plan\s*\*\s*\w*\s*,\s*int32_t\s+\w+\s*\)\s*;", header)
    assert "bit 2" in header
    res, args = _lib.SIGNATURES["rtd_plan_set_eval_order"]
    assert len(args) == 2
    _lib.load().rtd_plan_set_eval_order  # the built library exports it


@pytest.mark.parametrize("name", D.CASES)
def test_fixture_of_every_listed_case_respects_the_admission_rules(name):
    z = D.load(name)
    only_flux = bool(D.case_kwargs(name).get("only_flux", False))
    nlayers = len(z["tau_arr"])
    assert int(z["npoints"]) + int(z["nskipped"]) == 3 * nlayers and 10 * int(z["nskipped"]) <= 3 * nlayers
    edges = np.concatenate(([0.0], z["tau_arr"]))
    for t in z["tau"]:  # no point closer than three of the largest steps to an interface
        assert np.min(np.abs(edges - t)) >= 3 * float(z["h0"])
    assert len(z["phi"]) == 3
    for q in D.QUANTITIES:
        if q == "u" and only_flux:
            continue
        assert q in z.files, (name, q, "not admitted")
        assert float(z[q + ".unc"]) <= D.CAP
        assert 2 * float(z[q + ".h_half"]) <= float(z["h0"])  # the largest step of the stencil behind the stored value
        assert z[q].shape[-1 if q != "u" else -2] == len(z["tau"])
        if int(z[q + ".abs"]):
            assert not np.any(z[q])


@pytest.mark.parametrize("name", D.ONE_SIDED)
def test_one_sided_fixtures(name):
    z = D.load(name, one_sided=True)
    assert np.array_equal(z["tau"], np.concatenate(([0.0], z["tau_arr"])))
    for q in D.QUANTITIES:
        assert q in z.files and float(z[q + ".unc"]) <= D.CAP_ONE_SIDED, (name, q)
