"""The float64 oracle's Nakajima-Tanaka terms (oracle/nt_oracle.py) against the 40-digit closed-form truth of tools/nt_truth.py
(fixtures: tests/golden/nt, made by tests/golden/make_nt_truth_goldens.py).  The oracle restates the reference's float64 formulas and
is what every oracle-based NT test on the GPU compares with; the arbiter shares no code with it.

Distances are max|oracle - truth| / max|truth| over a fixture and order.  MEASURED is the worst of the three orders when the
fixtures were made (value / antiderivative / derivative in the comment); the bound is ten times that and never above CEILING.
The two near-node fixtures are where the shared float64 formulas cancel (att - e against mu0 / (mu0 - mu); chi's 1 / x^2) and
carry their own figure.
"""
import importlib.util
import os
import warnings

import numpy as np
import pytest

import goldens
import nt_truth_cases as NC

CEILING = 1e-9
MEASURED = {                          # value     antider   deriv
    "q6_L1": 2.9e-15,                 # 2.87e-15  2.34e-15  1.61e-15
    "q10_L2_low_sun": 3.9e-15,        # 3.05e-15  3.65e-15  3.87e-15
    "q16_L7_mixed": 6.4e-15,          # 3.90e-15  3.74e-15  6.38e-15
    "q16_L50": 1.6e-14,               # 1.55e-14  9.42e-15  1.42e-14
    "q18_L3": 4.9e-14,                # 4.21e-14  4.85e-14  1.96e-14
    "q34_L3": 9.8e-14,                # 8.31e-14  5.42e-14  9.77e-14
    "q66_L2": 2.9e-13,                # 2.36e-13  2.89e-13  1.77e-13
    "q32_L20_cloud": 1.7e-13,         # 1.44e-13  1.69e-13  6.03e-14
    "q32_L20_thick": 8.6e-14,         # 4.15e-14  8.54e-14  7.08e-14
    "q64_L5": 2.7e-13,                # 2.55e-13  2.68e-13  1.44e-13
    "q128_L2": 6.3e-13,               # 6.27e-13  5.10e-13  5.76e-13
    "tp_4a": 8.5e-13,                 # 8.21e-13  8.45e-13  2.00e-13
    "tp_4b": 8.6e-13,                 # 8.25e-13  8.57e-13  2.00e-13
    "tp_5a": 9.6e-14,                 # 9.56e-14  1.01e-14  4.00e-14
    "tp_5b": 5.5e-14,                 # 3.45e-14  2.89e-14  5.41e-14
    "batch7_q16_L6": 5.9e-14,         # 5.87e-14  4.71e-14  3.46e-14   (worst column)
}
MEASURED_NEAR_NODE = {
    "q16_L4_mu0_near_node": 1.3e-10,   # 1.29e-10  8.88e-11  2.22e-11   mu0 = node (1 + 1e-6): eps / 1e-6
    "q16_L4_smu0_near_node": 1.3e-7,   # 1.25e-07  1.52e-08  5.75e-09   scaled mu0 = node (1 + 1e-5): eps / 1e-5^2 times chi's terms
}
GOLDEN_TOL = dict(tp_4a=1e-7, tp_4b=1e-10, tp_5a=1e-7, tp_5b=1e-10)  # tests/test_oracle_vs_reference_goldens.py: 1e-7 at omega = 1 - 1e-6
EPS = np.finfo(float).eps


def _columns(case):
    for i, kw in enumerate(case.columns):
        yield kw, (case.tau[i] if case.batch else case.tau), {o: (t[i] if case.batch else t) for o, t in case.truth.items()}


def test_fixture_set_is_the_catalogue():
    have = sorted(f[:-4] for f in os.listdir(NC.NT_DIR) if f.endswith(".npz"))
    assert have == sorted(NC.WELL_CONDITIONED + NC.NEAR_NODE)
    assert set(MEASURED) == set(NC.WELL_CONDITIONED) and set(MEASURED_NEAR_NODE) == set(NC.NEAR_NODE)
    assert all(10 * v <= CEILING for v in MEASURED.values())


def test_arbiter_shares_no_code_with_oracle_or_package():
    src = open(os.path.join(goldens.HERE, "..", "tools", "nt_truth.py")).read()
    imports = [ln.split()[1].split(".")[0] for ln in src.splitlines() if ln.startswith(("import ", "from "))]
    assert sorted(set(imports)) == ["mpmath", "numpy"]


@pytest.mark.parametrize("order", NC.ORDERS)
@pytest.mark.parametrize("name", NC.WELL_CONDITIONED)
def test_oracle_terms_against_truth(name, order):
    case = NC.load(name)
    for kw, tau, truth in _columns(case):
        got = NC.oracle_terms(kw, tau, case.phi, order)
        assert np.all(np.isfinite(got))
        d = NC.distance(got, truth[order])
        print(f"{name} {order}: {d:.2e}")
        assert d <= 10 * MEASURED[name]


@pytest.mark.parametrize("order", NC.ORDERS)
@pytest.mark.parametrize("name", NC.NEAR_NODE)
def test_oracle_terms_near_a_node(name, order):
    """Here the reference's float64 formulas lose digits; the figure is the loss itself, not a bound the formulas ought to keep."""
    case = NC.load(name)
    d = NC.distance(NC.oracle_terms(case.columns[0], case.tau, case.phi, order), case.truth[order])
    print(f"{name} {order}: {d:.2e}")
    assert d <= 10 * MEASURED_NEAR_NODE[name]


@pytest.mark.parametrize("name", NC.TEST_PROBLEMS)
def test_test_problems_three_way(name):
    """Oracle u(NT on) - u(NT off) and the reference's captured u minus the oracle's u(NT off), both against the truth: this is
    what certifies the NT part of tests/golden/hp/golden_<4a|4b|5a|5b>.npz, which tools/hp_truth_case.py formed as the first of
    the two differences.  A difference of two u carries the rounding of u: 4 eps max|u| (two roundings per operand)."""
    from oracle import disort_oracle as O
    case = NC.load(name)
    kw = case.columns[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        on, off = O.pydisort(NT_cor=True, **kw)[4], O.pydisort(NT_cor=False, **kw)[4]
    for order in NC.ORDERS:
        u_off = off(case.tau, case.phi, **NC.ORACLE_KW[order])
        corr = on(case.tau, case.phi, **NC.ORACLE_KW[order]) - u_off
        truth = case.truth[order]
        err = np.max(np.abs(corr - truth))
        print(f"{name} {order}: on - off vs truth {err / np.max(np.abs(truth)):.2e} of max|truth|")
        assert err <= 10 * MEASURED[name] * np.max(np.abs(truth)) + 4 * EPS * np.max(np.abs(u_off))
    call = goldens.load(name[3:])[0]
    ev = next(e for e in call["evals"] if e["name"] == "u" and not e["kwargs"] and len(e["args"]) == 2)
    assert np.array_equal(np.atleast_1d(ev["args"][0]), case.tau) and np.array_equal(np.atleast_1d(ev["args"][1]), case.phi)
    ref_u = np.asarray(ev["out"]).reshape(case.truth["value"].shape)
    err = np.max(np.abs(ref_u - off(case.tau, case.phi) - case.truth["value"])) / np.max(np.abs(ref_u))
    print(f"{name}: reference golden - oracle u(NT off) vs truth {err:.2e} of max|u|")
    assert err <= GOLDEN_TOL[name]


def test_thick_atmosphere_oracle_finite_where_reference_is_not():
    """q32_L20_thick (20 layers, total optical depth 268): the reference's cumulative sums divide by a product of attenuations that
    has underflowed (pydisort.py:531-534, :575-578), so its corrected u has NaN there; the fixture records how many when it was made.
    The oracle's direct sums stay finite (and within MEASURED of the truth, above)."""
    case = NC.load("q32_L20_thick")
    assert int(case.z["reference_nonfinite"]) > 0 and int(case.z["reference_size"]) == case.truth["value"].size
    for order in NC.ORDERS:
        assert np.all(np.isfinite(NC.oracle_terms(case.columns[0], case.tau, case.phi, order)))
        assert np.all(np.isfinite(case.truth[order]))


@pytest.mark.parametrize("name", ["q6_L1", "q16_L7_mixed"])
def test_fixtures_regenerate_bit_for_bit(name):
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_nt_truth_goldens", os.path.join(goldens.HERE, "golden", "make_nt_truth_goldens.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    res = gen.build(name)
    z = np.load(os.path.join(NC.NT_DIR, name + ".npz"))
    assert sorted(z.files) == sorted(res)
    for k in z.files:
        a = np.asarray(res[k])
        assert a.shape == z[k].shape and a.astype(z[k].dtype).tobytes() == z[k].tobytes(), k
