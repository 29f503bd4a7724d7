"""CPU side of the deep thermal source polynomials (tests/thermal_deep_cases.py): the 40-digit tool's thermal family is pinned on
fixtures it did not write, every thermal fixture meets the conditions that make it a test of what it is named for, and both roads
from the user's polynomials to the coefficients the kernels use -- the front end's and the device preparation's arithmetic, compiled
for the host -- are held to exact rationals by a bound derived from the arithmetic as written."""
import os
import shutil
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import phase_cases
import thermal_deep_cases as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = Fraction(1, 2**53)  # unit roundoff


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import hp_truth_case
    finally:
        sys.path.pop(0)
    return hp_truth_case


@pytest.mark.parametrize("key", [f"{q}_{c}" for q in (6, 14, 30) for c in ("c2", "c3")])
def test_thermal_family_of_the_truth_tool_reproduces_the_shallow_phase_fixtures(key):
    """The thermal family forms the source about each layer's top from the RAW polynomials in exact arithmetic and evaluates the
    particular solution in the local variable; the phase family took the float64 coefficients in the absolute scaled depth.  On
    shallow columns (tau <= 2; c2 linear without delta-M, c3 quadratic with delta-M and a beam) the two formulations are the same
    numbers: the committed fixtures, written by the other path, are reproduced to 1e-14 of the scale."""
    H = _tool()
    kw = phase_cases.case(key)
    z = np.load(phase_cases.fixture_path(key))
    sol = H.solve_thermal(([kw], z["tau"]))[0]
    for name in ("u0", "flux_up"):
        got, want = sol[name][0], z[name]
        assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(want)), (key, name)


@pytest.mark.parametrize("key", TD.keys())
def test_thermal_fixture_meets_its_conditions(key):
    """Conditions, not measurements: R <= 1e4 (the largest single term of the particular solution over the field's scale: float64 can
    reach 1e-12 of the scale); the deep fixtures (degree 13 with delta-M, Ns = 17 and 20) record a loss >= 1e-6 of the source for
    the float64 substitution tau* = scale tau + shift, and those of Ns = 17 and 20 a loss >= 1e-7 for plain float64 Horner -- a
    regression to either defect is then at least 100 x the GPU ceiling of 1e-9."""
    path = TD.fixture_path(key)
    assert os.path.exists(path), f"python tools/hp_truth_case.py thermal {key}"
    z = np.load(path)
    kw = TD.case(key)
    assert np.array_equal(z["tau"], TD.points(kw))
    Q = kw["NQuad"]
    for order in ("", "derivative.", "antiderivative."):
        assert z[order + "u0"].shape == (Q, len(z["tau"])) and np.all(np.isfinite(z[order + "u0"]))
        assert z[order + "flux_up"].shape == z[order + "flux_down_diffuse"].shape == z["tau"].shape
    assert float(z["R"]) <= 1e4
    name = key.split("_")[1]
    if name in TD.DEEP:
        assert float(z["loss_substitution"]) >= 1e-6, float(z["loss_substitution"])
    if name[0] == "d" and TD.degree(name) + 1 in (17, 20):
        assert float(z["loss_horner"]) >= 1e-7, float(z["loss_horner"])
    if TD.degree(name) == 1:  # linear sources lose nothing on any road
        assert float(z["loss_substitution"]) <= 1e-13 and float(z["oracle_u0_scale_rel"]) <= 1e-9


def _bound(Ns):
    """Roundings of a coefficient on its way from the user's polynomial to the uploaded one (csrc/rtd_dd.h: rtd_source_local;
    _prepare.py): the double-double shift delivers the exact coefficient rounded twice at the most (2 u); coefficient i is
    multiplied by sc^-i, built from i products of the rounded reciprocal (2 i u) -- one more for the product itself; (1 - omega)
    and its product with 1 / sc (3 u) and the multiplication by it (1 u); the division by the rescale factor and the product with
    it that undoes it here (2 u).  9 + 2 i <= 7 + 2 Ns units, first order; 1.01 covers the second."""
    return 1.01 * (7 + 2 * Ns) * U


def _front_end_local(kw):
    """The local scaled source polynomials [L][Ns] the front end's ``prepare_columns`` leads to (in the units of the inputs): its
    s_local where it forms them itself, else its s_s -- the reference's coefficients in the absolute scaled depth -- Taylor-shifted
    to the tops of the layers as rtd_plan_set_columns does (csrc/rtd_dd.h compiled for the host: tests/cpu/dd_shift.cpp)."""
    from pydisort_amd._prepare import prepare_columns
    from test_host_logic import _dd_shift
    L, N = len(kw["tau_arr"]), kw["NQuad"] // 2
    q = prepare_columns(kw["tau_arr"][None], kw["omega_arr"][None], kw["NQuad"], kw["Leg_coeffs_all"][None], [kw["mu0"]], [kw["I0"]],
                        [kw["phi0"]], kw["NQuad"], 1, np.full((1, N, 1), kw["b_pos"]), np.full((1, N, 1), kw["b_neg"]),
                        kw["f_arr"][None], kw["s_poly_coeffs"][None], np.full((1, 1, N, N), TD.SURFACE), np.full((1, 1, N), TD.SURFACE))
    if q.get("s_local") is not None:
        loc = q["s_local"][0]
    else:
        Ns = q["s_s"].shape[2]
        loc = np.array(_dd_shift([(Ns, float(q["tau_s0"][0, l]), q["s_s"][0, l].tolist()) for l in range(L)]))
    return loc * q["rescale"][0]


@pytest.mark.parametrize("name", ["d1", "d3", "d5", "d9", "d13", "d16", "d19", "n5", "n13", "n19", "thin"])
def test_front_end_source_polynomials_against_exact_rationals(name):
    """The scaled source the kernels see, evaluated across every layer in exact arithmetic, against the one the user's float64
    polynomials define: within (7 + 2 Ns) u of the sum of the absolute values of the LOCAL terms.  The float64 substitution
    tau* = scale tau + shift of the reference misses this by seven orders at degree 9 and optical depth 90."""
    key = ("16_" if name == "d16" else "6_") + name
    kw = TD.case(key)
    exact, width = TD.exact_local_scaled(kw)
    got = _front_end_local(kw)
    if got.shape[1] < 3:
        # A linear source keeps the reference's arithmetic to the bit: tau* = scale tau + shift in float64, whose roundings are
        # units of the ABSOLUTE terms (1 - omega) / sc (|a_0| + |a_1| tau) -- 2 top / thickness + 1 = 60 local ones at the most
        # here, which is why it may stay.  The shift is a running sum over the layers (L u of tau*); the substitution, the factor and
        # the rescale factor add eight roundings.
        L = len(exact)
        for l in range(L):
            a = [abs(Fraction(float(v))) for v in kw["s_poly_coeffs"][l]]
            sc = Fraction(float(1.0 - kw["omega_arr"][l] * kw["f_arr"][l]))
            size = (1 - Fraction(float(kw["omega_arr"][l]))) / sc * (a[0] + a[1] * Fraction(float(kw["tau_arr"][l])))
            for x in (0, width[l] / 2, width[l]):
                err = abs(sum((Fraction(float(g)) - e) * x**i for i, (g, e) in enumerate(zip(got[l], exact[l]))))
                assert err <= (L + 8) * U * size, (key, l, float(err / size / U))
        return
    _, worst = TD.source_error(got, exact, width)
    print(f"front end {key}: {worst / float(U):.2f} u of the local terms (bound {float(_bound(got.shape[1]) / U):.1f} u)")
    assert worst <= float(_bound(got.shape[1])), (key, worst)


@pytest.mark.parametrize("name", ["d3", "d9", "d13", "d16", "d19", "n19"])
def test_device_preparation_arithmetic_against_exact_rationals(name):
    """rtd_source_local -- what rtd_prepare_columns_kernel runs per layer -- compiled for the host in a stand-alone program
    (tests/cpu/source_local.cpp) on the same columns, held to the same bound (less the two roundings of the rescale factor)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    key = ("16_" if name == "d16" else "6_") + name
    kw = TD.case(key)
    exact, width = TD.exact_local_scaled(kw)
    L, Ns = kw["s_poly_coeffs"].shape
    top = np.concatenate(([0.0], kw["tau_arr"][:-1]))
    sc = 1.0 - kw["omega_arr"] * kw["f_arr"]
    text = "".join(f"{Ns} {float(top[l])!r} {float(sc[l])!r} {float(kw['omega_arr'][l])!r} "
                   + " ".join(repr(float(x)) for x in kw["s_poly_coeffs"][l]) + "\n" for l in range(L))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "source_local")
        subprocess.run([gxx, "-O1", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpu", "source_local.cpp"), "-o", exe],
                       check=True)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    got = np.array([[float(x) for x in line.split()] for line in out])
    assert got.shape == (L, Ns)
    _, worst = TD.source_error(got, exact, width)
    print(f"device arithmetic {key}: {worst / float(U):.2f} u of the local terms")
    assert worst <= float(_bound(Ns) - 2 * U), (key, worst)
