"""The test-side truth of the actinic fluxes (tests/actinic_cases.py: the oracle's u0 and the closed forms of include/rtd.h) held
to the reference's own ``generate_diff_act_flux_funcs`` (fixtures tests/golden/actinic/*.npz, written by
tests/golden/make_actinic_goldens.py): the project's standing 1e-9 of the field scale, values and tau-antiderivatives, at tau = 0,
every interface, mid-layer points and the bottom.

In every fixture but "rescaled" the reference's rescale factor is 1.  "rescaled" (I0 = 2.5, b_pos = 0.1) documents the one
deviation: the reference forms the delta-M reclassification term R with the I0 it has divided by its
rescale factor and does not multiply back, so its flux_act_down_diffuse is low by R (1 - 1 / rescale) -- by that and by nothing
else.

Figures seen (each case prints its own): 7e-17 ... 2.3e-13 of the field scale (the largest at 34 streams and six layers);
"rescaled" 5.3e-15 and 1.5e-14 once the term is added, 3.0e-3 and 1.2e-3 before."""
import numpy as np
import pytest

import actinic_cases as A

TOL = 1e-9
CASES = A.cases()


def _scale_err(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_truth_matches_the_reference(name):
    kw, z = CASES[name], A.load(name)
    for k in ("tau_arr", "omega_arr", "f_arr"):  # the fixture belongs to this case
        assert np.array_equal(z[k], np.asarray(kw[k], float)), k
    assert float(z["mu0"]) == kw["mu0"] and float(z["I0"]) == kw["I0"] and int(z["NQuad"]) == kw["NQuad"]
    tau = z["tau"]
    assert np.array_equal(tau, A.points(kw)) and tau[0] == 0.0 and tau[-1] == kw["tau_arr"][-1]
    sol = A.solve(kw)
    rescale = float(sol.p["rescale"])
    assert (rescale != 1.0) == (name in A.RESCALED), rescale
    for suffix, order in (("", 0), (".antider", -1)):
        if order and name in A.VALUE_ONLY:
            assert "flux_act_up.antider" not in z.files
            continue
        t = A.truth(kw, tau, order, sol)
        up = _scale_err(t["flux_act_up"], z["flux_act_up" + suffix])
        want_dn = z["flux_act_down_diffuse" + suffix]
        if name in A.RESCALED:
            R, _ = A.reclassification(sol.p, float(kw["I0"]), tau, order)
            assert np.max(np.abs(R)) > 1e-3 * np.max(np.abs(want_dn))  # (the deviation is far above the bar: it is being tested)
            raw = _scale_err(t["flux_act_down_diffuse"], want_dn)
            assert raw > 1e3 * TOL, raw
            want_dn = want_dn + R * (1.0 - 1.0 / rescale)
            print(f"ACTINIC {name}{suffix}: the reference's down-diffuse differs by {raw:.2e} of the scale before the R (1 - 1/rescale) term")
        dn = _scale_err(t["flux_act_down_diffuse"], want_dn)
        print(f"ACTINIC {name}{suffix}: up {up:.2e}, down diffuse {dn:.2e} of the field scale (bar {TOL:.0e})")
        assert up < TOL and dn < TOL, (name, suffix, up, dn)


def test_no_beam_has_no_reclassification_and_no_direct_part():
    kw = CASES["L3_q6_no_beam"]
    for order in A.ORDERS:
        t = A.truth(kw, A.points(kw), order)
        assert np.all(t["flux_act_down_direct"] == 0.0) and np.all(np.isfinite(t["flux_act_down_diffuse"]))


def test_direct_part_is_the_direct_flux_over_mu0():
    """act_down_direct = flux_down_direct / mu0, in all three orders (the oracle's flux_down is pinned to the reference elsewhere)."""
    kw = CASES["L3_q16"]
    sol, tau = A.solve(kw), A.points(kw)
    for order in A.ORDERS:
        direct = sol.flux_down(tau, order < 0, is_derivative_wrt_tau=order > 0)[1]
        got = A.truth(kw, tau, order, sol)["flux_act_down_direct"]
        assert np.max(np.abs(got - direct / kw["mu0"])) <= 4 * np.finfo(float).eps * np.max(np.abs(got))
