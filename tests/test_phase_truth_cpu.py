"""The inputs of tests/phase_cases.py and their 40-digit fixtures (tests/golden/hp/phase_*.npz, tools/hp_truth_case.py phase ...),
checked on the CPU:

* every case has its fixture, at the case's own points and below 200 KB;
* every truncation is a phase function (non-negative over 4001 angles), the one deliberate exception aside;
* on the columns without a near-conservative layer (c2, c3, c4) the float64 oracle -- an independent restatement of the reference's
  equations -- is within 1e-9 of the scale of the truth up to 64 streams, and within ten times its measured distance at 66 ... 126: the
  40-digit machinery handles zeros, negative moments and tabulated Mie moments;
* on c0, c1, c5 and the six-layer column deep (an omega = 1 - 1e-6 layer) the oracle's distance is recomputed and must match the fixture's own record to 5 %
  (the convention of test_reference_algorithm_is_beyond_the_north_star_on_these_atmospheres); no upper bound is asked of the
  oracle there: at 62 ... 128 streams it is 6e-8 ... 1e-4 away, which is why these cases need a 40-digit arbiter."""
import os
import warnings

import numpy as np
import pytest

import goldens
import phase_cases as P
from oracle import disort_oracle as O

# the oracle's distance from the truth at 126 streams, of the scale, the worst of the five quantities (u0 in all three; u itself:
# 1.02e-9, 6.5e-11, 4.5e-9; the fluxes <= 1.7e-11) -- measured on the CPU; the bound is ten times it.  (62 streams: 2.0e-11,
# 1.5e-10, 4.5e-10.)
ORACLE_AT_126 = {"126_c2": 1.02e-9, "126_c3": 2.42e-10, "126_c4": 1.24e-8}
# the same at the stream counts of P.PADDED beyond 64, measured the same way (u0 or u the worst; the fluxes <= 8.3e-12)
ORACLE_BEYOND_64 = {
    "66_c2": 2.13e-10, "66_c3": 2.79e-10, "66_c4": 5.47e-10,
    "94_c2": 7.22e-10, "94_c3": 1.93e-10, "94_c4": 1.48e-9,
    "96_c2": 8.25e-10, "96_c3": 7.73e-10, "96_c4": 1.44e-9,
    "98_c2": 7.99e-10, "98_c3": 1.16e-9, "98_c4": 5.00e-9,
}
ORACLE_BEYOND_64.update(ORACLE_AT_126)

_ORACLE = {}


def oracle(key):
    """The oracle's five quantities at the case's points, computed once per case."""
    if key not in _ORACLE:
        kw = P.case(key)
        tau, phi = P.points(kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = O.pydisort(**kw)
            fd = ref[2](tau)
            _ORACLE[key] = dict(u=ref[4](tau, phi), u0=ref[3](tau), flux_up=ref[1](tau), flux_down_diffuse=fd[0], flux_down_direct=fd[1])
    return _ORACLE[key]


def test_the_case_list_is_what_it_says():
    keys = P.keys()
    assert len(keys) == 79 and len(set(keys)) == 79  # 5 x 6 + 5, the 7 x 6 of PADDED, the two deep ones
    assert sorted(k for k in keys if k.endswith("_deep")) == ["126_deep", "94_deep"]
    for key in keys:
        kw = P.case(key)
        NQuad = kw["NQuad"]
        L = len(kw["tau_arr"])
        # three layers up to 64 streams, two beyond; the one exception: the deep column has six
        assert L == (6 if key.endswith("_deep") else 3 if NQuad <= 64 else 2)
        assert kw["NFourier"] == 3 and kw["Leg_coeffs_all"].shape == (L, NQuad + 1) and len(kw["omega_arr"]) == L
        assert np.all(np.diff(np.concatenate(([0.0], kw["tau_arr"]))) > 0)
        near = bool(np.any(kw["omega_arr"] > 1 - 1e-5))
        assert near == (key.split("_")[1] in P.NEAR_CONSERVATIVE)
        assert not (near and "s_poly_coeffs" in kw)  # no thermal source beside a near-conservative layer
    for NQuad in P.DEEP:
        kw = P.case(f"{NQuad}_deep")
        assert np.allclose(np.diff(np.concatenate(([0.0], kw["tau_arr"]))), [0.3, 0.8, 1e-3, 0.9, 9.0, 2.0], rtol=1e-12)
        assert np.array_equal(kw["omega_arr"], [0.95, 1 - 1e-6, 0.5, 1 - 1e-6, 0.9, 0.0])
        assert np.array_equal(kw["f_arr"] > 0, [False, True, False, False, True, False])
        assert np.array_equal(kw["f_arr"][[1, 4]], kw["Leg_coeffs_all"][[1, 4], NQuad])
    for NQuad in P.FULL + P.PADDED:
        q = P.case(f"{NQuad}_c4")["BDRF_Fourier_modes"]
        mu = np.linspace(0.1, 0.9, 5)
        assert len(q) == 2 and all(not np.allclose(f(mu, mu), f(mu, mu).T) for f in q)  # a non-symmetric table in both modes
        assert np.count_nonzero(P.case(f"{NQuad}_c4")["Leg_coeffs_all"][0]) == 5
        c5 = P.case(f"{NQuad}_c5")["Leg_coeffs_all"][-2]
        assert np.ptp(c5[2:NQuad] / c5[1:NQuad - 1]) > 0.05  # cloud C1: tabulated Mie moments, no geometric sequence
        assert np.all(P.case(f"{NQuad}_c2")["Leg_coeffs_all"][:, 1] < 0)
        c3 = P.case(f"{NQuad}_c3")
        assert np.array_equal(c3["f_arr"], c3["Leg_coeffs_all"][:, NQuad]) and np.all(c3["f_arr"] > 0)


def test_every_case_has_its_fixture_at_its_own_points():
    for key in P.keys() + [P.NEGATIVE]:
        path = P.fixture_path(key)
        assert os.path.exists(path), f"run tools/hp_truth_case.py phase {key}"
        assert os.path.getsize(path) < 200_000, (path, os.path.getsize(path))
        kw = P.case(key)
        tau, phi = P.points(kw)
        z = np.load(path)
        assert np.array_equal(z["tau"], tau) and np.array_equal(z["phi"], phi)
        assert len(tau) == 2 * len(kw["tau_arr"]) + 1  # the top, every interface, the bottom, one interior point per layer
        Q = kw["NQuad"]
        assert z["u"].shape == (Q, len(tau), 3) and z["u0"].shape == (Q, len(tau))
        for k in ("flux_up", "flux_down_diffuse", "flux_down_direct"):
            assert z[k].shape == (len(tau),) and np.all(np.isfinite(z[k]))
        assert np.all(np.isfinite(z["u"])) and np.max(np.abs(z["u"])) > 0


def test_every_truncation_is_a_phase_function():
    for key in P.keys():
        m = P.truncation_minimum(P.case(key))
        assert np.all(m >= 0), (key, m)
    assert P.truncation_minimum(P.case(P.NEGATIVE))[1] < -0.2  # the deliberate exception: -0.25 in the middle layer


def test_the_largest_parameters_of_the_smaller_stream_counts_would_not_be():
    """(-0.6)^l and 0.8 0.8^l + 0.2 (-0.5)^l are phase functions at 16 terms and not at 8: why g, g1, g2 shrink with the stream count."""
    for leg in (lambda n: P.henyey_greenstein(-0.6, n), lambda n: P.double_henyey_greenstein(0.8, 0.8, -0.5, n)):
        assert P.truncation_minimum(dict(NQuad=16, Leg_coeffs_all=leg(17)))[0] > 0
        assert P.truncation_minimum(dict(NQuad=8, Leg_coeffs_all=leg(9)))[0] < 0


@pytest.mark.parametrize("key", [f"{q}_{c}" for q in P.FULL + P.PADDED for c in ("c2", "c3", "c4")])
def test_oracle_and_truth_agree_where_float64_can(key):
    z = np.load(P.fixture_path(key))
    got = oracle(key)
    NQuad = int(key.split("_")[0])
    if NQuad <= 64:
        bound = 1e-9
    else:
        bound = 10 * ORACLE_BEYOND_64[key]
    for k in ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct"):
        a, _ = goldens.max_rel_err(got[k], z[k])
        print(f"{key} {k}: oracle {a:.3e} of the scale of the truth (bound {bound:.1e})")
        assert a < bound, (key, k, a)


@pytest.mark.parametrize("key", [k for k in P.keys() if k.split("_")[1] in P.NEAR_CONSERVATIVE] + [P.NEGATIVE])
def test_oracle_distance_on_the_near_conservative_columns_is_the_recorded_one(key):
    z = np.load(P.fixture_path(key))
    a, b = goldens.max_rel_err(oracle(key)["u"], z["u"])
    print(f"{key}: oracle {a:.3e} of the scale, {b:.3e} pointwise")
    assert abs(a - float(z["oracle_u_scale_rel"])) <= 0.05 * a
    assert abs(b - float(z["oracle_u_pointwise_rel"])) <= 0.05 * b


def test_flux_down_of_the_fixtures_is_the_truths_own():
    """Both parts of flux_down are formed from the truth's u0 and the direct beam's closed form: the diffuse part plus the direct
    part is the quadrature sum over the downward streams plus the delta-scaled beam, whatever the delta-M scaling moved."""
    for key in ("14_c3", "30_c5", "6_c2"):
        kw = P.case(key)
        tau, _ = P.points(kw)
        z = np.load(P.fixture_path(key))
        N = kw["NQuad"] // 2
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            p = O.prepare(**kw)
        mu, w = p["mu"], p["W"]
        total = z["flux_down_diffuse"] + z["flux_down_direct"]
        quad = 2 * np.pi * (mu * w) @ z["u0"][N:]
        assert np.allclose(z["flux_down_direct"], kw["I0"] * kw["mu0"] * np.exp(-tau / kw["mu0"]), rtol=1e-15, atol=0)
        assert np.all(total - quad >= -1e-15) and np.all(total - quad <= kw["I0"] * kw["mu0"] + 1e-15)
        if "f_arr" not in kw:
            assert np.allclose(z["flux_down_diffuse"], quad, rtol=1e-14, atol=1e-16)
