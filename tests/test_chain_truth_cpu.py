"""The inputs of tests/chain_cases.py and their 40-digit fixtures (tests/golden/hp/chain_*.npz, tools/hp_truth_case.py chain ...),
checked on the CPU:

* the case list is what it says: the key set, the layer counts, the five-layer pattern per offset, delta-M on the cloud layers only;
* every case has its fixture, at the case's own points, of the right shapes, finite and below 200 KB;
* every delta-M-scaled truncation is a phase function (non-negative over 4001 angles);
* the float64 oracle's distance from the truth, recomputed, matches the fixture's own record to 5 % (the convention of
  tests/test_phase_truth_cpu.py).  No upper bound is asked of the oracle: every chain carries omega = 1 - 1e-6 layers, and the oracle
  is 1.2e-10 (8 streams) ... 2.5e-5 (96) of the scale away, which is why these chains need a 40-digit arbiter;
* flux_down_direct is the closed form, and both parts of flux_down are the truth's own."""
import os
import warnings

import numpy as np
import pytest

import chain_cases as C
import goldens
import phase_cases as P
from oracle import disort_oracle as O

KEYS = ["8_L9", "10_L21", "14_L21", "16_L21", "18_L21", "30_L21", "32_L19", "32_L20", "32_L21", "32_L41", "34_L25", "62_L25",
        "64_L25", "66_L9", "96_L9", "98_L9", "128_L9"]
WITH_OFFSETS = ["16_L21", "32_L21", "64_L25", "96_L9"]


def test_the_case_list_is_what_it_says():
    keys = C.keys()
    assert len(keys) == 33 and len(set(keys)) == 33
    assert set(keys) == set(KEYS) | {f"{k}_s{s}" for k in WITH_OFFSETS for s in (1, 2, 3, 4)}
    assert C.BATCHES == tuple(C.parse(k)[:2] for k in WITH_OFFSETS) and C.OFFSETS == (0, 1, 2, 3, 4)
    thickness = np.array([0.3, 0.8, 1e-3, 2.5, 0.05])
    omega = np.array([1 - 1e-6, 0.9, 0.5, 1 - 1e-6, 0.0])
    for key in keys:
        NQuad, L, s = C.parse(key)
        assert key == C.key_of(NQuad, L, s) and key.startswith(f"{NQuad}_L{L}")
        kw = C.case(key)
        t = (np.arange(L) + s) % 5
        assert kw["NQuad"] == NQuad and kw["NFourier"] == 3 and kw["Leg_coeffs_all"].shape == (L, NQuad + 1)
        assert np.allclose(np.diff(np.concatenate(([0.0], kw["tau_arr"]))), thickness[t], rtol=1e-9)
        assert np.array_equal(kw["omega_arr"], omega[t])
        n = NQuad + 1
        for l in range(L):
            want = (P.rayleigh(n), P.cloud_c1(n), P.isotropic(n), P.rayleigh(n), P.isotropic(n))[t[l]]
            assert np.array_equal(kw["Leg_coeffs_all"][l], want)
        assert np.array_equal(kw["f_arr"] > 0, t == 1)  # delta-M on the cloud layers only
        assert np.array_equal(kw["f_arr"][t == 1], kw["Leg_coeffs_all"][t == 1, NQuad])
        assert (kw["mu0"], kw["I0"], kw["phi0"]) == (0.6, 2.0, 0.5) and kw["BDRF_Fourier_modes"] == [0.3]
        assert "s_poly_coeffs" not in kw  # no thermal source beside a near-conservative layer
        assert np.any(kw["omega_arr"] > 1 - 1e-5)
    # the window of rtd_bc_mfma_kernel: its last resident layer is non-scattering, the first refilled one near-conservative
    kw = C.case("32_L21")
    assert C.WINDOW == 20 and kw["omega_arr"][C.WINDOW - 1] == 0.0 and kw["omega_arr"][C.WINDOW] == 1 - 1e-6
    assert [C.parse(k)[1] for k in ("32_L19", "32_L20", "32_L21", "32_L41")] == [C.WINDOW - 1, C.WINDOW, C.WINDOW + 1, 2 * C.WINDOW + 1]


def test_the_window_constant_is_the_kernels():
    src = open(os.path.join(os.path.dirname(P.HERE), "pythonic-disort_amd", "csrc", "rtd_bc.hip")).read()
    assert f"#define RTD_BCF_WIN {C.WINDOW} " in src


def test_the_batches_stack_the_five_offsets():
    for NQuad, L in C.BATCHES:
        cfg, tau = C.batch_kwargs(NQuad, L)
        assert tau.shape == (5, 2 * L + 1)
        for s in C.OFFSETS:
            kw = C.case(C.key_of(NQuad, L, s))
            for k in ("tau_arr", "omega_arr", "Leg_coeffs_all", "f_arr"):
                assert np.array_equal(cfg[k][s], kw[k])
            assert np.array_equal(tau[s], C.points(kw)[0])
            assert (cfg["mu0"][s], cfg["I0"][s], cfg["phi0"][s]) == (kw["mu0"], kw["I0"], kw["phi0"])
        assert np.all(cfg["bdrf_q"] == 0.3) and np.all(cfg["bdrf_q0"] == 0.3) and cfg["bdrf_q"].shape == (5, 1, NQuad // 2, NQuad // 2)
        # unlike layers side by side: no two offsets have the same layer type anywhere
        assert all(len(set(cfg["omega_arr"][:, l])) >= 4 for l in range(L))


def test_every_case_has_its_fixture_at_its_own_points():
    for key in C.keys():
        path = C.fixture_path(key)
        assert os.path.exists(path), f"run tools/hp_truth_case.py chain {key}"
        assert os.path.getsize(path) < 200_000, (path, os.path.getsize(path))
        kw = C.case(key)
        tau, phi = C.points(kw)
        z = np.load(path)
        assert np.array_equal(z["tau"], tau) and np.array_equal(z["phi"], phi)
        assert len(tau) == 2 * len(kw["tau_arr"]) + 1  # the top, every interface, the bottom, one interior point per layer
        assert np.array_equal(tau[::2], C.interfaces(kw))
        Q = kw["NQuad"]
        assert z["u"].shape == (Q, len(tau), 3) and z["u0"].shape == (Q, len(tau))
        for k in ("flux_up", "flux_down_diffuse", "flux_down_direct"):
            assert z[k].shape == (len(tau),) and np.all(np.isfinite(z[k]))
        assert np.all(np.isfinite(z["u"])) and np.all(np.isfinite(z["u0"])) and np.max(np.abs(z["u"])) > 0


def test_every_truncation_is_a_phase_function():
    for key in C.keys():
        m = P.truncation_minimum(C.case(key))
        assert np.all(m >= 0), (key, m)


@pytest.mark.parametrize("key", C.keys())
def test_oracle_distance_is_the_recorded_one(key):
    z = np.load(C.fixture_path(key))
    kw = C.case(key)
    tau, phi = C.points(kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = O.pydisort(**kw)
        a, b = goldens.max_rel_err(ref[4](tau, phi), z["u"])
        c, _ = goldens.max_rel_err(ref[3](tau), z["u0"])
    print(f"chain {key}: oracle {a:.3e} of the scale, {b:.3e} pointwise; u0 {c:.3e}")
    assert abs(a - float(z["oracle_u_scale_rel"])) <= 0.05 * a
    assert abs(b - float(z["oracle_u_pointwise_rel"])) <= 0.05 * b
    assert abs(c - float(z["oracle_u0_scale_rel"])) <= 0.05 * c


def test_flux_down_of_the_fixtures_is_the_truths_own():
    """flux_down_direct is the closed form; the diffuse part plus the direct part is the quadrature sum over the downward streams plus
    the delta-scaled beam, whatever the delta-M scaling of the cloud layers moved."""
    for key in ("8_L9", "16_L21_s3", "32_L41", "64_L25", "128_L9"):
        kw = C.case(key)
        tau, _ = C.points(kw)
        z = np.load(C.fixture_path(key))
        N = kw["NQuad"] // 2
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            p = O.prepare(**kw)
        total = z["flux_down_diffuse"] + z["flux_down_direct"]
        quad = 2 * np.pi * (p["mu"] * p["W"]) @ z["u0"][N:]
        assert np.allclose(z["flux_down_direct"], kw["I0"] * kw["mu0"] * np.exp(-tau / kw["mu0"]), rtol=1e-15, atol=0)
        assert np.all(total - quad >= -1e-15) and np.all(total - quad <= kw["I0"] * kw["mu0"] + 1e-15)
        first_cloud = int(np.argmax(kw["f_arr"] > 0))
        above = tau <= np.concatenate(([0.0], kw["tau_arr"]))[first_cloud]  # above the first delta-M layer nothing was moved
        assert np.allclose(z["flux_down_diffuse"][above], quad[above], rtol=1e-13, atol=1e-15)
