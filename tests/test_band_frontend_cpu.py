"""pydisort_band / solve_band_streamed / band_mix: what the Python layer does before anything touches the device -- validation
messages in the style of pydisort_batch, the shapes of I0 / weights / levels / per-profile arrays, the level -> tau table, and the
layers' net flux convergence on synthetic reduced arrays.  The library is needed for symbol presence only."""
import inspect
import re

import numpy as np
import pytest

P, G, S, L, NQ = 3, 5, 2, 3, 8


def _kw(**over):
    rng = np.random.default_rng(5)
    kw = dict(dtau_abs=rng.uniform(0.0, 0.5, (P, G, L)), dtau_spec=rng.uniform(0.05, 0.4, (P, L, S)),
              omega_spec=rng.uniform(0.1, 1.0, (P, L, S)), Leg_spec=np.array([0.7, 0.3])[:, None] ** np.arange(NQ + 1)[None, :],
              NQuad=NQ, mu0=0.6, I0=1.0, phi0=0.0, weights=np.full(G, 0.2))
    kw["dtau_abs"][:, 0, :] += 0.01
    kw.update(over)
    return kw


def _inputs(**over):
    from pydisort_amd import band
    kw = _kw(**over)
    names = list(inspect.signature(band._band_inputs).parameters)
    defaults = dict(NLeg=None, NFourier=None, delta_M=True, only_flux=False, b_pos=0, b_neg=0, bdrf_q=None, bdrf_q0=None, thermal=None)
    return band._band_inputs(*[kw.get(n, defaults.get(n)) for n in names])


def test_the_public_names_and_signatures_exist():
    import pydisort_amd
    from pydisort_amd import _lib
    for name in ("pydisort_band", "solve_band_streamed", "band_mix", "BandSolution"):
        assert name in pydisort_amd.__all__ and hasattr(pydisort_amd, name)
    want = ["dtau_abs", "dtau_spec", "omega_spec", "Leg_spec", "NQuad", "mu0", "I0", "phi0", "weights"]
    assert list(inspect.signature(pydisort_amd.pydisort_band).parameters)[:9] == want
    streamed = inspect.signature(pydisort_amd.solve_band_streamed).parameters
    assert list(streamed)[:9] == want and {"levels", "phi", "chunk_columns"} <= set(streamed)
    for k in ("NLeg", "NFourier", "delta_M", "only_flux", "b_pos", "b_neg", "bdrf_q", "bdrf_q0", "thermal", "device", "work_columns",
              "numeric_errors", "retain", "retain_bytes"):
        assert k in inspect.signature(pydisort_amd.pydisort_band).parameters, k
    for sym in ("rtd_band_mix", "rtd_plan_set_columns_band", "rtd_plan_set_band_weights", "rtd_plan_fetch_band", "rtd_plan_evaluate_band"):
        assert sym in _lib.SIGNATURES and hasattr(_lib.load(), sym)
    assert _lib.load().rtd_version() >= 213
    assert [n for n, _ in _lib.rtd_band._fields_] == ["nprofiles", "ngpoints", "nspecies", "nleg_all", "delta_m", "dtau_abs", "dtau_spec",
                                                      "omega_spec", "leg_spec"]
    for m in ("set_columns_band", "set_band_weights", "fetch_band", "evaluate_band"):
        assert hasattr(pydisort_amd._Plan, m)


BAD = [
    (dict(dtau_abs=np.ones((P, L))), "dtau_abs must have the shape [P, G, L]"),
    (dict(dtau_spec=np.ones((P, L + 1, S))), "dtau_spec must have the shape"),
    (dict(omega_spec=np.ones((P, L, S + 1)) * 0.5), "omega_spec must have the shape of dtau_spec"),
    (dict(Leg_spec=np.ones((S + 1, NQ + 1))), "Leg_spec must have the shape"),
    (dict(NQuad=7), "NQuad must be even"),
    (dict(NLeg=NQ + 2), "Need 0 < NFourier <= NLeg <= NQuad"),
    (dict(Leg_spec=np.array([0.7, 0.3])[:, None] ** np.arange(NQ)[None, :]), "delta_M needs more Legendre coefficients"),
    (dict(dtau_abs=-np.ones((P, G, L))), "must not be negative"),
    (dict(omega_spec=np.full((P, L, S), 1.5)), "albedo of every species must be between 0 and 1"),
    (dict(Leg_spec=0.9 * np.array([0.7, 0.3])[:, None] ** np.arange(NQ + 1)[None, :]), "zeroth Legendre coefficient"),
    (dict(dtau_abs=np.zeros((P, G, L)), dtau_spec=np.zeros((P, L, S))), "positive optical thickness"),
    (dict(dtau_abs=np.zeros((P, G, L)), omega_spec=np.ones((P, L, S))), "albedo of the mixture"),
    (dict(weights=np.ones(G + 1)), "weights must have the shape"),
    (dict(weights=np.ones((2, 2, G))), "weights must have the shape"),
    (dict(mu0=np.full(G, 0.5)), "mu0 must be a scalar or [P"),
    (dict(phi0=np.zeros((P, G))), "phi0 must be a scalar or [P"),
    (dict(I0=np.ones(G + 2)), "I0 must be a scalar, [G"),
    (dict(I0=-1.0), "Need I0 >= 0"),
    (dict(mu0=1.5), "Need I0 >= 0 and 0 < mu0 <= 1"),
    (dict(b_pos=np.ones(P + 1)), "b_pos must be given per profile"),
    (dict(b_neg=np.ones((P, NQ // 2 + 1))), "b_neg must be given per profile"),
    (dict(bdrf_q=np.ones((P, 1, 4, 4))), "Give bdrf_q and bdrf_q0 together"),
    (dict(bdrf_q=np.ones((P, 1, 3, 4)), bdrf_q0=np.ones((P, 1, 4))), "bdrf_q must have the shape"),
    (dict(thermal=dict(TEMPER=np.ones(L + 1))), "thermal: WVNMLO is required"),
    (dict(thermal=dict(TEMPER=np.ones((P + 1, L + 1)), WVNMLO=1.0, WVNMHI=2.0)), "thermal: TEMPER must be given per profile"),
    (dict(thermal=dict(TEMPER=np.ones(L + 1), WVNMLO=1.0, WVNMHI=2.0, BTEMP=np.ones(4))), "thermal: BTEMP must be given per profile"),
]


@pytest.mark.parametrize("override,msg", BAD)
def test_invalid_band_inputs_raise_before_any_device_work(override, msg):
    with pytest.raises(ValueError, match=re.escape(msg)):
        _inputs(**override)


def test_the_mixture_is_checked_through_the_least_absorbing_point_only():
    """omega = 1 at ONE spectral point of one layer (no absorption there, conservative scatterers) is refused, although the other
    four points of that layer are fine; and no array of P G columns x NLeg moments is formed on the host."""
    a = np.full((P, G, L), 0.3)
    a[1, 3, 2] = 0.0
    om = np.full((P, L, S), 0.8)
    om[1, 2, :] = 1.0
    with pytest.raises(ValueError, match="albedo of the mixture"):
        _inputs(dtau_abs=a, omega_spec=om)
    a[1, 3, 2] = 1e-6
    prep, w, squeeze = _inputs(dtau_abs=a, omega_spec=om)
    biggest = max(np.asarray(v).size for d in (prep["band"], prep["cols"]) for v in d.values() if v is not None and not isinstance(v, bool))
    assert biggest == P * G * L


def test_shapes_of_I0_weights_and_per_profile_arrays():
    C, N = P * G, NQ // 2
    prep, w, squeeze = _inputs()
    assert squeeze and w.shape == (1, G) and (prep["C"], prep["L"], prep["N"], prep["P"], prep["M"], prep["Ns"], prep["NBDRF"]) == (C, L, N, NQ, NQ, 0, 0)
    assert prep["beam"] and prep["cols"]["b_pos"] is None and prep["band"]["delta_m"] is True
    assert np.array_equal(prep["cols"]["I0"], np.ones(C))
    # I0 per spectral point, per profile, per both: column p G + g
    g_vals, p_vals = np.arange(1.0, G + 1), 10.0 * np.arange(1.0, P + 1)
    assert np.array_equal(_inputs(I0=g_vals)[0]["cols"]["I0"], np.tile(g_vals, P))
    assert np.array_equal(_inputs(I0=p_vals)[0]["cols"]["I0"], np.repeat(p_vals, G))
    both = p_vals[:, None] + g_vals[None, :]
    assert np.array_equal(_inputs(I0=both)[0]["cols"]["I0"], both.reshape(C))
    assert np.array_equal(_inputs(mu0=np.array([0.3, 0.5, 0.7]))[0]["cols"]["mu0"], np.repeat([0.3, 0.5, 0.7], G))
    # weight sets
    w2 = np.arange(2.0 * G).reshape(2, G)
    prep, w, squeeze = _inputs(weights=w2)
    assert not squeeze and np.array_equal(w, w2)
    # only_flux and no delta-M scaling
    prep, _, _ = _inputs(only_flux=True, delta_M=False, Leg_spec=np.array([0.7, 0.3])[:, None] ** np.arange(NQ)[None, :])
    assert prep["M"] == 1 and prep["band"]["delta_m"] is False
    # boundary arrays per profile are repeated to the columns, per column are taken as they are; [., M, N] on the way to the library
    bp = np.arange(1.0, P + 1)
    prep, _, _ = _inputs(b_pos=bp, b_neg=np.arange(1.0, C + 1)[:, None] * np.ones((1, N)))
    assert prep["cols"]["b_pos"].shape == (C, NQ, N) and np.array_equal(prep["cols"]["b_pos"][:, 0, 0], np.repeat(bp, G))
    assert np.all(prep["cols"]["b_pos"][:, 1:] == 0) and np.array_equal(prep["cols"]["b_neg"][:, 0, 2], np.arange(1.0, C + 1))
    b3 = np.arange(1.0 * P * N * NQ).reshape(P, N, NQ)
    assert np.array_equal(_inputs(b_pos=b3)[0]["cols"]["b_pos"][G + 1], b3[1].T)
    q, q0 = np.arange(1.0 * P * 2 * N * N).reshape(P, 2, N, N), np.ones((C, 2, N))
    prep, _, _ = _inputs(bdrf_q=q, bdrf_q0=q0)
    assert prep["NBDRF"] == 2 and np.array_equal(prep["cols"]["bdrf_q"][2 * G + 4], q[2]) and prep["cols"]["bdrf_q0"].shape == (C, 2, N)
    # thermal: per profile, per column or shared
    th = dict(TEMPER=200.0 + np.arange(1.0 * P * (L + 1)).reshape(P, L + 1), WVNMLO=np.arange(1.0, C + 1), WVNMHI=5000.0, BTEMP=np.array([280.0, 290.0, 300.0]))
    prep, _, _ = _inputs(thermal=th)
    t = prep["thermal"]
    assert prep["Ns"] == 2 and t["TEMPER"].shape == (C, L + 1) and np.array_equal(t["TEMPER"][G], th["TEMPER"][1])
    assert np.array_equal(t["WVNMLO"], th["WVNMLO"]) and np.array_equal(t["BTEMP"], np.repeat(th["BTEMP"], G)) and t["TTEMP"] is None


def test_level_table_and_net_flux_convergence():
    from pydisort_amd import band
    tau = np.cumsum(np.arange(1.0, 1 + 4 * L).reshape(4, L), axis=1)
    table = band.level_tau(tau)
    assert table.shape == (4, L + 1) and np.all(table[:, 0] == 0) and np.array_equal(table[:, 1:], tau)
    assert np.array_equal(band.level_tau(tau, [L, 0, 2]), table[:, [L, 0, 2]]) and band.level_tau(tau, 1).shape == (4, 1)
    assert band.level_tau(tau, [0, L]).flags["C_CONTIGUOUS"]
    for bad in ([-1], [L + 1], [0.5], [[0, 1]], []):
        with pytest.raises(ValueError, match="levels must"):
            band.level_tau(tau, bad)
    # F_net = down - up at L + 1 levels -> what each layer keeps
    up = np.array([[[1.0, 2.0, 4.0, 8.0]]])
    dd = np.array([[[0.0, 3.0, 5.0, 6.0]]])
    dr = np.array([[[10.0, 7.0, 2.0, 1.0]]])
    conv = band.net_flux_convergence(up, dd, dr)
    assert conv.shape == (1, 1, L) and np.array_equal(conv[0, 0], [9.0 - 8.0, 8.0 - 3.0, 3.0 - (-1.0)])
    assert np.isclose(conv.sum(), (dd + dr - up)[0, 0, 0] - (dd + dr - up)[0, 0, -1])
