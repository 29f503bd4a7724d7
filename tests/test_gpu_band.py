"""k-distribution bands on the device: pydisort_band / band_mix / Plan.fetch_band / Plan.evaluate_band
(include/rtd.h: rtd_band_mix, rtd_plan_set_columns_band, rtd_plan_set_band_weights, rtd_plan_fetch_band, rtd_plan_evaluate_band).

Shapes: 3 profiles x 5 spectral points, 2 scatterer species (Henyey-Greenstein + Rayleigh), 3 layers, 2 weight sets; 8, 16 and 32
streams.  Every bound is derived, none is measured:

* mixing: each output is a sum of at most S + L + 1 rounded terms and one division, all terms >= 0, so it is held to
  (S + L + 4) 2^-53 of its own 40-digit value (mpmath);
* the band entry gives the SAME BITS as pydisort_batch(device_prepare=True) fed with band_mix's arrays: same input bits, same
  kernels;
* reduction: exact products and G double-double additions, rounded once: one unit in the last place of the exact weighted sum
  (fractions.Fraction over the unreduced arrays of the same plan) plus 2^-90 sum_g |w x|;
* end to end against the CPU oracle on NumPy-mixed columns, NumPy-weighted: the project's standing 1e-9 of the field scale.

Figures seen on an MI355X (each test prints its own): mixing 2.17 ... 2.46 of the 9 units of 2^-53 allowed; reduction 0.500 ulp of
the 1 ulp + 2^-90 sum|w x| allowed, identical bits for one window and windows of 4; oracle 5.4e-13 (u), 5.1e-13 (u0), <= 1.7e-14
(fluxes) of the field scale, of the 1e-9 allowed."""
import functools
import math
from fractions import Fraction
from math import pi

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, G, S, L, K = 3, 5, 2, 3, 2
PHI = np.array([0.0, 1.0, pi])


@functools.lru_cache(maxsize=None)
def band(NQuad, dead_layer=False, thermal=False):
    """The band of every test (built once per shape and left unchanged): keyword arguments of pydisort_band without weights."""
    rng = np.random.default_rng(100 + NQuad)
    nleg_all = NQuad + 3
    k = np.arange(nleg_all)
    rayleigh = np.zeros(nleg_all)
    rayleigh[0], rayleigh[2] = 1.0, 0.1
    kw = dict(dtau_abs=rng.uniform(0.02, 0.6, (P, G, L)) * 10.0 ** rng.uniform(-1.0, 0.5, (P, G, 1)),
              dtau_spec=rng.uniform(0.05, 0.5, (P, L, S)), omega_spec=rng.uniform(0.5, 0.98, (P, L, S)),
              Leg_spec=np.stack((0.75 ** k, rayleigh)), NQuad=NQuad, mu0=rng.uniform(0.3, 0.9, P), I0=rng.uniform(0.5, 2.0, (P, G)),
              phi0=rng.uniform(0.0, 2 * pi, P), b_pos=rng.uniform(0.0, 0.3, P), b_neg=rng.uniform(0.0, 0.2, (P * G, NQuad // 2)))
    if dead_layer:
        kw["omega_spec"][1, 1, :] = 0.0  # profile 1, layer 1: nothing scatters
        kw["dtau_spec"][1, 1, 0] = 0.0
    if thermal:
        kw["thermal"] = dict(TEMPER=np.sort(rng.uniform(200.0, 300.0, (P, L + 1)), axis=1), WVNMLO=500.0, WVNMHI=900.0,
                             BTEMP=rng.uniform(280.0, 310.0, P), TTEMP=60.0, TEMIS=0.8)
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return kw


WEIGHTS = np.array([[2.5e-3, -7.0e2, 1.3, -4.0e-2, 9.1e2], [-1.0e3, 3.3e-3, 5.0e1, 6.2e-1, -8.0e-3]])


def numpy_mix(kw, NLeg, delta_M):
    """The definitions of include/rtd.h in NumPy: what a caller did on the host before."""
    t = kw["omega_spec"] * kw["dtau_spec"]
    sca = t.sum(axis=2)
    dtau = kw["dtau_spec"].sum(axis=2)[:, None, :] + kw["dtau_abs"]
    with np.errstate(invalid="ignore", divide="ignore"):
        leg = np.einsum("pls,sk->plk", t, kw["Leg_spec"][:, :NLeg + 1]) / sca[:, :, None]
    leg[sca == 0] = 0.0
    leg[:, :, 0] = 1.0
    f = leg[:, :, NLeg] if delta_M else np.zeros((P, L))
    rep = lambda a: np.repeat(a, G, axis=0)  # noqa: E731
    return (np.cumsum(dtau, axis=2).reshape(P * G, L), (sca[:, None, :] / dtau).reshape(P * G, L), rep(f), rep(leg[:, :, :NLeg]))


# ---- 3. mixing arithmetic -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NLeg,delta_M", [(8, True), (8, False), (32, True)])
def test_band_mix_against_forty_digits(NLeg, delta_M):
    import mpmath
    import pydisort_amd
    kw = band(NLeg, dead_layer=True)
    tau, om, f, leg = pydisort_amd.band_mix(kw["dtau_abs"], kw["dtau_spec"], kw["omega_spec"], kw["Leg_spec"], NLeg, delta_M=delta_M)
    assert tau.shape == om.shape == f.shape == (P * G, L) and leg.shape == (P * G, L, NLeg)
    mp = mpmath.mp.clone()
    mp.dps = 40
    bound = (S + L + 4) * mp.mpf(2) ** -53
    worst = mp.mpf(0)

    def hold(got, exact):
        nonlocal worst
        err = abs(mp.mpf(float(got)) - exact)
        assert err <= bound * exact, (float(got), exact)  # (every term is >= 0: the expression is its own sum of absolute values)
        if exact > 0:
            worst = max(worst, err / exact * mp.mpf(2) ** 53)

    for p in range(P):
        for l in range(L):
            t = [mp.mpf(float(kw["omega_spec"][p, l, s])) * mp.mpf(float(kw["dtau_spec"][p, l, s])) for s in range(S)]
            sca, ext = sum(t), sum(mp.mpf(float(kw["dtau_spec"][p, l, s])) for s in range(S))
            moments = [sum(t[s] * mp.mpf(float(kw["Leg_spec"][s, k])) for s in range(S)) / sca if sca > 0 else mp.mpf(0) for k in range(NLeg + 1)]
            for g in range(G):
                c = p * G + g
                hold(om[c, l], sca / (ext + mp.mpf(float(kw["dtau_abs"][p, g, l]))))
                hold(f[c, l], moments[NLeg] if delta_M else mp.mpf(0))
                assert leg[c, l, 0] == 1.0
                for k in range(1, NLeg):
                    hold(leg[c, l, k], moments[k])
        for g in range(G):
            run = mp.mpf(0)
            for l in range(L):
                run += sum(mp.mpf(float(kw["dtau_spec"][p, l, s])) for s in range(S)) + mp.mpf(float(kw["dtau_abs"][p, g, l]))
                hold(tau[p * G + g, l], run)
    assert np.all(leg[G:2 * G, 1, 1:] == 0.0) and np.all(f[G:2 * G, 1] == 0.0)  # the layer without a scatterer
    print(f"MIX NLeg {NLeg} delta_M {delta_M}: worst {float(worst):.2f} of {S + L + 4} units of 2^-53")


# ---- 4. same bits through the band entry --------------------------------------------------------------------------------------------
def _fields(sol, tau):
    fd = sol.flux_down(tau)
    return dict(u=sol.u(tau, PHI), u0=sol.u0(tau), flux_up=sol.flux_up(tau), flux_down_diffuse=fd[0], flux_down_direct=fd[1])


@pytest.mark.parametrize("NQuad,dead,thermal", [(8, True, False), (32, False, False), (16, False, True)])
def test_band_entry_gives_the_bits_of_the_batch_entry(NQuad, dead, thermal):
    import pydisort_amd
    kw = band(NQuad, dead, thermal)
    tau, om, f, leg = pydisort_amd.band_mix(kw["dtau_abs"], kw["dtau_spec"], kw["omega_spec"], kw["Leg_spec"], NQuad, delta_M=True)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS)
    assert np.array_equal(bsol.tau_arr.reshape(P * G, L), tau) and bsol.plan.windows()[1] == 1
    rep = lambda a: np.repeat(a, G, axis=0)  # noqa: E731
    th = None
    if thermal:
        th = {k: (rep(v) if isinstance(v, np.ndarray) else v) for k, v in kw["thermal"].items()}
    _, sol = pydisort_amd.pydisort_batch(tau, om, NQuad, leg, rep(kw["mu0"]), kw["I0"].reshape(-1), rep(kw["phi0"]), f_arr=f,
                                         b_pos=rep(kw["b_pos"]), b_neg=kw["b_neg"], device_prepare=True, thermal=th)
    assert sol.plan.windows() == bsol.plan.windows()
    levels = np.concatenate((np.zeros((P * G, 1)), tau), axis=1)
    want, got = _fields(sol, levels), _fields(bsol.columns, levels)
    for k in want:
        assert np.all(np.isfinite(want[k])) and np.max(np.abs(want[k])) > 0, k
        assert np.array_equal(got[k], want[k]), (k, float(np.max(np.abs(got[k] - want[k]))))


# ---- 5. reduction -------------------------------------------------------------------------------------------------------------------
def hold_reduced(red, full, w, profiles=range(P)):
    """red [P, K, ...] against sum_g w[k][g] full[p G + g][...] in exact rational arithmetic; returns the worst error in ulps."""
    X, R = full.reshape(P, G, -1), red.reshape(P, w.shape[0], -1)
    wf = [[Fraction(float(v)) for v in row] for row in w]
    worst = 0.0
    for p in profiles:
        xf = [[Fraction(float(v)) for v in X[p, g]] for g in range(G)]
        for k in range(w.shape[0]):
            for e in range(X.shape[2]):
                terms = [wf[k][g] * xf[g][e] for g in range(G)]
                exact = sum(terms)
                ulp = Fraction(math.ulp(float(exact)))
                err = abs(Fraction(float(R[p, k, e])) - exact)
                assert err <= ulp + sum(abs(t) for t in terms) / 2 ** 90, (p, k, e, float(R[p, k, e]), float(exact))
                worst = max(worst, float(err / ulp))
    return worst


@functools.lru_cache(maxsize=None)
def _reduced_and_full(NQuad, work_columns):
    import pydisort_amd
    from pydisort_amd.band import level_tau
    kw = band(NQuad)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS, work_columns=work_columns)
    plan = bsol.plan
    assert plan.windows()[1] == (1 if work_columns == 0 else 4)
    out = {}
    plan.set_eval_points(level_tau(plan.prep["tau"]), PHI)  # all levels: the fused interface evaluation of the run path
    plan.run()
    out["fetch"] = (plan.fetch_band(), plan.fetch())
    for nphi in (1, 3):
        sub = level_tau(plan.prep["tau"], [1, 3])
        out["evaluate", nphi] = (plan.evaluate_band(sub, PHI[:nphi]), plan.evaluate(sub, PHI[:nphi]))
    plan.close()
    return out


@pytest.mark.parametrize("NQuad", [8, 32])
@pytest.mark.parametrize("work_columns", [0, 4])
def test_reduction_is_the_correctly_rounded_weighted_sum(NQuad, work_columns):
    res = _reduced_and_full(NQuad, work_columns)
    worst = 0.0
    for key, (red, full) in res.items():
        nlev, nphi = (L + 1, 3) if key == "fetch" else (2, key[1])
        assert red["u"].shape == (P, K, NQuad, nlev, nphi) and red["u0"].shape == (P, K, NQuad, nlev) and red["flux_up"].shape == (P, K, nlev)
        for k in ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct"):
            assert np.all(np.isfinite(full[k])) and np.max(np.abs(full[k])) > 0, (key, k)
            worst = max(worst, hold_reduced(red[k], full[k], WEIGHTS))
    print(f"REDUCE NQuad {NQuad} work_columns {work_columns}: worst {worst:.3f} ulp of the exact weighted sum")


@pytest.mark.parametrize("NQuad", [8, 32])
def test_reduced_bits_do_not_depend_on_the_window(NQuad):
    a, b = _reduced_and_full(NQuad, 0), _reduced_and_full(NQuad, 4)
    same = 0
    for key in a:
        for k in a[key][0]:
            if np.array_equal(a[key][1][k], b[key][1][k]):  # identical unreduced arrays -> identical reduced bits
                assert np.array_equal(a[key][0][k], b[key][0][k]), (key, k)
                same += 1
    print(f"WINDOW NQuad {NQuad}: {same} of {5 * len(a)} unreduced arrays identical between one window and windows of 4")


def test_band_solution_evaluators_and_the_streamed_form_agree_with_the_plan():
    """BandSolution's evaluators, the dropped K axis of weights [G], net_flux_convergence and solve_band_streamed all return what
    Plan.evaluate_band returns at the same levels."""
    import pydisort_amd
    from pydisort_amd.band import level_tau, net_flux_convergence
    kw = band(8)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS)
    ref = bsol.plan.evaluate_band(level_tau(bsol.plan.prep["tau"]), PHI)
    assert np.array_equal(bsol.flux_up(), ref["flux_up"]) and np.array_equal(bsol.u0([0, 2]), ref["u0"][..., [0, 2]])
    assert np.array_equal(bsol.u([3], PHI[:2]), ref["u"][..., [3], :2])
    dd, dr = bsol.flux_down()
    assert np.array_equal(dd, ref["flux_down_diffuse"]) and np.array_equal(dr, ref["flux_down_direct"])
    conv = bsol.net_flux_convergence()
    assert conv.shape == (P, K, L) and np.array_equal(conv, net_flux_convergence(ref["flux_up"], dd, dr))
    _, one = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS[1])
    assert one.flux_up().shape == (P, L + 1) and np.array_equal(one.flux_up(), ref["flux_up"][:, 1])
    out = pydisort_amd.solve_band_streamed(**kw, weights=WEIGHTS, phi=PHI, chunk_columns=4)
    assert np.array_equal(out["tau_arr"], bsol.tau_arr) and out["u"].shape == (P, K, 8, L + 1, 3)
    for k in ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct"):
        scale = np.max(np.abs(ref[k]))
        assert np.max(np.abs(out[k] - ref[k])) <= 1e-9 * scale, k  # (windows of 4, the fused evaluation: other kernels; the project's bar)
    sub = pydisort_amd.solve_band_streamed(**kw, weights=WEIGHTS[0], levels=[0, L], only_flux=True)
    assert "u" not in sub and sub["flux_up"].shape == (P, 2)
    assert np.max(np.abs(sub["flux_up"] - ref["flux_up"][:, 0][:, [0, L]])) <= 1e-9 * np.max(np.abs(ref["flux_up"]))


def test_band_stages_refuse_mode_shards():
    """Not combined in this change: a mode shard on a band plan, band weights or band inputs on a sharded plan."""
    import pydisort_amd
    from pydisort_amd.synthetic import cfg4_columns
    kw = band(8)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS)
    with pytest.raises(ValueError, match="not combined"):
        bsol.plan.set_mode_shard(0, 2, 8)
    bsol.plan.set_mode_shard(0, 1, 8)  # the default shard is no shard
    _, sol = pydisort_amd.pydisort_batch(**cfg4_columns(P * G, L=L, NQuad=8), mode_shard=(0, 2))
    with pytest.raises(ValueError, match="not combined"):
        sol.plan.set_band_weights(WEIGHTS)
    sol.plan._sharded = False  # past the Python check: the library refuses on its own
    with pytest.raises(RuntimeError, match="not combined"):
        sol.plan.set_band_weights(WEIGHTS)


# ---- 6. end to end against the oracle -----------------------------------------------------------------------------------------------
def test_band_results_match_the_oracle_on_numpy_mixed_columns():
    import warnings
    import goldens
    import pydisort_amd
    from conftest import record_parity
    from oracle import disort_oracle as O
    NQuad = 16
    kw = band(NQuad)
    tau, om, f, leg = numpy_mix(kw, NQuad, True)
    assert np.max(om) <= 0.99
    levels = np.concatenate((np.zeros((P * G, 1)), tau), axis=1)
    N = NQuad // 2
    want = dict(u=np.zeros((P, K, NQuad, L + 1, 3)), u0=np.zeros((P, K, NQuad, L + 1)), flux_up=np.zeros((P, K, L + 1)),
                flux_down_diffuse=np.zeros((P, K, L + 1)), flux_down_direct=np.zeros((P, K, L + 1)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for p in range(P):
            for g in range(G):
                c = p * G + g
                ref = O.pydisort(tau[c], om[c], NQuad, leg[c], float(kw["mu0"][p]), float(kw["I0"][p, g]), float(kw["phi0"][p]), f_arr=f[c],
                                 b_pos=float(kw["b_pos"][p]), b_neg=kw["b_neg"][c])
                fd = ref[2](levels[c])
                one = dict(u=ref[4](levels[c], PHI), u0=ref[3](levels[c]), flux_up=ref[1](levels[c]), flux_down_diffuse=fd[0],
                           flux_down_direct=fd[1])
                for k in want:
                    want[k][p] += WEIGHTS[:, g].reshape((K,) + (1,) * one[k].ndim) * one[k][None]
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS)
    assert len(bsol.mu_arr) == 2 * N
    dd, dr = bsol.flux_down()
    got = dict(u=bsol.u(None, PHI), u0=bsol.u0(), flux_up=bsol.flux_up(), flux_down_diffuse=dd, flux_down_direct=dr)
    for k in want:
        # the field scale of a weighted sum with mixed signs is that of its terms
        a, b = goldens.max_rel_err(got[k], want[k])
        print(f"ORACLE {k}: {a:.2e} of the field scale, {b:.2e} pointwise")
        record_parity(f"band/q16/{k}", a, b, 1e-9, None, against="oracle")


# ---- 7. a bad profile ---------------------------------------------------------------------------------------------------------------
def test_a_bad_profile_is_nan_and_the_others_keep_their_results():
    """Species 1 has a first moment of 2.5: no phase function, and 1 - omega g_1 < 0 wherever it dominates -- the eigen stage of
    Fourier mode 0 fails there.  Only profile 1 contains it."""
    import pydisort_amd
    from pydisort_amd.band import level_tau
    NQuad = 8
    kw = dict(band(NQuad))
    leg = kw["Leg_spec"].copy()
    leg[1, 1:] = 0.0
    leg[1, 1] = 2.5
    ds, om = kw["dtau_spec"].copy(), kw["omega_spec"].copy()
    ds[:, :, 1] = 0.0
    ds[1, :, 1] = 5.0
    om[1, :, 1] = 0.97
    kw.update(Leg_spec=leg, dtau_spec=ds, omega_spec=om)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS, numeric_errors="nan")
    plan = bsol.plan
    tau = level_tau(plan.prep["tau"])
    red, full = plan.evaluate_band(tau, PHI), plan.evaluate(tau, PHI)
    st = plan.column_status()
    assert np.all(st[G:2 * G] & 0xFF) and not np.any(st[:G]) and not np.any(st[2 * G:])
    for k in ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct"):
        assert np.all(np.isnan(red[k][1])), k
        assert np.all(np.isfinite(red[k][[0, 2]])), k
        hold_reduced(red[k], full[k], WEIGHTS, profiles=(0, 2))
    assert np.all(np.isnan(bsol.flux_up()[1])) and np.all(np.isfinite(bsol.flux_up()[[0, 2]]))
    _, raising = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS)
    with pytest.raises(pydisort_amd._lib.NumericalError):
        raising.flux_up()
    with pytest.raises(np.linalg.LinAlgError):
        raising.u([0], PHI)
