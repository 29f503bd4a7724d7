"""Nakajima-Tanaka corrections whose inputs the DEVICE forms (include/rtd.h: rtd_plan_request_nt, rtd_plan_get_nt; kernels
rtd_nt_wfull_kernel, rtd_nt_wfull_band_kernel, rtd_nt_ims_kernel of csrc/rtd_api.hip, arithmetic csrc/rtd_nt_prep.h) on every entry
that prepares on the device: pydisort_batch(device_prepare=True, NT_cor=True), solve_columns_streamed, pydisort_band and
solve_band_streamed(NT_cor=True).

1. inputs: Plan.get_nt() against exact Fraction values within the bounds derived in tests/nt_prep_cases.py (the bounds of
   tests/test_nt_prep_cpu.py, no others); the band's weighted phase function has P rows and is (2k + 1) x band_mix's moments bit for bit.
2. truth: on - off against the committed 40-digit fixtures of tests/golden/nt, held as tests/test_gpu_nt_truth.py holds the
   host-prepared path -- the same apply kernels, inputs that differ by a few roundings: 10 x MEASURED (copied from there) of
   max|truth|, never above 1e-9, plus 4 eps max|off u|.
3. the band entry gives the bits of the batch entry fed with band_mix's arrays: corrected and uncorrected, three tau-orders.
4. the reduced corrected u is the correctly rounded weighted sum of the plan's own unreduced corrected u (test_gpu_band's check).
5. two columns of a band against tools/nt_truth.correction run on the device's own float64 inputs.
6. solve_columns_streamed with NT_cor gives the bits of the plan-driven device-prepared batch.
7. the states of the C ABI through Plan.

Figures seen on an MI355X (each test prints its own).  1: worst 0.231 (batch) and 0.146 (band) of the derived bound.  2, max|corr -
truth| / max|truth|, value / antiderivative / derivative: q6_L1 1.5e-15 / 1.8e-15 / 1.6e-15; q18_L3 5.4e-15 / 5.2e-15 / 5.2e-15;
q34_L3 5.8e-14 / 9.5e-14 / 2.6e-14; q66_L2 1.9e-13 / 1.6e-13 / 1.6e-13; batch7_q16_L6 4.4e-14 / 3.7e-14 / 3.7e-14, the same with
windows of three -- the host-prepared path's own figures to two digits.  3: identical in all 36 comparisons.  4: 0.500 ulp.  5: the
ordinary column 2.2e-14, the chosen column of the dead-layer profile 4.5e-14 / 2.5e-14 / 1.3e-14 of max|truth|.  The other four
columns of that profile, whose scaled mu0 lie 3.6e-5 ... 3.0e-4 from a quadrature node, are at 4.7e-12, 4.0e-11, 5.8e-13 and
1.0e-12 (value) -- with host-prepared inputs the same to three digits: the apply kernels' conditioning next to a node, which the
well-conditioned bound does not cover and this change does not touch.  7: a plan without a request holds 2 210 712 bytes, as the
host-prepared plan without corrections; with one 2 240 728, as the host-prepared plan with uploaded corrections."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import nt_prep_cases as NP
import nt_truth_cases as NC
from test_gpu_band import G, K, L, P, PHI, WEIGHTS, band, hold_reduced

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
CEILING = 1e-9
# tests/test_gpu_nt_truth.py: MEASURED, max|corr - truth| / max|truth| of the host-prepared path per padding class NP and order
# (value, antiderivative, derivative), measured on one MI355X
MEASURED = {
    4: (1.5e-15, 1.8e-15, 1.7e-15),
    8: (4.5e-14, 3.8e-14, 3.8e-14),
    16: (7.0e-13, 7.6e-13, 4.2e-13),
    32: (1.7e-13, 3.3e-13, 1.8e-13),
    64: (1.9e-13, 1.6e-13, 2.0e-13),
}
ORDER_FLAGS = dict(value={}, antiderivative=dict(antiderivative=True), derivative=dict(derivative=True))


def padding_class(NQuad):
    n = 4
    while n < NQuad // 2:
        n *= 2
    return n


def tol_for(NQuad, order):
    tol = 10 * MEASURED[padding_class(NQuad)][NC.ORDERS.index(order)]
    assert tol <= CEILING
    return tol


@functools.lru_cache(maxsize=None)
def nt_truth():
    spec = importlib.util.spec_from_file_location("nt_truth", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "nt_truth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hold_correction(label, on, off, truth, tol):
    """on, off: dicts of Plan.evaluate; truth [C, NQuad, ntau, nphi].  The bound of tests/test_gpu_nt_truth.py, per column."""
    for k in ("u0", "flux_up", "flux_down_diffuse", "flux_down_direct"):
        assert np.array_equal(on[k], off[k]), k
    assert np.all(np.isfinite(on["u"])) and np.all(np.isfinite(off["u"]))
    worst = 0.0
    for c in range(truth.shape[0]):
        corr = on["u"][c] - off["u"][c]
        scale = np.max(np.abs(truth[c]))
        assert scale > 0
        err = np.max(np.abs(corr - truth[c])) / scale
        rounding = 4 * EPS * np.max(np.abs(off["u"][c])) / scale
        print(f"nt-device {label} column {c}: {err:.3e} of max|truth|, rounding term {rounding:.3e}, tol {tol:.3e}")
        assert err <= tol + rounding, (label, c, err, tol, rounding)
        worst = max(worst, err)
    return worst


# ---- 1. inputs ------------------------------------------------------------------------------------------------------------------------
def test_inputs_of_a_device_prepared_batch():
    import pydisort_amd
    c = NP.columns(3, 1, C=3)
    _, sol = pydisort_amd.pydisort_batch(c["tau"], c["omega"], 8, c["leg"], c["mu0"], c["I0"], np.zeros(3), NLeg=NP.NLEG, f_arr=c["f"],
                                         device_prepare=True, NT_cor=True)
    nt = sol.plan.get_nt()
    assert nt["wfull"].shape == (3, 3, NP.NALL) and nt["ims_coef"].shape == (3, NP.NALL) and nt["ims_par"].shape == (3, 2)
    assert np.array_equal(nt["f"], c["f"])
    worst = 0.0
    for i in range(3):
        NP.hold_wfull(nt["wfull"][i], c["leg"][i])
        # the plan's rescaled beam: I0 / max(I0, 0, 0) = 1
        worst = max(worst, NP.hold_ims(nt["ims_coef"][i], nt["ims_par"][i], c["tau"][i], c["omega"][i], c["f"][i], c["leg"][i], NP.NLEG,
                                       c["mu0"][i], 1.0))
    assert np.all(nt["ims_coef"][2] == 0) and nt["ims_par"][2, 0] == c["mu0"][2] and nt["ims_par"][2, 1] == 0  # f = 0: no IMS term
    assert np.all(np.isfinite(sol.u(c["tau"], PHI)))
    print(f"NT-DEVICE inputs, batch: worst {worst:.3f} of the derived bound")
    sol.plan.close()


def _band_arrays(NQuad, dead=True):
    import pydisort_amd
    kw = band(NQuad, dead)
    nall = kw["Leg_spec"].shape[1]
    tau, om, f, _ = pydisort_amd.band_mix(kw["dtau_abs"], kw["dtau_spec"], kw["omega_spec"], kw["Leg_spec"], NQuad, delta_M=True)
    full = pydisort_amd.band_mix(kw["dtau_abs"], kw["dtau_spec"], kw["omega_spec"], kw["Leg_spec"], nall, delta_M=False)[3]
    return kw, tau, om, f, full


def test_inputs_of_a_band():
    import pydisort_amd
    NQuad = 8
    kw, tau, om, f, full = _band_arrays(NQuad)
    nall = NQuad + 3
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS, NT_cor=True)
    nt = bsol.plan.get_nt()
    assert nt["wfull"].shape == (P, L, nall)  # one row per profile
    assert np.array_equal(nt["wfull"], (2 * np.arange(nall) + 1)[None, None, :] * full[::G])  # (an integer times a double: one rounding)
    assert np.array_equal(nt["wfull"][1, 1], np.eye(1, nall)[0])  # the layer without a scatterer: (1, 0, ...)
    assert np.array_equal(nt["f"], f) and np.array_equal(bsol.tau_arr.reshape(P * G, L), tau)
    I0 = kw["I0"].reshape(-1)
    big = np.maximum(I0, np.maximum(np.repeat(kw["b_pos"], G), kw["b_neg"].max(axis=1)))
    worst = 0.0
    for c in range(P * G):
        worst = max(worst, NP.hold_ims(nt["ims_coef"][c], nt["ims_par"][c], tau[c], om[c], f[c], full[c], NQuad, kw["mu0"][c // G], I0[c] / big[c]))
    print(f"NT-DEVICE inputs, band: worst {worst:.3f} of the derived bound")
    bsol.plan.close()


# ---- 2. truth -------------------------------------------------------------------------------------------------------------------------
_PLANS = {}


def _plan(name, **extra):
    import pydisort_amd
    key = (name, tuple(sorted(extra.items())))
    if key not in _PLANS:
        for sol in _PLANS.values():
            sol.plan.close()
        _PLANS.clear()
        _, sol = pydisort_amd.pydisort_batch(NT_cor=True, device_prepare=True, **NC.batch_kwargs(NC.load(name)), **extra)
        _PLANS[key] = sol
    return _PLANS[key]


@pytest.mark.parametrize("order", NC.ORDERS)
@pytest.mark.parametrize("name,work_columns", [("q6_L1", 0), ("q18_L3", 0), ("q34_L3", 0), ("q66_L2", 0), (NC.BATCH, 0), (NC.BATCH, 3)])
def test_device_formed_corrections_against_truth(name, work_columns, order):
    case = NC.load(name)
    extra = dict(work_columns=work_columns) if work_columns else {}
    sol = _plan(name, **extra)
    if work_columns:
        assert sol.plan.windows()[1] == 3
    tau = case.tau if case.batch else case.tau[None]
    truth = case.truth[order] if case.batch else case.truth[order][None]
    on = sol.plan.evaluate(tau, case.phi, **ORDER_FLAGS[order])
    off = sol.plan.evaluate(tau, case.phi, skip_nt=True, **ORDER_FLAGS[order])
    worst = hold_correction(f"{name} work_columns={work_columns} {order}", on, off, truth, tol_for(case.columns[0]["NQuad"], order))
    print(f"NT-DEVICE truth {name} work_columns={work_columns} {order}: worst {worst:.2e} of max|truth|")


# ---- 3. same bits, band against batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("work_columns", [0, 4])
@pytest.mark.parametrize("NQuad", [8, 16, 32])
def test_band_entry_gives_the_corrected_bits_of_the_batch_entry(NQuad, work_columns):
    import pydisort_amd
    kw, tau, om, f, full = _band_arrays(NQuad)
    rep = lambda a: np.repeat(a, G, axis=0)  # noqa: E731
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS, NT_cor=True, work_columns=work_columns)
    _, sol = pydisort_amd.pydisort_batch(tau, om, NQuad, full, rep(kw["mu0"]), kw["I0"].reshape(-1), rep(kw["phi0"]), NLeg=NQuad, f_arr=f,
                                         b_pos=rep(kw["b_pos"]), b_neg=kw["b_neg"], device_prepare=True, NT_cor=True,
                                         work_columns=work_columns)
    assert sol.plan.windows() == bsol.plan.windows() and bsol.plan.windows()[1] == (1 if work_columns == 0 else 4)
    mid = np.concatenate((0.5 * tau[:, :1], 0.5 * (tau[:, 1:] + tau[:, :-1])), axis=1)
    pts = np.ascontiguousarray(np.concatenate((np.zeros((P * G, 1)), tau, mid), axis=1))
    for order, flags in ORDER_FLAGS.items():
        for skip in (False, True):
            got = bsol.plan.evaluate(pts, PHI, skip_nt=skip, want=("u",), **flags)["u"]
            want = sol.plan.evaluate(pts, PHI, skip_nt=skip, want=("u",), **flags)["u"]
            assert np.all(np.isfinite(want)) and np.max(np.abs(want)) > 0
            assert np.array_equal(got, want), (order, skip, float(np.max(np.abs(got - want))))
            if not skip:
                on = want
        assert not np.array_equal(on, want), order  # (want is now the uncorrected field: the correction is not nothing)
    bsol.plan.close()
    sol.plan.close()


# ---- 4. reduction after correction ----------------------------------------------------------------------------------------------------
def test_reduced_u_is_the_rounded_weighted_sum_of_the_corrected_u():
    import pydisort_amd
    from pydisort_amd.band import level_tau
    NQuad = 8
    kw = band(NQuad, True)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS, NT_cor=True)
    _, plain = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS)
    lv = level_tau(bsol.plan.prep["tau"])
    red, full = bsol.plan.evaluate_band(lv, PHI), bsol.plan.evaluate(lv, PHI)
    assert np.array_equal(bsol.u(None, PHI), red["u"])
    worst = hold_reduced(red["u"], full["u"], WEIGHTS)
    base = plain.plan.evaluate_band(lv, PHI)
    assert np.array_equal(full["u"], bsol.columns.u(lv, PHI)) and not np.array_equal(full["u"], plain.columns.u(lv, PHI))
    assert not np.array_equal(red["u"], base["u"])  # a silently skipped correction fails here
    for k in ("u0", "flux_up", "flux_down_diffuse", "flux_down_direct"):
        assert np.array_equal(red[k], base[k]), k
    bsol.plan.close()
    # the streamed form: windows of 4, the run path; its plan driven by hand for the unreduced field
    out = pydisort_amd.solve_band_streamed(**kw, weights=WEIGHTS, phi=PHI, chunk_columns=4, NT_cor=True)
    off = pydisort_amd.solve_band_streamed(**kw, weights=WEIGHTS, phi=PHI, chunk_columns=4)
    _, hand = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS, work_columns=4, retain=False, _defer_solve=True, NT_cor=True)
    assert hand.plan.windows()[1] == 4
    hand.plan.set_eval_points(lv, PHI)
    hand.plan.run()
    r2, f2 = hand.plan.fetch_band(), hand.plan.fetch()
    assert np.array_equal(out["u"], r2["u"])
    worst = max(worst, hold_reduced(out["u"], f2["u"], WEIGHTS))
    assert np.max(np.abs(f2["u"] - full["u"])) <= 1e-9 * np.max(np.abs(full["u"]))  # (other kernels on the run path: the project's bar)
    assert not np.array_equal(out["u"], off["u"])
    for k in ("u0", "flux_up", "flux_down_diffuse", "flux_down_direct"):
        assert np.array_equal(out[k], off[k]), k
    print(f"NT-DEVICE reduce: worst {worst:.3f} ulp of the exact weighted sum of the corrected u")
    hand.plan.close()
    plain.plan.close()


# ---- 5. band against truth ------------------------------------------------------------------------------------------------------------
def test_band_columns_against_forty_digits():
    import pydisort_amd
    NQuad = 16
    kw, tau, om, f, full = _band_arrays(NQuad)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS, NT_cor=True)
    assert np.array_equal(bsol.tau_arr.reshape(P * G, L), tau)
    # An ordinary column, and one of profile 1, whose middle layer has no scatterer.  The bound of item 2 is that of the WELL-CONDITIONED
    # fixtures: near a quadrature node the closed forms cancel (chi divides by x = 1 / mu - 1 / scaled mu0 twice, TMS by mu0 - mu) and
    # tests/test_gpu_nt_truth.py holds such fixtures to the float64 oracle's own loss instead.  This band's profile 1 has mu0 = 0.40737,
    # 9.1e-4 from a node, and the scaled mu0 of its five columns lie 3.6e-5 ... 5.5e-4 from it (their errors grow as the distance
    # shrinks, see the module's docstring -- with host-prepared inputs to the same three digits).  Which of the five is taken is decided by the INPUTS:
    # the one whose scaled mu0, formed here in NumPy, is farthest from every node.
    w = om * tau
    smu0 = np.repeat(kw["mu0"], G) / (1.0 - (f * w).sum(axis=1) / tau.sum(axis=1))
    dist = np.min(np.abs(bsol.mu_arr[None, :NQuad // 2] - smu0[:, None]), axis=1)
    print("NT-DEVICE band truth: distance of the scaled mu0 from the nearest node, profile 1:", " ".join(f"{d:.2e}" for d in dist[G:2 * G]))
    cols = [2, G + int(np.argmax(dist[G:2 * G]))]
    frac = np.array([0.0, 0.4, 1.0, 1.5, 2.0, 2.7, 3.0])  # in layers: interfaces and interior points, the dead layer included
    table = np.concatenate((np.zeros((P * G, 1)), tau), axis=1)
    lo = np.minimum(frac.astype(int), L - 1)
    pts = np.ascontiguousarray(table[:, lo] + (frac - lo)[None, :] * (table[:, lo + 1] - table[:, lo]))
    pts[:, -1] = tau[:, -1]
    for order, flags in ORDER_FLAGS.items():
        on = bsol.plan.evaluate(pts, PHI, **flags)
        off = bsol.plan.evaluate(pts, PHI, skip_nt=True, **flags)
        truth = np.stack([nt_truth().correction(dict(tau_arr=tau[c], omega_arr=om[c], NQuad=NQuad, Leg_coeffs_all=full[c], mu0=kw["mu0"][c // G],
                                                     I0=kw["I0"].reshape(-1)[c], phi0=kw["phi0"][c // G], f_arr=f[c], NLeg=NQuad),
                                                pts[c], PHI)[order] for c in cols])
        sub = lambda d: {k: v[cols] for k, v in d.items() if v is not None}  # noqa: E731
        worst = hold_correction(f"band q16 {order}", sub(on), sub(off), truth, tol_for(NQuad, order))
        print(f"NT-DEVICE band truth {order}: worst {worst:.2e} of max|truth|")
    bsol.plan.close()


# ---- 6. streamed ----------------------------------------------------------------------------------------------------------------------
def test_streamed_columns_give_the_bits_of_the_plan_driven_batch():
    import pydisort_amd
    case = NC.load(NC.BATCH)
    cfg = dict(NC.batch_kwargs(case), NT_cor=True)
    out = pydisort_amd.solve_columns_streamed(cfg, case.tau, case.phi, chunk_columns=3)
    _, sol = pydisort_amd.pydisort_batch(device_prepare=True, work_columns=3, _defer_solve=True, **cfg)
    assert sol.plan.windows()[1] == 3
    sol.plan.set_eval_points(case.tau, case.phi)
    want = sol.plan.run_fetch()
    for k in want:
        assert np.array_equal(out[k], want[k]), k
    off = pydisort_amd.solve_columns_streamed(dict(cfg, NT_cor=False), case.tau, case.phi, chunk_columns=3)
    hold_correction("streamed batch7 value", out, off, case.truth["value"], tol_for(16, "value"))
    flux = pydisort_amd.solve_columns_streamed(cfg, case.tau, case.phi, chunk_columns=3, only_flux=True)  # NT_cor ignored
    assert "u" not in flux and np.all(np.isfinite(flux["flux_up"]))
    sol.plan.close()


# ---- 7. states at the C ABI, through Plan ---------------------------------------------------------------------------------------------
def test_states_of_the_request():
    import pydisort_amd
    case = NC.load(NC.BATCH)
    kw_b = NC.batch_kwargs(case)
    kw_a = dict(kw_b, tau_arr=1.7 * kw_b["tau_arr"], mu0=np.roll(kw_b["mu0"], 1), omega_arr=np.roll(kw_b["omega_arr"], 2, axis=0))
    _, fresh = pydisort_amd.pydisort_batch(NT_cor=True, device_prepare=True, **kw_b)
    _, sol = pydisort_amd.pydisort_batch(NT_cor=True, device_prepare=True, **kw_a)
    _, host = pydisort_amd.pydisort_batch(NT_cor=True, **kw_b)
    _, plain = pydisort_amd.pydisort_batch(device_prepare=True, **kw_b)
    plan = sol.plan
    plan.evaluate(case.tau, case.phi)  # builds the correction tables from batch A
    nall = kw_b["Leg_coeffs_all"].shape[2]
    # a request, then the host-prepared upload: RTD_ERR_STATE
    with pytest.raises(RuntimeError, match="librtd error 4"):
        plan.set_columns(host.prep)
    # a request that does not match the columns: RTD_ERR_ARG (too many moments; no more than nleg)
    for bad in (nall + 1, kw_b["NLeg"]):
        plan.request_nt(bad)
        with pytest.raises(RuntimeError, match="librtd error 1"):
            plan.set_columns_raw(fresh.prep["raw"])
    plan.request_nt(nall)
    # new columns on the same plan: inputs and tables are rebuilt -- the bits of a fresh plan
    plan.set_columns_raw(fresh.prep["raw"])
    plan.solve()
    a, b = plan.get_nt(), fresh.plan.get_nt()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for order, flags in ORDER_FLAGS.items():
        got, want = plan.evaluate(case.tau, case.phi, **flags), fresh.plan.evaluate(case.tau, case.phi, **flags)
        assert np.array_equal(got["u"], want["u"]), order
    # the corrections switched off: the uncorrected bits; the next columns switch them on again (the request is sticky)
    off = plan.evaluate(case.tau, case.phi, skip_nt=True)
    on = plan.evaluate(case.tau, case.phi)
    plan.clear_nt()
    assert np.array_equal(plan.evaluate(case.tau, case.phi)["u"], off["u"]) and not np.array_equal(on["u"], off["u"])
    with pytest.raises(RuntimeError, match="librtd error 4"):
        plan.get_nt()
    plan.set_columns_raw(fresh.prep["raw"])
    plan.solve()
    assert np.array_equal(plan.evaluate(case.tau, case.phi)["u"], on["u"])
    # the request withdrawn: plain columns, no corrections, and the host-prepared upload is accepted again
    plan.request_nt(0)
    plan.clear_nt()
    plan.set_columns_raw(fresh.prep["raw"])
    plan.solve()
    assert np.array_equal(plan.evaluate(case.tau, case.phi)["u"], off["u"])
    plan.set_columns(host.prep)
    with pytest.raises(RuntimeError, match="librtd error 4"):
        plain.plan.get_nt()
    for s in (fresh, sol, host, plain):
        s.plan.close()


def test_a_plan_without_a_request_holds_what_it_held():
    """Without a request a device-prepared plan holds exactly what the (untouched) host-prepared plan without corrections holds; with
    one, exactly what the host-prepared plan with uploaded corrections holds: the same five buffers of the same sizes.
    (device_bytes counts the blocks as the library's pool hands them out, which may be larger than asked for: the pool is emptied
    before each plan and again before its evaluation buffers grow, so that every block is fresh and of the size asked.)"""
    import pydisort_amd
    case = NC.load(NC.BATCH)
    kw = NC.batch_kwargs(case)

    def held(**extra):
        pydisort_amd.pool_trim()
        _, s = pydisort_amd.pydisort_batch(**kw, **extra)
        pydisort_amd.pool_trim()
        s.plan.evaluate(case.tau, case.phi)
        n = s.plan.device_bytes()
        s.plan.close()
        return n

    plain_host, plain = held(), held(device_prepare=True)
    nt_host, nt_device = held(NT_cor=True), held(NT_cor=True, device_prepare=True)
    print(f"NT-DEVICE bytes: plain {plain_host} / {plain}, with corrections {nt_host} / {nt_device}")
    assert plain == plain_host
    assert nt_device == nt_host > plain
