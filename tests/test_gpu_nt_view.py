"""Nakajima-Tanaka corrections evaluated at the viewing angles themselves (include/rtd.h: rtd_plan_set_view_nt; csrc/rtd_nt_view.hip:
rtd_nt_view_tables_kernel, rtd_nt_view_apply_kernel; arithmetic csrc/rtd_nt_view.h) on the device, against the 40-digit truth of
tools/nt_view_truth.py (fixtures tests/golden/nt_view, made by tests/golden/make_nt_view_goldens.py).

1. Corrections against truth.  u_at(corrections="at_angles") of a plan with NT_cor=True minus u_at of the same columns with NT_cor=False
   is the kernels' correction (the interpolant of the uncorrected u is the same in both: same kernels, same inputs).  Held, per column:
       |difference - truth| <= tol max|truth| + 2 eps |u_at without corrections|   pointwise
   with tol by tests/nt_view_cases.py: ten times what the EXISTING node kernels show against their truth in that padding class and
   order, under the ceiling 1e-9 -- the coincidence angles (mu = -mu0, -mu0 (1 +- 1e-9), minus the scaled mu0 and its neighbour)
   under the SAME bound.  Through evaluate, run, run_fetch, lean and full retained plans, the three tau-orders, device- and
   host-prepared corrections; and at minus the DEVICE's own ims_par[0] (Plan.get_nt) and its neighbour at 1e-9, with the truth formed
   at run time.
2. Identical bits: one window against windows of 4; a shared list against the same list per column; the streamed form against a plan
   driven by hand; the band entry against the batch entry fed with band_mix's arrays at 8 / 16 / 32 streams (G = 5, windows of 4); u,
   u0, the fluxes and u0_at with the mode on against the mode off; every result with the mode off against a plan on which the new
   symbol was never called.
3. Band reduction: the reduced band view within 1 ulp + 2^-90 sum|w x| of the exact weighted sum of the unreduced view
   (tests/test_gpu_band.py: hold_reduced); a failed profile is NaN and the others are kept.
4. At an exact node the new mode's value equals that node's row of the corrected u to within the same tolerance (not bit for bit: a
   different kernel forms it).

Worst figures seen on an MI355X, max over the columns of max(|difference - truth| - 2 eps |u_at|) / max|truth|, value / antiderivative /
derivative (the bound of the class in brackets; nothing of these enters a bound):
   NP 4   q6_L1                   4.3e-16 / 1.3e-16 / 5.1e-16   [1.5e-14 / 1.8e-14 / 1.7e-14]
   NP 8   batch6_q16_L3           1.5e-14 / 6.4e-15 / 1.4e-14   [4.5e-13 / 3.8e-13 / 3.8e-13]   the same through device-prepared corrections,
          full and lean retained plans, run and run_fetch in windows of 4
          q16_L4_mu0_near_node    7.4e-15 / 3.0e-15 / 1.4e-14;   q16_L4_smu0_near_node  3.5e-15 / 2.6e-15 / 1.3e-14
          (the node kernels lose 1.3e-10 and 1.3e-7 on these two inputs at the node next to mu0: tests/test_gpu_nt_truth.py)
          at minus the device's own ims_par[0] and its two neighbours at 1e-9: 2.3e-15 / 2.3e-15 / 2.9e-15, host- and device-prepared
   NP 16  q32_L20_cloud           8.6e-15 / 8.7e-15 / 1.6e-14   [7.0e-12 / 7.6e-12 / 4.2e-12]
   NP 32  q34_L3                  9.9e-14 / 9.9e-14 / 7.8e-14   [1.7e-12 / 3.3e-12 / 1.8e-12]
At the coincidence angles alone the figure is the fixture's own or smaller: the worst point of a value is as a rule mu = -mu0 at
phi = phi0, the forward direction, where the series is largest -- and it sits at 1/17 of its bound or below.  Band reduction 0.499 ulp;
at an exact node at most 1.2e-14 of the largest correction at the nodes (batch6_q16_L3); every bit comparison identical."""
import numpy as np
import pytest

import nt_view_cases as VC

pytestmark = pytest.mark.gpu

EPS = VC.EPS
ORDER_KW = dict(value={}, antiderivative=dict(is_antiderivative_wrt_tau=True), derivative=dict(is_derivative_wrt_tau=True))
ORDER_INT = VC.ORDER_INT


@pytest.fixture(scope="module")
def amd():
    import pydisort_amd
    from pydisort_amd import _engine
    assert _engine.device_count() >= 1, "no HIP device visible"
    return pydisort_amd


_PLANS = {}


def pair(amd, name, **extra):
    """(with NT_cor, without) for one fixture and set of options; only the latest pair is kept."""
    key = (name, tuple(sorted(extra.items())))
    if key not in _PLANS:
        for sols in _PLANS.values():
            for s in sols:
                s.plan.close()
        _PLANS.clear()
        kw = VC.load(name).kw
        _PLANS[key] = (amd.pydisort_batch(NT_cor=True, **kw, **extra)[1], amd.pydisort_batch(NT_cor=False, **kw, **extra)[1])
    return _PLANS[key]


def angles(case):
    return case.mu if case.C > 1 else case.mu[0]


def hold(label, on, off, truth, case, order, hot=None):
    """on, off [C, nmu, ntau, nphi]: the views with and without corrections."""
    assert on.shape == truth.shape == off.shape, (label, on.shape, truth.shape)
    assert np.all(np.isfinite(on)) and np.all(np.isfinite(off)), label
    tol = VC.tolerance(case.kw["NQuad"], order)
    allow = 2 * EPS * np.abs(off)
    err = VC.worst(on - off, truth, allow)
    hot = VC.coincidence(case) if hot is None else hot
    err_hot = max((float(np.max(np.maximum(np.abs(on[c] - off[c] - truth[c]) - allow[c], 0.0)[hot[c]]) / np.max(np.abs(truth[c])))
                   for c in range(truth.shape[0]) if hot[c].any()), default=0.0)
    print(f"NT-VIEW {label} {order}: {err:.2e} of max|truth| (coincidence angles {err_hot:.2e}), tol {tol:.2e}, "
          f"max|correction| / max|u_at| {np.max(np.abs(truth)) / np.max(np.abs(off)):.2e}")
    assert err <= tol and err_hot <= tol, (label, order, err, err_hot, tol)
    return err


# ---- 1. against truth -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", VC.ORDERS)
@pytest.mark.parametrize("name", VC.NAMES)
def test_corrections_against_truth(amd, name, order):
    case = VC.load(name)
    on, off = pair(amd, name)
    mu = angles(case)
    got = on.u_at(mu, case.tau, case.phi, corrections="at_angles", **ORDER_KW[order])
    base = off.u_at(mu, case.tau, case.phi, **ORDER_KW[order])
    assert np.array_equal(base, off.u_at(mu, case.tau, case.phi, corrections="at_angles", **ORDER_KW[order]))  # no corrections: the mode is ignored
    hold(f"evaluate {name}", got, base, case.truth[order], case, order)


ENTRIES = {
    "device-prepared": dict(device_prepare=True),
    "full": dict(work_columns=4, retain="full"),
    "lean": dict(work_columns=4, retain="lean"),
    "run": dict(work_columns=4, retain=False, _defer_solve=True),
    "run_fetch": dict(work_columns=4, retain=False, device_prepare=True, _defer_solve=True),
}


def through(sol, entry, case, order, corrections):
    plan, mu = sol.plan, angles(case)
    if entry in ("run", "run_fetch"):
        assert plan.windows() == (4, 2)
        plan.set_view(mu, corrections=corrections)
        plan.set_eval_points(case.tau, case.phi)
        plan.set_eval_order(ORDER_INT[order])
        if entry == "run":
            plan.run()
        else:
            plan.run_fetch()
        return plan.fetch_view(("u",))["u_mu"]
    if entry in ("full", "lean"):
        assert plan.windows() == (4, 2) and plan.retained_form() == entry
    return sol.u_at(mu, case.tau, case.phi, corrections=corrections, **ORDER_KW[order])


@pytest.mark.parametrize("order", VC.ORDERS)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_entry_against_truth(amd, entry, order):
    case = VC.load(VC.BATCH)
    on, off = pair(amd, VC.BATCH, **ENTRIES[entry])
    got = through(on, entry, case, order, "at_angles")
    base = through(off, entry, case, order, "interpolated")
    hold(f"{entry} {VC.BATCH}", got, base, case.truth[order], case, order)


@pytest.mark.parametrize("prepared", ["host", "device"])
def test_at_the_devices_own_scaled_mu0(amd, prepared):
    """mu = -ims_par[0] of each column as the DEVICE holds it (chi's x is then exactly 0 in the kernel) and its neighbour at 1e-9; the
    truth is formed here, at those very angles."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import nt_view_truth
    case = VC.load(VC.BATCH)
    on, off = pair(amd, VC.BATCH, **(dict(device_prepare=True) if prepared == "device" else {}))
    s = on.plan.get_nt()["ims_par"][:, 0]
    assert np.all((s > 0) & (s * (1 + 1e-9) < 1))
    mu = np.ascontiguousarray(np.stack((-s, -s * (1 + 1e-9), -s * (1 - 1e-9)), axis=1))
    cols = [{k: (v if np.ndim(v) == 0 else v[c]) for k, v in case.kw.items()} for c in range(case.C)]
    truth = {o: np.stack([nt_view_truth.correction(cols[c], mu[c], case.tau[c], case.phi)[o] for c in range(case.C)]) for o in VC.ORDERS}
    for order in VC.ORDERS:
        got = on.u_at(mu, case.tau, case.phi, corrections="at_angles", **ORDER_KW[order])
        base = off.u_at(mu, case.tau, case.phi, **ORDER_KW[order])
        hold(f"own scaled mu0, {prepared}-prepared", got, base, truth[order], case, order, hot=np.ones(mu.shape, bool))


# ---- 2. identical bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", VC.ORDERS)
def test_bits_depend_on_neither_the_window_nor_the_sharing(amd, order):
    case = VC.load(VC.BATCH)
    kw = dict(case.kw, NT_cor=True)
    shared = case.mu[2]
    res = []
    for wc, mu in ((0, case.mu), (4, case.mu), (0, shared), (4, np.tile(shared, (case.C, 1)))):
        _, sol = amd.pydisort_batch(**kw, work_columns=wc)
        assert sol.plan.windows()[1] == (1 if wc == 0 else 2)
        res.append(sol.u_at(mu, case.tau, case.phi, corrections="at_angles", **ORDER_KW[order]))
        sol.plan.close()
    assert np.all(np.isfinite(res[0])) and np.array_equal(res[0], res[1])
    assert np.array_equal(res[2], res[3]) and np.array_equal(res[2][2], res[0][2])


@pytest.mark.parametrize("order", VC.ORDERS)
def test_streamed_form_gives_the_bits_of_the_plan_driven_by_hand(amd, order):
    case = VC.load(VC.BATCH)
    cfg = dict(case.kw, NT_cor=True)
    got = amd.solve_columns_streamed(cfg, case.tau, case.phi, chunk_columns=4, mu=case.mu, tau_order=ORDER_INT[order], view_corrections="at_angles")
    _, sol = amd.pydisort_batch(**cfg, work_columns=4, device_prepare=True, _defer_solve=True)
    plan = sol.plan
    plan.set_view(case.mu, corrections="at_angles")
    plan.set_eval_points(case.tau, case.phi)
    plan.set_eval_order(ORDER_INT[order])
    out, want = plan.run_fetch(), plan.fetch_view()
    plan.close()
    plain = amd.solve_columns_streamed(cfg, case.tau, case.phi, chunk_columns=4, mu=case.mu, tau_order=ORDER_INT[order])
    for k in ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct"):
        assert np.array_equal(got[k], out[k]) and np.array_equal(got[k], plain[k]), k  # (and the mode changes none of them)
    assert np.array_equal(got["u_mu"], want["u_mu"]) and np.array_equal(got["u0_mu"], want["u0_mu"])
    assert np.array_equal(got["u0_mu"], plain["u0_mu"]) and not np.array_equal(got["u_mu"], plain["u_mu"])


@pytest.mark.parametrize("NQuad", [8, 16, 32])
def test_band_columns_give_the_bits_of_the_batch_entry(amd, NQuad):
    import test_gpu_nt_device as D
    import view_cases as V
    kw, tau, om, f, full = D._band_arrays(NQuad)
    rep = lambda a: np.repeat(a, D.G, axis=0)  # noqa: E731
    _, bsol = amd.pydisort_band(**kw, weights=D.WEIGHTS, NT_cor=True, work_columns=4)
    _, sol = amd.pydisort_batch(tau, om, NQuad, full, rep(kw["mu0"]), kw["I0"].reshape(-1), rep(kw["phi0"]), NLeg=NQuad, f_arr=f,
                                b_pos=rep(kw["b_pos"]), b_neg=kw["b_neg"], device_prepare=True, NT_cor=True, work_columns=4)
    assert sol.plan.windows() == bsol.plan.windows() and bsol.plan.windows()[1] == 4 and D.G == 5
    x = V.nodes(NQuad)
    mu = np.array([0.23, -0.37, x[1], -x[len(x) // 2], 1.0, -1.0, float(kw["mu0"][0]), -float(kw["mu0"][0]), -float(kw["mu0"][1]) * (1 + 1e-9), -1e-3])
    mid = np.concatenate((0.5 * tau[:, :1], 0.5 * (tau[:, 1:] + tau[:, :-1])), axis=1)
    pts = np.ascontiguousarray(np.concatenate((np.zeros((D.P * D.G, 1)), tau, mid), axis=1))
    for order in VC.ORDERS:
        got = bsol.columns.u_at(mu, pts, D.PHI, corrections="at_angles", **ORDER_KW[order])
        want = sol.u_at(mu, pts, D.PHI, corrections="at_angles", **ORDER_KW[order])
        assert np.all(np.isfinite(want)) and np.max(np.abs(want)) > 0
        assert np.array_equal(got, want), (order, float(np.max(np.abs(got - want))))
        assert not np.array_equal(want, sol.u_at(mu, pts, D.PHI, **ORDER_KW[order])), order  # (the mode is not nothing)
    bsol.plan.close()
    sol.plan.close()


KEYS = ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct", "u_mu", "u0_mu")


@pytest.mark.parametrize("extra", [dict(), dict(work_columns=4, retain="lean"), dict(device_prepare=True)], ids=["one-window", "lean", "device-prepared"])
def test_the_mode_changes_nothing_else_and_leaves_nothing_behind(amd, extra):
    """Mode on against mode off on one plan: u, u0, the fluxes and u0_mu keep their bits.  Then the same plan back in mode 0 against a
    plan on which rtd_plan_set_view_nt was never called: every result, u_mu included, bit for bit -- through evaluate and through run."""
    case = VC.load(VC.BATCH)
    kw = dict(case.kw, NT_cor=True)
    _, used = amd.pydisort_batch(**kw, **extra)
    _, fresh = amd.pydisort_batch(**kw, **extra)
    want = ("u", "u0", "flux", "view")
    for order in VC.ORDERS:
        fl = dict(antiderivative=order == "antiderivative", derivative=order == "derivative")
        fresh.plan.set_view(case.mu)
        ref = fresh.plan.evaluate(case.tau, case.phi, want=want, **fl)
        used.plan.set_view(case.mu, corrections="at_angles")
        on = used.plan.evaluate(case.tau, case.phi, want=want, **fl)
        for k in KEYS:
            assert np.array_equal(on[k], ref[k]) == (k != "u_mu"), (order, k)
        assert np.array_equal(used.u0_at(case.mu, case.tau, **ORDER_KW[order]), ref["u0_mu"])
        used.plan.set_view(case.mu, corrections="interpolated")
        off = used.plan.evaluate(case.tau, case.phi, want=want, **fl)
        for k in KEYS:
            assert np.array_equal(off[k], ref[k]), (order, k)
    for plan, modes in ((used.plan, ("at_angles", "interpolated")), (fresh.plan, (None,))):
        plan.set_eval_points(case.tau, case.phi)
        for m in modes:
            plan.set_view(case.mu, **({} if m is None else dict(corrections=m)))
            plan.run()
            res = dict(plan.fetch(), **plan.fetch_view())
        if plan is used.plan:
            kept = res
    for k in KEYS:
        assert np.array_equal(kept[k], res[k]), k
    used.plan.close()
    fresh.plan.close()


# ---- 3. band reduction -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("work_columns", [0, 4])
def test_band_reduction_is_the_correctly_rounded_weighted_sum(amd, work_columns):
    import test_gpu_band as B
    from pydisort_amd.band import level_tau
    NQuad = 8
    kw = B.band(NQuad, True)
    _, bsol = amd.pydisort_band(**kw, weights=B.WEIGHTS, NT_cor=True, work_columns=work_columns)
    plan = bsol.plan
    assert plan.windows()[1] == (1 if work_columns == 0 else 4)
    mu0 = kw["mu0"]
    mu = np.array([[0.9, -mu0[0], -0.45, 1.0], [0.2, -mu0[1] * (1 + 1e-9), -1.0, -1e-3], [0.55, mu0[2], -mu0[2], -0.62]])  # [P, nmu]
    worst = 0.0
    plan.set_view(np.repeat(mu, B.G, axis=0), corrections="at_angles")
    plan.set_eval_points(level_tau(plan.prep["tau"]), B.PHI)
    plan.run()
    red, full = plan.fetch_band_view(), plan.fetch_view()
    for k in ("u_mu", "u0_mu"):
        assert np.all(np.isfinite(full[k])) and np.max(np.abs(full[k])) > 0
        worst = max(worst, B.hold_reduced(red[k], full[k], B.WEIGHTS))
    sub = level_tau(plan.prep["tau"], [1, 3])
    for order in VC.ORDERS:
        r = plan.evaluate_band(sub, B.PHI, want=("view",), antiderivative=order == "antiderivative", derivative=order == "derivative")
        worst = max(worst, B.hold_reduced(r["u_mu"], plan.fetch_view()["u_mu"], B.WEIGHTS))
    got = bsol.u_at(mu, [1, 3], B.PHI, corrections="at_angles")
    assert got.shape == (B.P, B.K, mu.shape[1], 2, len(B.PHI))
    assert np.array_equal(got, plan.evaluate_band(sub, B.PHI, want=("view_u",))["u_mu"])
    assert not np.array_equal(got, bsol.u_at(mu, [1, 3], B.PHI))
    plan.close()
    out = amd.solve_band_streamed(**kw, weights=B.WEIGHTS, levels=[1, 3], phi=B.PHI, chunk_columns=4, NT_cor=True, mu=mu, view_corrections="at_angles")
    assert out["u_mu"].shape == got.shape and np.max(np.abs(out["u_mu"] - got)) <= 1e-9 * np.max(np.abs(got))  # (the run path: other kernels)
    print(f"NT-VIEW REDUCE work_columns {work_columns}: worst {worst:.3f} ulp of the exact weighted sum")


def test_a_bad_profile_is_nan_and_the_others_keep_their_results(amd):
    """The bad profile of tests/test_gpu_band.py (a species whose first moment is 2.5: mode 0 of profile 1 fails)."""
    import test_gpu_band as B
    import view_cases as V
    kw = dict(B.band(8))
    leg = kw["Leg_spec"].copy()
    leg[1, 1:] = 0.0
    leg[1, 1] = 2.5
    ds, om = kw["dtau_spec"].copy(), kw["omega_spec"].copy()
    ds[:, :, 1] = 0.0
    ds[1, :, 1] = 5.0
    om[1, :, 1] = 0.97
    kw.update(Leg_spec=leg, dtau_spec=ds, omega_spec=om)
    mu = np.array([0.4, -float(kw["mu0"][0]), -0.8, V.nodes(8)[1]])
    _, bsol = amd.pydisort_band(**kw, weights=B.WEIGHTS, numeric_errors="nan", NT_cor=True)
    plan = bsol.plan
    plan.set_view(mu, corrections="at_angles")
    lev = np.concatenate((np.zeros((B.P * B.G, 1)), plan.prep["tau"]), axis=1)
    red = plan.evaluate_band(lev, B.PHI, want=("view",))
    full = plan.evaluate(lev, B.PHI, want=("view",))
    for k in ("u_mu", "u0_mu"):
        assert np.all(np.isnan(red[k][1])) and np.all(np.isnan(full[k][B.G:2 * B.G])), k
        assert np.all(np.isfinite(red[k][[0, 2]])), k
        B.hold_reduced(red[k], full[k], B.WEIGHTS, profiles=(0, 2))
    plan.close()


# ---- 4. at an exact node --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", VC.ORDERS)
@pytest.mark.parametrize("name", ["q6_L1", VC.BATCH, "q34_L3"])
def test_at_a_node_the_value_is_the_corrected_row(amd, name, order):
    case = VC.load(name)
    on, off = pair(amd, name)
    N = case.kw["NQuad"] // 2
    x = on.mu_arr[:N]
    pick = sorted({0, N // 2, N - 1})
    mu = np.concatenate((x[pick], -x[pick]))
    rows = pick + [N + j for j in pick]
    got = on.u_at(mu, case.tau, case.phi, corrections="at_angles", **ORDER_KW[order])
    corrected = on.u(case.tau, case.phi, **ORDER_KW[order])
    plain = off.u(case.tau, case.phi, **ORDER_KW[order])
    tol = VC.tolerance(case.kw["NQuad"], order)
    for c in range(case.C):
        scale = np.max(np.abs(corrected[c] - plain[c]))
        err = np.abs(got[c] - corrected[c, rows]) - 2 * EPS * np.abs(plain[c, rows])
        print(f"NT-VIEW node {name} {order} column {c}: {np.max(err) / scale:.2e} of the largest correction at the nodes, tol {tol:.2e}")
        assert np.max(err) <= tol * scale, (name, order, c)
    assert np.array_equal(on.u_at(mu, case.tau, case.phi, **ORDER_KW[order]), corrected[:, rows])  # (the interpolating mode copies the row)
