"""Radiances at user polar angles on the device: Plan.set_view / fetch_view / fetch_band_view, want=("view",),
BatchSolution.u_at / u0_at, BandSolution.u_at / u0_at and mu= of the two streamed forms (include/rtd.h: rtd_plan_set_view_mu,
rtd_plan_fetch_view, rtd_plan_fetch_band_view; csrc/rtd_api.hip: rtd_view_basis_kernel, rtd_view_apply_kernel).

Shapes: the batch of tests/test_gpu_actinic.py -- 6 columns x 3 layers at 6, 16 and 34 streams (N = 3, 8, 17), column 2 with I0 = 0,
column 4 with f = 0 -- with all Fourier modes; points tau = 0, every interface and two interior depths; two azimuths, so that a
wrong stride shows.  Angles: view_cases.mu_list (1, a node, the float next above a node, 0.37, +0.0, -0.62, a negated node, -1)
shared by the columns, and a [C, nmu] draw that mixes the hemispheres, with a node and a zero, per column.

Every bound is derived, none is measured.  u = 2^-53, gamma_k = k u / (1 - k u), X the plan's OWN fetched u / u0, x = prep["mu"],
l_j the exact basis of the float64 nodes at the float64 angle (fractions.Fraction), Lambda = sum_j |l_j|.  The kernels form
  t_j = fl(b_j / fl(a - x_j))  with the host's rounded weight b_j: 3 roundings,                         t_j (1 + theta_3)
  s   = t_0 + ... + t_{N-1}:   N - 1 additions of those: |s^ - s| <= gamma_{N+2} sum |t_j| = gamma_{N+2} Lambda |s|
  l_j = fl(t_j / s):           1 rounding, and the divisor's relative error, which counts twice (Higham, Lemma 3.3)
  out = l_0 X_0 + ... :        N products and N - 1 additions, at most N roundings on any term (fewer when the compiler fuses)
so every term l_j X_j carries a relative error theta_k with k = 3 + 1 + N + 2 (N + 2) Lambda: the weight's rounding is in there
twice, once in the numerator and once under the denominator.  |out - sum_j l_j X_j| <= gamma_k sum_j |l_j X_j|, k = N + 4 +
2 (N + 2) Lambda(mu).  At a node the result is the node's row, bit for bit.

End to end: 1e-9 Lambda(mu) of the reference array's scale (the node values are held at 1e-9 of the scale and interpolation
amplifies by at most Lambda).  Reduction: as tests/test_gpu_band.py, one ulp of the exact weighted sum + 2^-90 sum |w x|.  Each test
prints its worst ratio to its bound.

Figures seen on an MI355X: against the plan's own u and u0 at worst 0.18 of the bound (evaluate and retained plans, 6 streams,
per-column angles; 0.11 after run / run_fetch), node rows bit for bit; identical bits for one window and windows of 4, shared and
per-column lists, the streamed form and the plan driven by hand, the band entry and the batch entry; reduction 0.500 ulp of the
1 ulp + 2^-90 sum |w x| allowed; against the reference's fixtures 2.7e-12 (34 streams; <= 1.9e-13 at 6 and 16), the same through the
drop-in; against the oracle + model 1.0e-10 (34 streams, tau-derivative; <= 1.3e-13 at 6 and 16), of the 1e-9 Lambda allowed."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import view_cases as V

pytestmark = pytest.mark.gpu

C, L = 6, 3
NQUADS = (6, 16, 34)
ORDERS = (0, -1, 1)
U = Fraction(1, 2 ** 53)
PHI = np.array([0.3, 2.1])
KEYS = ("u_mu", "u0_mu")


def batch(NQuad, nt=False):
    """The batch of tests/test_gpu_actinic.py with all Fourier modes; nt: NT_cor=True, and what the host-prepared corrections
    need of every column: a beam (column 2 gets one) and a truncated phase function (column 4 gets its moment NLeg back)."""
    import test_gpu_actinic as T
    cfg = dict(T.batch(NQuad), only_flux=False)
    if nt:
        I0, f = cfg["I0"].copy(), cfg["f_arr"].copy()
        I0[2] = 0.8
        f[4] = cfg["Leg_coeffs_all"][4, :, NQuad]
        cfg.update(I0=I0, f_arr=f, NT_cor=True)
    return cfg


def points(tau_arr):
    import test_gpu_actinic as T
    return T.points(tau_arr)


def levels(tau_arr):
    import test_gpu_actinic as T
    return T.levels(tau_arr)


def shared_mu(NQuad):
    return V.mu_list(V.nodes(NQuad))


@functools.lru_cache(maxsize=None)
def column_mu(NQuad):
    """[C, nmu]: both hemispheres in every column, a node, a negated node, +0.0 and -0.0 somewhere."""
    x = V.nodes(NQuad)
    rng = np.random.default_rng(900 + NQuad)
    mu = rng.uniform(-1.0, 1.0, (C, 5))
    mu[:, 0] = np.abs(mu[:, 0])
    mu[:, 1] = -np.abs(mu[:, 1])
    mu[0, 2], mu[1, 2], mu[2, 3], mu[3, 3], mu[4, 4], mu[5, 4] = x[0], -x[-1], 0.0, -0.0, 1.0, -1.0
    mu.setflags(write=False)
    return mu


def flags(order):
    return dict(antiderivative=order < 0, derivative=order > 0)


@functools.lru_cache(maxsize=None)
def _exact(NQuad, key):
    """The exact bases of the shared list (key None) or of column `key` of column_mu."""
    mu = shared_mu(NQuad) if key is None else column_mu(NQuad)[key]
    return V.exact_basis(mu, V.nodes(NQuad))


def hold_to_own(NQuad, mu, X, got, label):
    """got [C, nmu, ...] against the exact interpolating polynomial of X [C, 2N, ...], the plan's own results, under the bound of
    the module docstring; a node's row bit for bit.  -> the worst error over its bound."""
    x = V.nodes(NQuad)
    N = len(x)
    per_column = np.ndim(mu) == 2
    assert got.shape == (X.shape[0], np.shape(mu)[-1]) + X.shape[2:], (label, got.shape)
    worst = 0.0
    for c in range(X.shape[0]):
        mus = mu[c] if per_column else mu
        basis = _exact(NQuad, c if per_column else None)
        Xc = X[c].reshape(2 * N, -1)
        Gc = got[c].reshape(len(mus), -1)
        for m, v in enumerate(mus):
            half = 0 if v > 0 else N
            hit = np.nonzero(abs(v) == x)[0]
            if len(hit):
                assert Gc[m].tobytes() == Xc[half + hit[0]].tobytes(), (label, c, float(v), "node row")
                continue
            lam = sum(abs(t) for t in basis[m])
            k = N + 4 + 2 * (N + 2) * lam
            gam = k * U / (1 - k * U)
            for e in range(Xc.shape[1]):
                terms = [basis[m][j] * Fraction(float(Xc[half + j, e])) for j in range(N)]
                want, size = sum(terms), sum(abs(t) for t in terms)
                err = abs(Fraction(float(Gc[m, e])) - want)
                assert err <= gam * size, (label, c, float(v), e, float(Gc[m, e]), float(want), float(err), float(gam * size))
                if size:
                    worst = max(worst, float(err / (gam * size)))
    return worst


# ---- 4. the exact interpolant of the plan's own results --------------------------------------------------------------------------
@pytest.mark.parametrize("NQuad,nt", [(6, False), (16, False), (34, False), (16, True)])
def test_view_is_the_exact_interpolant_of_the_plans_own_results(NQuad, nt):
    import pydisort_amd
    cfg = batch(NQuad, nt)
    _, sol = pydisort_amd.pydisort_batch(**cfg)
    tau = points(cfg["tau_arr"])
    for mu in (shared_mu(NQuad), column_mu(NQuad)):
        sol.plan.set_view(mu)
        for order in ORDERS:
            r = sol.plan.evaluate(tau, PHI, want=("u", "u0", "view"), **flags(order))
            assert all(np.all(np.isfinite(r[k])) for k in KEYS)
            label = f"evaluate q{NQuad} nt {nt} order {order}"
            worst = max(hold_to_own(NQuad, mu, r["u"], r["u_mu"], label), hold_to_own(NQuad, mu, r["u0"], r["u0_mu"], label))
            print(f"VIEW OWN NQuad {NQuad} nt {nt} {'per-column' if np.ndim(mu) == 2 else 'shared'} order {order:+d}: worst {worst:.3f} of the bound")
    # u left on the device gives the same bits
    only = sol.plan.evaluate(tau, PHI, want=("view",), **flags(1))
    assert only["u"] is None and np.array_equal(only["u_mu"], r["u_mu"]) and np.array_equal(only["u0_mu"], r["u0_mu"])
    sol.plan.close()


@pytest.mark.parametrize("NQuad", NQUADS)
def test_view_after_run_and_run_fetch(NQuad):
    """run() at the interfaces (the fused evaluation) + fetch() + fetch_view(); set_eval_order(+-1); run_fetch()."""
    import pydisort_amd
    cfg = batch(NQuad)
    _, sol = pydisort_amd.pydisort_batch(**cfg, _defer_solve=True)
    plan, lev, mu = sol.plan, levels(cfg["tau_arr"]), shared_mu(NQuad)
    plan.set_view(mu)
    plan.set_eval_points(lev, PHI)
    for order in ORDERS:
        plan.set_eval_order(order)
        plan.run()
        full, view = plan.fetch(), plan.fetch_view()
        label = f"run q{NQuad} order {order}"
        worst = max(hold_to_own(NQuad, mu, full["u"], view["u_mu"], label), hold_to_own(NQuad, mu, full["u0"], view["u0_mu"], label))
        out = plan.run_fetch()
        view2 = plan.fetch_view()
        label = f"run_fetch q{NQuad} order {order}"
        worst = max(worst, hold_to_own(NQuad, mu, out["u"], view2["u_mu"], label), hold_to_own(NQuad, mu, out["u0"], view2["u0_mu"], label))
        print(f"VIEW RUN NQuad {NQuad} order {order:+d}: worst {worst:.3f} of the bound")
    plan.close()


@pytest.mark.parametrize("NQuad,retain", [(6, "full"), (34, "full"), (16, "lean")])
def test_view_of_retained_plans(NQuad, retain):
    import pydisort_amd
    cfg = batch(NQuad)
    _, sol = pydisort_amd.pydisort_batch(**cfg, work_columns=4, retain=retain)
    assert sol.plan.windows() == (4, 2) and sol.plan.retained_form() == retain
    tau, mu = points(cfg["tau_arr"]), column_mu(NQuad)
    sol.plan.set_view(mu)
    for order in ORDERS:
        r = sol.plan.evaluate(tau, PHI, want=("u", "u0", "view"), **flags(order))
        label = f"{retain} q{NQuad} order {order}"
        worst = max(hold_to_own(NQuad, mu, r["u"], r["u_mu"], label), hold_to_own(NQuad, mu, r["u0"], r["u0_mu"], label))
        print(f"VIEW RETAINED {retain} NQuad {NQuad} order {order:+d}: worst {worst:.3f} of the bound")
    sol.plan.close()


# ---- 5. identical bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NQuad", NQUADS)
def test_view_bits_depend_on_neither_the_window_nor_the_sharing(NQuad):
    """work_columns = 4 (two windows, the second partial) against one window; the shared list against the same list per column."""
    import pydisort_amd
    cfg = batch(NQuad)
    tau, mu = points(cfg["tau_arr"]), shared_mu(NQuad)
    res = []
    for wc, per_column in ((0, False), (4, False), (0, True)):
        _, sol = pydisort_amd.pydisort_batch(**cfg, work_columns=wc)
        assert sol.plan.windows()[1] == (1 if wc == 0 else 2)
        sol.plan.set_view(np.tile(mu, (C, 1)) if per_column else mu)
        res.append([sol.plan.evaluate(tau, PHI, want=("view",), **flags(order)) for order in ORDERS])
        sol.plan.close()
    for other in res[1:]:
        for a, b in zip(res[0], other):
            for k in KEYS:
                assert np.all(np.isfinite(a[k])) and np.array_equal(a[k], b[k]), (k, float(np.max(np.abs(a[k] - b[k]))))


@pytest.mark.parametrize("order", ORDERS)
def test_streamed_batch_gives_the_bits_of_the_plan_driven_by_hand(order):
    import pydisort_amd
    NQuad = 16
    cfg = dict(batch(NQuad))
    cfg.pop("only_flux")
    tau, mu = points(cfg["tau_arr"]), column_mu(NQuad)
    got = pydisort_amd.solve_columns_streamed(cfg, tau, PHI, chunk_columns=4, mu=mu, tau_order=order)
    _, sol = pydisort_amd.pydisort_batch(**cfg, work_columns=4, device_prepare=True, _defer_solve=True)
    plan = sol.plan
    plan.set_view(mu)
    plan.set_eval_points(tau, PHI)
    plan.set_eval_order(order)
    out = plan.run_fetch()
    want = plan.fetch_view()
    plan.close()
    assert np.array_equal(got["u"], out["u"]) and np.array_equal(got["u0"], out["u0"])
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    # preallocated arrays, u left on the device
    mine = {k: np.full((C, tau.shape[1]), -7.0) for k in ("flux_up", "flux_down_diffuse", "flux_down_direct")}
    mine["u0"] = np.full((C, NQuad, tau.shape[1]), -7.0)
    mine["u0_mu"] = np.full((C, mu.shape[1], tau.shape[1]), -7.0)
    kept = mine["u0_mu"]
    again = pydisort_amd.solve_columns_streamed(cfg, tau, PHI, chunk_columns=4, mu=mu, tau_order=order, out=mine)
    assert again is mine and "u" not in mine and mine["u0_mu"] is kept
    assert all(np.array_equal(mine[k], want[k]) for k in KEYS) and np.array_equal(mine["u0"], out["u0"])
    flux = pydisort_amd.solve_columns_streamed(cfg, tau, None, chunk_columns=4, mu=mu, tau_order=order, only_flux=True)
    assert "u_mu" not in flux and "u" not in flux and flux["u0_mu"].shape == want["u0_mu"].shape
    assert np.max(np.abs(flux["u0_mu"] - want["u0_mu"])) <= 1e-9 * np.max(np.abs(want["u0_mu"]))  # (one mode: other kernels)


@pytest.mark.parametrize("NQuad", [8, 16, 32])
def test_band_columns_give_the_bits_of_the_batch_entry(NQuad):
    import pydisort_amd
    import test_gpu_band as B
    kw = B.band(NQuad)
    tau, om, f, leg = pydisort_amd.band_mix(kw["dtau_abs"], kw["dtau_spec"], kw["omega_spec"], kw["Leg_spec"], NQuad, delta_M=True)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=B.WEIGHTS)
    rep = lambda a: np.repeat(a, B.G, axis=0)  # noqa: E731
    _, sol = pydisort_amd.pydisort_batch(tau, om, NQuad, leg, rep(kw["mu0"]), kw["I0"].reshape(-1), rep(kw["phi0"]), f_arr=f,
                                         b_pos=rep(kw["b_pos"]), b_neg=kw["b_neg"], device_prepare=True)
    lev, mu = levels(tau), shared_mu(NQuad)
    for order in ORDERS:
        ikw = dict(is_antiderivative_wrt_tau=order < 0, is_derivative_wrt_tau=order > 0)
        for got, want in ((bsol.columns.u_at(mu, lev, PHI, **ikw), sol.u_at(mu, lev, PHI, **ikw)),
                          (bsol.columns.u0_at(mu, lev, **ikw), sol.u0_at(mu, lev, **ikw))):
            assert np.all(np.isfinite(want)) and np.max(np.abs(want)) > 0
            assert np.array_equal(got, want), float(np.max(np.abs(got - want)))
    bsol.plan.close()
    sol.plan.close()


# ---- 6. band reduction ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NQuad", [8, 32])
@pytest.mark.parametrize("work_columns", [0, 4])
def test_band_reduction_is_the_correctly_rounded_weighted_sum(NQuad, work_columns):
    import pydisort_amd
    import test_gpu_band as B
    from pydisort_amd.band import level_tau
    _, bsol = pydisort_amd.pydisort_band(**B.band(NQuad), weights=B.WEIGHTS, work_columns=work_columns)
    plan = bsol.plan
    assert plan.windows()[1] == (1 if work_columns == 0 else 4)
    x = V.nodes(NQuad)
    mu = np.array([[0.9, x[1], 0.0, -0.45], [0.2, -x[0], 1.0, -1.0], [0.55, 0.37, -0.0, -0.62]])  # [P, nmu]
    nmu = mu.shape[1]
    plan.set_view(np.repeat(mu, B.G, axis=0))
    lev = level_tau(plan.prep["tau"])
    plan.set_eval_points(lev, PHI)
    plan.run()
    red, full = plan.fetch_band_view(), plan.fetch_view()
    worst = 0.0
    for k, tail in (("u_mu", (nmu, B.L + 1, len(PHI))), ("u0_mu", (nmu, B.L + 1))):
        assert red[k].shape == (B.P, B.K) + tail and full[k].shape == (B.P * B.G,) + tail
        assert np.all(np.isfinite(full[k])) and np.max(np.abs(full[k])) > 0
        worst = max(worst, B.hold_reduced(red[k], full[k], B.WEIGHTS))
    sub = level_tau(plan.prep["tau"], [1, 3])
    for order in ORDERS:
        r = plan.evaluate_band(sub, PHI, want=("view",), **flags(order))
        f = plan.fetch_view()
        for k in KEYS:
            worst = max(worst, B.hold_reduced(r[k], f[k], B.WEIGHTS))
    # the evaluators, per profile angles
    got = bsol.u_at(mu, [1, 3], PHI)
    assert got.shape == (B.P, B.K, nmu, 2, len(PHI)) and np.array_equal(got, plan.evaluate_band(sub, PHI, want=("view_u",))["u_mu"])
    assert bsol.u0_at(mu[0]).shape == (B.P, B.K, nmu, B.L + 1)
    with pytest.raises(ValueError, match="same for the columns of a band profile"):
        bad = np.repeat(mu, B.G, axis=0)
        bad[1, 0] = 0.91
        plan.set_view(bad)
    plan.close()
    print(f"VIEW REDUCE NQuad {NQuad} work_columns {work_columns}: worst {worst:.3f} ulp of the exact weighted sum")


def test_streamed_band_agrees_with_the_evaluators():
    import pydisort_amd
    import test_gpu_band as B
    kw = B.band(8)
    mu = shared_mu(8)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=B.WEIGHTS)
    ref = (bsol.u_at(mu, None, PHI), bsol.u0_at(mu))
    bsol.plan.close()
    out = pydisort_amd.solve_band_streamed(**kw, weights=B.WEIGHTS, phi=PHI, chunk_columns=4, mu=mu)
    plain = pydisort_amd.solve_band_streamed(**kw, weights=B.WEIGHTS, phi=PHI, chunk_columns=4)
    assert not any(k in plain for k in KEYS) and np.array_equal(plain["u"], out["u"])
    for k, want in zip(KEYS, ref):
        assert out[k].shape == want.shape
        assert np.max(np.abs(out[k] - want)) <= 1e-9 * np.max(np.abs(want)), k  # (windows of 4, the fused evaluation: other kernels)
    one = pydisort_amd.solve_band_streamed(**kw, weights=B.WEIGHTS[1], levels=[0, B.L], only_flux=True, mu=np.tile(mu, (B.P, 1)))
    assert "u_mu" not in one and one["u0_mu"].shape == (B.P, len(mu), 2)


def test_a_bad_profile_is_nan_and_the_others_keep_their_results():
    """The bad profile of tests/test_gpu_band.py (a species whose first moment is 2.5: mode 0 of profile 1 fails)."""
    import pydisort_amd
    import test_gpu_band as B
    kw = dict(B.band(8))
    leg = kw["Leg_spec"].copy()
    leg[1, 1:] = 0.0
    leg[1, 1] = 2.5
    ds, om = kw["dtau_spec"].copy(), kw["omega_spec"].copy()
    ds[:, :, 1] = 0.0
    ds[1, :, 1] = 5.0
    om[1, :, 1] = 0.97
    kw.update(Leg_spec=leg, dtau_spec=ds, omega_spec=om)
    mu = shared_mu(8)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=B.WEIGHTS, numeric_errors="nan")
    bsol.plan.set_view(mu)
    lev = levels(bsol.plan.prep["tau"])
    red = bsol.plan.evaluate_band(lev, PHI, want=("view",))
    full = bsol.plan.evaluate(lev, PHI, want=("view",))
    for k in KEYS:
        assert np.all(np.isnan(red[k][1])) and np.all(np.isnan(full[k][B.G:2 * B.G])), k
        assert np.all(np.isfinite(red[k][[0, 2]])), k
        B.hold_reduced(red[k], full[k], B.WEIGHTS, profiles=(0, 2))
    _, raising = pydisort_amd.pydisort_band(**kw, weights=B.WEIGHTS)
    with pytest.raises(pydisort_amd._lib.NumericalError):
        raising.u0_at(mu)
    for s in (bsol, raising):
        s.plan.close()


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------
def hold_to_reference(name, got, want, lam, against):
    """1e-9 Lambda(mu) of the scale of `want`, point by point; `got`, `want` [nmu, ...], lam [nmu]."""
    from conftest import record_parity
    import goldens
    scale = np.max(np.abs(want))
    assert scale > 0
    weighted = float(np.max(np.abs(got - want) / (lam.reshape((-1,) + (1,) * (want.ndim - 1)) * scale)))
    print(f"VIEW {against.upper()} {name}: {weighted:.2e} of Lambda x the scale (bar {V.TOL:.0e}), Lambda <= {np.max(lam):.2f}")
    record_parity(f"view/{name}", weighted, goldens.max_rel_err(got, want)[1], V.TOL, None, against=against, lebesgue_max=float(np.max(lam)))


@pytest.mark.parametrize("name", sorted(V.cases()))
def test_u_at_matches_the_reference_fixtures(name):
    """One fixture case as a batch of two equal columns, and the drop-in pydisort + subroutines.interpolate on the same case."""
    import pydisort_amd
    from pydisort_amd import subroutines
    kw = V.cases()[name]
    g = V.load(name)
    mu, tau, phi = g["mu"], g["tau"], g["phi"]
    lam = V.lebesgue(mu, V.nodes(kw["NQuad"]))
    lead = lambda v: np.stack((v, v)) if isinstance(v, np.ndarray) else v  # noqa: E731
    bkw = {k: lead(v) for k, v in kw.items() if k not in ("NQuad", "NLeg", "only_flux", "NT_cor")}
    bkw.update({k: np.full(2, float(kw[k])) for k in ("mu0", "I0", "phi0")})
    _, sol = pydisort_amd.pydisort_batch(NQuad=kw["NQuad"], NLeg=kw["NLeg"], NT_cor=bool(kw.get("NT_cor")), **bkw)
    res = pydisort_amd.pydisort(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    drop_u, drop_u0 = subroutines.interpolate(res[4]), subroutines.interpolate(res[3])
    for suffix, antider in (("", False), (".antider", True)):
        if antider and name in V.VALUE_ONLY:
            continue
        got_u, got_u0 = sol.u_at(mu, tau, phi, antider), sol.u0_at(mu, tau, antider)
        assert np.array_equal(got_u[0], got_u[1]) and np.array_equal(got_u0[0], got_u0[1])
        hold_to_reference(f"{name}/batch/u_mu{suffix}", got_u[0], g["u_mu" + suffix], lam, "reference")
        hold_to_reference(f"{name}/batch/u0_mu{suffix}", got_u0[0], g["u0_mu" + suffix], lam, "reference")
        hold_to_reference(f"{name}/drop_in/u_mu{suffix}", np.asarray(drop_u(mu, tau, phi, antider)), g["u_mu" + suffix], lam, "reference")
        hold_to_reference(f"{name}/drop_in/u0_mu{suffix}", np.asarray(drop_u0(mu, tau, antider)), g["u0_mu" + suffix], lam, "reference")
    with pytest.raises(ValueError, match="mu values must be between -1 and 1."):
        sol.u_at([0.5, 1.5], tau, phi)
    with pytest.raises(ValueError):
        sol.u0_at(mu, tau, True, is_derivative_wrt_tau=True)
    sol.plan.close()


@functools.lru_cache(maxsize=None)
def oracle_nodes(NQuad):
    """[order] -> (u [C, 2N, ntau, nphi], u0 [C, 2N, ntau]) of the CPU oracle at points(tau_arr); once per shape, shared."""
    import test_gpu_actinic as T
    cfg = batch(NQuad)
    tau = points(cfg["tau_arr"])
    out = {order: (np.empty((C, NQuad, tau.shape[1], len(PHI))), np.empty((C, NQuad, tau.shape[1]))) for order in ORDERS}
    for c in range(C):
        u, u0 = V.oracle(T.column_kwargs(cfg, c))
        for order in ORDERS:
            out[order][0][c] = u(tau[c], PHI, order < 0, is_derivative_wrt_tau=order > 0)
            out[order][1][c] = u0(tau[c], order < 0, is_derivative_wrt_tau=order > 0)
    return out


@pytest.mark.parametrize("NQuad", NQUADS)
def test_u_at_matches_the_oracle_and_the_model(NQuad):
    import pydisort_amd
    cfg = batch(NQuad)
    tau, mu, x = points(cfg["tau_arr"]), column_mu(NQuad), V.nodes(NQuad)
    _, sol = pydisort_amd.pydisort_batch(**cfg)
    for order in ORDERS:
        kw = dict(is_antiderivative_wrt_tau=order < 0, is_derivative_wrt_tau=order > 0)
        got_u, got_u0 = sol.u_at(mu, tau, PHI, **kw), sol.u0_at(mu, tau, **kw)
        for c in range(C):
            lam = V.lebesgue(mu[c], x)
            hold_to_reference(f"q{NQuad}/order{order:+d}/col{c}/u_mu", got_u[c], V.interpolate(mu[c], x, oracle_nodes(NQuad)[order][0][c]), lam, "oracle")
            hold_to_reference(f"q{NQuad}/order{order:+d}/col{c}/u0_mu", got_u0[c], V.interpolate(mu[c], x, oracle_nodes(NQuad)[order][1][c]), lam, "oracle")
    sol.plan.close()


def test_view_of_mode_shards_sums_to_the_unsharded_result():
    import pydisort_amd
    NQuad = 16
    cfg = dict(batch(NQuad), NFourier=4)
    tau, mu, x = points(cfg["tau_arr"]), column_mu(NQuad), V.nodes(NQuad)
    lam = np.stack([V.lebesgue(mu[c], x) for c in range(C)])
    _, whole = pydisort_amd.pydisort_batch(**cfg)
    parts = [pydisort_amd.pydisort_batch(**cfg, mode_shard=(r, 2))[1] for r in range(2)]
    for s in parts + [whole]:
        s.plan.set_view(mu)
    for order in ORDERS:
        w = whole.plan.evaluate(tau, PHI, want=("view",), **flags(order))
        p = [s.plan.evaluate(tau, PHI, want=("view",), **flags(order)) for s in parts]
        assert np.any(p[1]["u_mu"] != 0.0)  # (the shard without mode 0 carries its part of u)
        for k in KEYS:
            tol = V.TOL * lam.reshape(lam.shape + (1,) * (w[k].ndim - 2)) * np.max(np.abs(w[k]))
            assert np.all(np.abs(p[0][k] + p[1][k] - w[k]) <= tol), (order, k)
    for s in parts + [whole]:
        s.plan.close()


# ---- 8. nothing else moves --------------------------------------------------------------------------------------------------------------
def test_a_request_changes_no_other_result_and_no_request_holds_nothing_more():
    import pydisort_amd
    cfg = batch(6)
    tau = points(cfg["tau_arr"])
    pydisort_amd.pool_trim()  # (both plans carved from fresh blocks of the sizes they ask for: tests/test_gpu_actinic.py)
    _, sol = pydisort_amd.pydisort_batch(**cfg)
    pydisort_amd.pool_trim()
    _, twin = pydisort_amd.pydisort_batch(**cfg)
    with pytest.raises(ValueError, match="set_view must precede"):
        sol.plan.fetch_view()
    sol.plan.set_view(shared_mu(6))
    with pytest.raises(RuntimeError, match="nothing to fetch"):
        sol.plan.fetch_view()
    assert sol.plan.device_bytes() == twin.plan.device_bytes()  # (the request alone holds nothing)
    a = sol.plan.evaluate(tau, PHI, want=("u", "u0", "flux", "view"))
    b = twin.plan.evaluate(tau, PHI, want=("u", "u0", "flux"))
    for k in ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct"):
        assert np.array_equal(a[k], b[k]), k
    nmu, nt = len(shared_mu(6)), tau.shape[1]
    held = 8 * (nmu + 3 + nmu * 3 + C * nmu * nt * (len(PHI) + 1))  # angles, weights, basis, the two interpolated arrays
    assert sol.plan.device_bytes() >= twin.plan.device_bytes() + held  # (the view buffers came with the first fetch, and only there)
    sol.plan.evaluate(tau, None, want=("u0",))
    with pytest.raises(RuntimeError, match="formed no u"):
        sol.plan._checked(sol.plan._lib.rtd_plan_fetch_view(sol.plan._h, a["u_mu"].ctypes.data, None), {})
    assert sol.plan.fetch_view()["u_mu"] is None  # (no azimuths in the latest evaluation: u0_mu alone)
    sol.plan.evaluate(tau, PHI, want=("u0",))  # azimuths, but u was not wanted: none was formed
    with pytest.raises(RuntimeError, match="formed no u"):
        sol.plan.fetch_view()
    sol.plan.set_view(None)
    with pytest.raises(ValueError, match="set_view must precede"):
        sol.plan.fetch_view()
    sol.plan.close()
    twin.plan.close()


def test_the_c_example_prints_what_u_at_returns(tmp_path):
    """examples/solve_columns.c (plain C99, -pedantic -Werror) ends with rtd_plan_set_view_mu + rtd_plan_fetch_view on the inputs
    of tests/test_gpu_c_example.py: its "view" lines against BatchSolution.u_at (the nodes come from a Newton iteration in C there
    and from numpy here: agreement to 1e-12, as that test)."""
    import os
    import re
    import shutil
    import subprocess
    import pydisort_amd
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "pythonic-disort_amd", "pydisort_amd")
    exe = str(tmp_path / "solve_columns")
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-O2", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "solve_columns.c"), os.path.join(libdir, "librtd.so"), "-lm", "-Wl,-rpath," + libdir, "-o", exe],
                   check=True)
    Cn, Ln, NQ = 4, 3, 16
    r = subprocess.run([exe, str(Cn)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [[float(v) for v in re.findall(r"\] ([-+]?\d\.\d+(?:e[-+]?\d+)?)", ln)] for ln in r.stdout.splitlines() if ln.startswith("view")]
    assert len(rows) == Cn and all(len(v) == 2 for v in rows), r.stdout
    c, l = np.arange(Cn)[:, None], np.arange(Ln)[None, :]
    g = 0.55 + 0.1 * l + 0.01 * c
    cfg = dict(tau_arr=0.4 * (l + 1) * (1.0 + 0.05 * c), omega_arr=np.broadcast_to(0.95 - 0.1 * l, (Cn, Ln)).copy(), NQuad=NQ,
               Leg_coeffs_all=g[:, :, None] ** np.arange(NQ + 1)[None, None, :], mu0=0.3 + 0.6 * (np.arange(Cn) + 1.0) / (Cn + 1.0),
               I0=np.full(Cn, 3.0), phi0=np.full(Cn, 0.5), f_arr=g ** NQ)
    _, sol = pydisort_amd.pydisort_batch(**cfg)
    tau = np.stack([np.zeros(Cn), 0.37 * cfg["tau_arr"][:, -1]], axis=1)
    u = sol.u_at([0.8, -0.6], tau, np.array([0.0, 2.0]))
    want = np.stack([u[:, 0, 0, 0], u[:, 1, 1, 1]], axis=1)
    assert np.allclose(np.array(rows), want, rtol=1e-12, atol=1e-14), np.max(np.abs(np.array(rows) - want) / np.abs(want))
    sol.plan.close()
