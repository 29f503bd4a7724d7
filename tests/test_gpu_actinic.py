"""Actinic fluxes on the device: Plan.fetch_actinic / fetch_band_actinic, want=("act",), BatchSolution.flux_act_up / flux_act_down,
BandSolution.flux_act_up / flux_act_down / actinic_flux and actinic=True of the two streamed forms (include/rtd.h:
rtd_plan_fetch_actinic, rtd_plan_fetch_band_actinic; csrc/rtd_api.hip: rtd_actinic_kernel).

Shapes: 6 columns x 3 layers; 6, 16 and 34 streams (N = 3, 8, 17: no power of two, every padded class of u0); NLeg = NQuad of
NQuad + 3 Henyey-Greenstein moments, f_arr = moment NLeg; column 4 has f_arr = 0, column 2 has I0 = 0, column 1 has a surface
source above its beam (rescale != I0); every column its own mu0.  Points: tau = 0, each interface (the last one is the bottom) and
two interior points.

Every bound is derived, none is measured.  With u = 2^-53, gamma_k = k u / (1 - k u), x the plan's OWN fetched u0, w = prep["W"]:

* sums: the kernel forms fl(2 pi) sum_i w_i x_i with N products (fused or not), N - 1 additions and one multiplication by
  fl(2 pi): N + 1 roundings at most, held to the exact rational sum (fractions.Fraction) within gamma_{N+2} fl(2 pi) sum |w_i x_i|;
* exponential terms: I0 e^(-tau*/mu0) and I0 e^(-tau/mu0) times their order factors, against mpmath on the exact float64 inputs.
  tau* = taus0[l+1] - (tau_arr[l] - tau) sc takes three roundings, each at most u times a magnitude below
  taus0[l+1] + (tau_arr[l] - tau) sc, and the quotient by mu0 one more: 4 X u in the exponent, X = that sum over mu0, which is the
  relative error of the exponential; a 1-ulp exp (2 u), rescale I0 and its product with the exponential (2 u), -sc/mu0 and its
  application (2 u): (6 + 4 X) u, held at (8 + 4 X) u |term|;
* act_down_diffuse = sums + R: R = es - ed rounds once (u |R| <= u (|es| + |ed|): inside the 2 u per term that the line above
  leaves unused) and the final addition once more: u |result| on top of the two bounds above.

End to end (oracle u0 + closed forms, tests/actinic_cases.py) and against the drop-in's generate_diff_act_flux_funcs: the
project's standing 1e-9 of each output's scale over the batch.  Reduction: as tests/test_gpu_band.py, one ulp of the exact
weighted sum + 2^-90 sum |w x|.  Each test prints its worst ratio to its bound.

Figures seen on an MI355X: against the plan's own u0 at worst 0.39 of the bound (evaluate, retained plans) and 0.34 (run,
run_fetch); identical bits for one window and windows of 4, for the streamed form and the plan driven by hand, and for the band
entry and the batch entry; against the truth 1.2e-12 of the scale (34 streams; 1.2e-13 with thermal sources, 1.5e-14 for the mode
shards), against the drop-in 2.4e-16, of the 1e-9 allowed; reduction 0.499 ulp of the 1 ulp + 2^-90 sum |w x| allowed."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import actinic_cases as A

pytestmark = pytest.mark.gpu

C, L = 6, 3
NQUADS = (6, 16, 34)
KEYS = A.KEYS
U = Fraction(1, 2 ** 53)
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def batch(NQuad, beam=True):
    """Keyword arguments of pydisort_batch for the batch of every test (built once per shape and left unchanged)."""
    rng = np.random.default_rng(500 + NQuad)
    g = rng.uniform(0.55, 0.8, (C, 1, 1))
    leg = np.broadcast_to(g ** np.arange(NQuad + 3)[None, None, :], (C, L, NQuad + 3)).copy()
    f = leg[:, :, NQuad].copy()
    f[4] = 0.0
    I0 = rng.uniform(0.5, 2.0, C)
    I0[2] = 0.0
    b_pos = rng.uniform(0.0, 0.3, C)
    b_pos[1] = 3.0  # above the column's beam: rescale is not I0 there
    cfg = dict(tau_arr=np.cumsum(rng.uniform(0.15, 0.8, (C, L)), axis=1), omega_arr=rng.uniform(0.5, 0.97, (C, L)), NQuad=NQuad,
               Leg_coeffs_all=leg, mu0=rng.uniform(0.3, 0.95, C), I0=I0 if beam else np.zeros(C), phi0=rng.uniform(0.0, 6.0, C), NLeg=NQuad,
               f_arr=f, b_pos=b_pos, only_flux=True)
    for v in cfg.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cfg


def column_kwargs(cfg, c, **extra):
    """One column of a batch as keyword arguments of the one-column ``pydisort`` (the oracle's and the drop-in's)."""
    kw = {k: (v[c] if isinstance(v, np.ndarray) else v) for k, v in cfg.items()}
    for k in ("mu0", "I0", "phi0", "b_pos"):
        if np.ndim(kw[k]) == 0:
            kw[k] = float(kw[k])
    kw.update(extra)
    return kw


def points(tau_arr):
    t1, t2, t3 = tau_arr[:, 0], tau_arr[:, 1], tau_arr[:, 2]
    return np.ascontiguousarray(np.stack((np.zeros(len(t1)), t1, t2, t3, 0.4 * t1, t1 + 0.6 * (t2 - t1)), axis=1))


def levels(tau_arr):
    return np.ascontiguousarray(np.concatenate((np.zeros((len(tau_arr), 1)), tau_arr), axis=1))


def hold_to_own_u0(prep, tau, order, u0, act, label):
    """The three arrays against the plan's own u0 and its prepared float64 inputs under the bounds of the module docstring.
    -> the worst error over its bound."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 40
    N = prep["N"]
    u = mp.mpf(2) ** -53
    two_pi = Fraction(float(2.0 * np.pi))
    gam = (N + 2) * U / (1 - (N + 2) * U)
    W = [Fraction(float(v)) for v in prep["W"]]
    worst = 0.0
    fr = lambda q: mp.mpf(q.numerator) / mp.mpf(q.denominator)  # noqa: E731
    for c in range(u0.shape[0]):
        for t in range(u0.shape[2]):
            sums, mags = [], []
            for half in (0, N):
                terms = [W[i] * Fraction(float(u0[c, half + i, t])) for i in range(N)]
                sums.append(two_pi * sum(terms))
                mags.append(gam * two_pi * sum(abs(v) for v in terms))
            es = ed = term_bound = mp.mpf(0)
            beam = bool(prep["beam"]) and float(prep["I0"][c]) != 0.0
            if beam:
                x, mu0 = mp.mpf(float(tau[c, t])), mp.mpf(float(prep["mu0"][c]))
                I0 = mp.mpf(float(prep["rescale"][c])) * mp.mpf(float(prep["I0"][c]))
                l = int(np.argmax(tau[c, t] <= prep["tau"][c]))
                sc = mp.mpf(float(prep["scale_tau"][c, l]))
                far = (mp.mpf(float(prep["tau"][c, l])) - x) * sc
                top = mp.mpf(float(prep["tau_s0"][c, l + 1]))
                X = (top + far) / mu0
                es, ed = I0 * mp.exp(-(top - far) / mu0), I0 * mp.exp(-x / mu0)
                if order < 0:
                    es, ed = es / (-sc / mu0), ed * (-mu0)
                elif order > 0:
                    es, ed = es * (-sc / mu0), ed / (-mu0)
                term_bound = (8 + 4 * X) * u
            got = [mp.mpf(float(act[k][c, t])) for k in KEYS]
            want = [fr(sums[0]), fr(sums[1]) + es - ed, ed]
            bound = [fr(mags[0]), fr(mags[1]) + term_bound * (abs(es) + abs(ed)) + u * abs(want[1]), term_bound * abs(ed)]
            for k in range(3):
                err = abs(got[k] - want[k])
                assert err <= bound[k], (label, KEYS[k], c, t, float(got[k]), float(want[k]), float(err), float(bound[k]))
                if bound[k] > 0:
                    worst = max(worst, float(err / bound[k]))
            if not beam:
                assert act[KEYS[2]][c, t] == 0.0
    return worst


def flags(order):
    return dict(antiderivative=order < 0, derivative=order > 0)


# ---- 1. the weighted sum of the plan's own u0 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("NQuad", NQUADS)
def test_actinic_is_the_weighted_sum_of_the_plans_own_u0(NQuad):
    import pydisort_amd
    cfg = batch(NQuad)
    _, sol = pydisort_amd.pydisort_batch(**cfg)
    tau = points(cfg["tau_arr"])
    for order in A.ORDERS:
        r = sol.plan.evaluate(tau, None, want=("u0", "act"), **flags(order))
        assert all(r[k].shape == (C, tau.shape[1]) and np.all(np.isfinite(r[k])) for k in KEYS)
        assert np.all(r[KEYS[2]][2] == 0.0) and np.all(r[KEYS[2]][[0, 1, 3, 4, 5]] != 0.0)  # (column 2 has no beam)
        worst = hold_to_own_u0(sol.prep, tau, order, r["u0"], r, f"q{NQuad} order {order}")
        print(f"ACTINIC OWN-U0 NQuad {NQuad} order {order:+d}: worst {worst:.3f} of the bound")
    sol.plan.close()


# ---- 2. every path that fills the result buffers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("NQuad", NQUADS)
def test_actinic_after_run_and_run_fetch(NQuad):
    """run() at the interfaces (the fused evaluation) + fetch() + fetch_actinic(); set_eval_order(+-1); run_fetch()."""
    import pydisort_amd
    cfg = batch(NQuad)
    _, sol = pydisort_amd.pydisort_batch(**cfg, _defer_solve=True)
    plan, lev = sol.plan, levels(cfg["tau_arr"])
    plan.set_eval_points(lev, np.array([0.0]))
    for order in A.ORDERS:
        plan.set_eval_order(order)
        plan.run()
        full, act = plan.fetch(), plan.fetch_actinic()
        worst = hold_to_own_u0(sol.prep, lev, order, full["u0"], act, f"run q{NQuad} order {order}")
        out = plan.run_fetch()
        act2 = plan.fetch_actinic()
        worst = max(worst, hold_to_own_u0(sol.prep, lev, order, out["u0"], act2, f"run_fetch q{NQuad} order {order}"))
        print(f"ACTINIC RUN NQuad {NQuad} order {order:+d}: worst {worst:.3f} of the bound")
    plan.close()


@pytest.mark.parametrize("NQuad,retain", [(6, "full"), (34, "full"), (16, "lean")])
def test_actinic_of_retained_plans(NQuad, retain):
    import pydisort_amd
    cfg = batch(NQuad)
    _, sol = pydisort_amd.pydisort_batch(**cfg, work_columns=4, retain=retain)
    assert sol.plan.windows() == (4, 2) and sol.plan.retained_form() == retain
    tau = points(cfg["tau_arr"])
    for order in A.ORDERS:
        r = sol.plan.evaluate(tau, None, want=("u0", "act"), **flags(order))
        worst = hold_to_own_u0(sol.prep, tau, order, r["u0"], r, f"{retain} q{NQuad} order {order}")
        print(f"ACTINIC RETAINED {retain} NQuad {NQuad} order {order:+d}: worst {worst:.3f} of the bound")
    sol.plan.close()


@pytest.mark.parametrize("NQuad", NQUADS)
def test_actinic_bits_do_not_depend_on_the_window(NQuad):
    """work_columns = 4 (two windows, the second partial) against one window."""
    import pydisort_amd
    cfg = batch(NQuad)
    tau = points(cfg["tau_arr"])
    res = []
    for wc in (0, 4):
        _, sol = pydisort_amd.pydisort_batch(**cfg, work_columns=wc)
        assert sol.plan.windows()[1] == (1 if wc == 0 else 2)
        res.append([sol.plan.evaluate(tau, None, want=("act",), **flags(order)) for order in A.ORDERS])
        sol.plan.close()
    for a, b in zip(*res):
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), (k, float(np.max(np.abs(a[k] - b[k]))))


@pytest.mark.parametrize("order", A.ORDERS)
def test_streamed_batch_gives_the_bits_of_the_plan_driven_by_hand(order):
    import pydisort_amd
    cfg = dict(batch(16))
    cfg.pop("only_flux")
    tau = points(cfg["tau_arr"])
    got = pydisort_amd.solve_columns_streamed(cfg, tau, None, chunk_columns=4, only_flux=True, actinic=True, tau_order=order)
    _, sol = pydisort_amd.pydisort_batch(**cfg, only_flux=True, work_columns=4, device_prepare=True, _defer_solve=True)
    plan = sol.plan
    plan.set_eval_points(tau, np.array([0.0]))
    plan.set_eval_order(order)
    out = plan.run_fetch()
    want = plan.fetch_actinic()
    plan.close()
    assert np.array_equal(got["u0"], out["u0"])
    for k in KEYS:
        assert got[k].shape == (C, tau.shape[1]) and np.array_equal(got[k], want[k]), k
    # preallocated arrays, u0 left on the device
    mine = {k: np.full((C, tau.shape[1]), -7.0) for k in KEYS + ("flux_up", "flux_down_diffuse", "flux_down_direct")}
    again = pydisort_amd.solve_columns_streamed(cfg, tau, None, chunk_columns=4, only_flux=True, actinic=True, tau_order=order, out=mine)
    assert again is mine and "u0" not in mine and all(np.array_equal(mine[k], want[k]) for k in KEYS)
    with pytest.raises(ValueError, match="flux_act_up"):
        pydisort_amd.solve_columns_streamed(cfg, tau, None, chunk_columns=4, only_flux=True, actinic=True,
                                            out=dict(mine, flux_act_up=np.zeros((C, 2))))


# ---- 3. end to end against the truth of tests/actinic_cases.py ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_truth(NQuad, beam=True):
    """[order] -> dict of [C, ntau] arrays at points(tau_arr); computed once per shape and shared."""
    cfg = batch(NQuad, beam)
    tau = points(cfg["tau_arr"])
    out = {order: {k: np.empty(tau.shape) for k in KEYS} for order in A.ORDERS}
    for c in range(C):
        kw = column_kwargs(cfg, c)
        sol = A.solve(kw)
        for order in A.ORDERS:
            t = A.truth(kw, tau[c], order, sol)
            for k in KEYS:
                out[order][k][c] = t[k]
    return out


def hold_to_truth(name, got, want):
    from conftest import record_parity
    import goldens
    for k in KEYS:
        if np.max(np.abs(want[k])) == 0.0:
            assert np.all(got[k] == 0.0), (name, k)
            continue
        a, b = goldens.max_rel_err(got[k], want[k])
        print(f"ACTINIC TRUTH {name} {k}: {a:.2e} of the scale (bar {TOL:.0e}), {b:.2e} pointwise")
        record_parity(f"actinic/{name}/{k}", a, b, TOL, None, against="oracle")


@pytest.mark.parametrize("NQuad", NQUADS)
@pytest.mark.parametrize("device_prepare", [False, True])
def test_actinic_matches_the_truth(NQuad, device_prepare):
    import pydisort_amd
    cfg = batch(NQuad)
    _, sol = pydisort_amd.pydisort_batch(**cfg, device_prepare=device_prepare)
    tau = points(cfg["tau_arr"])
    for order in A.ORDERS:
        kw = dict(is_antiderivative_wrt_tau=order < 0, is_derivative_wrt_tau=order > 0)
        dd, dr = sol.flux_act_down(tau, **kw)
        got = dict(flux_act_up=sol.flux_act_up(tau, **kw), flux_act_down_diffuse=dd, flux_act_down_direct=dr)
        hold_to_truth(f"q{NQuad}/{'device' if device_prepare else 'host'}_prepared/order{order:+d}", got, oracle_truth(NQuad)[order])
    sol.plan.close()


@pytest.mark.parametrize("beam", [True, False])
def test_actinic_with_thermal_sources_matches_the_truth(beam):
    """thermal=: sources formed on the device from temperatures; the truth takes them from 40-digit band integrals on the host.
    Without a beam R = D = 0 exactly."""
    import pydisort_amd
    import test_gpu_thermal_batch as T
    NQuad, N = 16, 8
    cfg = dict(batch(NQuad, beam))
    rng = np.random.default_rng(77)
    th = dict(TEMPER=np.sort(rng.uniform(200.0, 300.0, (C, L + 1)), axis=1), WVNMLO=np.full(C, 500.0), WVNMHI=np.full(C, 900.0),
              BTEMP=rng.uniform(280.0, 310.0, C), TTEMP=np.full(C, 60.0), TEMIS=np.full(C, 0.8))
    _, sol = pydisort_amd.pydisort_batch(**cfg, thermal=th)
    tau = points(cfg["tau_arr"])
    host = dict(cfg, b_pos=np.broadcast_to(cfg["b_pos"][:, None], (C, N)))
    sp, b_pos, b_neg = T._host_sources(dict(host, b_neg=np.zeros(C)), th, np.ones((C, N)))
    for order in A.ORDERS:
        r = sol.plan.evaluate(tau, None, want=("act",), **flags(order))
        want = {k: np.empty(tau.shape) for k in KEYS}
        for c in range(C):
            kw = column_kwargs(cfg, c, b_pos=b_pos[c], b_neg=b_neg[c], s_poly_coeffs=sp[c])
            t = A.truth(kw, tau[c], order)
            for k in KEYS:
                want[k][c] = t[k]
        if not beam:
            assert np.all(r[KEYS[2]] == 0.0) and np.all(want[KEYS[2]] == 0.0)
        hold_to_truth(f"q{NQuad}/thermal_{'beam' if beam else 'only'}/order{order:+d}", r, want)
    sol.plan.close()


def test_actinic_of_mode_shards_sums_to_the_unsharded_result():
    import pydisort_amd
    NQuad = 16
    cfg = dict(batch(NQuad), only_flux=False, NFourier=4)
    tau = points(cfg["tau_arr"])
    _, whole = pydisort_amd.pydisort_batch(**cfg)
    parts = [pydisort_amd.pydisort_batch(**cfg, mode_shard=(r, 2))[1] for r in range(2)]
    for order in A.ORDERS:
        w = whole.plan.evaluate(tau, None, want=("act",), **flags(order))
        p = [s.plan.evaluate(tau, None, want=("act",), **flags(order)) for s in parts]
        for k in KEYS:
            assert np.all(p[1][k] == 0.0), k  # (the shard without mode 0)
            assert np.array_equal(p[0][k] + p[1][k], p[0][k])
            assert np.max(np.abs(p[0][k] - w[k])) <= TOL * np.max(np.abs(w[k])), k
        hold_to_truth(f"q{NQuad}/mode_shards/order{order:+d}", {k: p[0][k] + p[1][k] for k in KEYS}, oracle_truth(NQuad)[order])
    for s in parts + [whole]:
        s.plan.close()


# ---- 4. the drop-in's host functions ------------------------------------------------------------------------------------------------
def test_batch_agrees_with_the_drop_ins_generate_diff_act_flux_funcs():
    import goldens
    import pydisort_amd
    from pydisort_amd import subroutines
    NQuad = 16
    cfg = batch(NQuad)
    tau = points(cfg["tau_arr"])
    _, sol = pydisort_amd.pydisort_batch(**cfg)
    got = {order: sol.plan.evaluate(tau, None, want=("act",), **flags(order)) for order in A.ORDERS}
    want = {order: {k: np.empty(tau.shape) for k in KEYS[:2]} for order in A.ORDERS}
    for c in range(C):
        res = pydisort_amd.pydisort(**column_kwargs(cfg, c))
        up, down = subroutines.generate_diff_act_flux_funcs(res[3])
        for order in A.ORDERS:
            kw = {"is_derivative_wrt_tau": True} if order > 0 else {}
            want[order][KEYS[0]][c] = up(tau[c], order < 0, **kw)
            want[order][KEYS[1]][c] = down(tau[c], order < 0, **kw)
    for order in A.ORDERS:
        for k in KEYS[:2]:
            a, _ = goldens.max_rel_err(got[order][k], want[order][k])
            print(f"ACTINIC DROP-IN order {order:+d} {k}: {a:.2e} of the scale (bar {TOL:.0e})")
            assert a < TOL, (order, k, a)
    sol.plan.close()


# ---- 5. bands -------------------------------------------------------------------------------------------------------------------------
def test_band_columns_give_the_bits_of_the_batch_entry():
    import pydisort_amd
    import test_gpu_band as B
    NQuad = 16
    kw = B.band(NQuad)
    tau, om, f, leg = pydisort_amd.band_mix(kw["dtau_abs"], kw["dtau_spec"], kw["omega_spec"], kw["Leg_spec"], NQuad, delta_M=True)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=B.WEIGHTS)
    rep = lambda a: np.repeat(a, B.G, axis=0)  # noqa: E731
    _, sol = pydisort_amd.pydisort_batch(tau, om, NQuad, leg, rep(kw["mu0"]), kw["I0"].reshape(-1), rep(kw["phi0"]), f_arr=f,
                                         b_pos=rep(kw["b_pos"]), b_neg=kw["b_neg"], device_prepare=True)
    lev = levels(tau)
    for order in A.ORDERS:
        ikw = dict(is_antiderivative_wrt_tau=order < 0, is_derivative_wrt_tau=order > 0)
        for got, want in ((bsol.columns.flux_act_up(lev, **ikw), sol.flux_act_up(lev, **ikw)),
                          (bsol.columns.flux_act_down(lev, **ikw)[0], sol.flux_act_down(lev, **ikw)[0]),
                          (bsol.columns.flux_act_down(lev, **ikw)[1], sol.flux_act_down(lev, **ikw)[1])):
            assert np.all(np.isfinite(want)) and np.max(np.abs(want)) > 0
            assert np.array_equal(got, want), float(np.max(np.abs(got - want)))
    bsol.plan.close()
    sol.plan.close()


@functools.lru_cache(maxsize=None)
def _band_reduced_and_full(NQuad, work_columns):
    import pydisort_amd
    import test_gpu_band as B
    from pydisort_amd.band import level_tau
    _, bsol = pydisort_amd.pydisort_band(**B.band(NQuad), weights=B.WEIGHTS, work_columns=work_columns)
    plan = bsol.plan
    assert plan.windows()[1] == (1 if work_columns == 0 else 4)
    lev = level_tau(plan.prep["tau"])
    plan.set_eval_points(lev, np.array([0.0]))
    plan.run()
    out = {"fetch": (plan.fetch_band_actinic(), plan.fetch_actinic())}
    sub = level_tau(plan.prep["tau"], [1, 3])
    for order in A.ORDERS:
        out["evaluate", order] = (plan.evaluate_band(sub, None, want=("act",), **flags(order)),
                                  plan.evaluate(sub, None, want=("act",), **flags(order)))
    tot = (bsol.actinic_flux(), bsol.flux_act_up(), bsol.flux_act_down())
    plan.close()
    return out, tot


@pytest.mark.parametrize("NQuad", [8, 32])
@pytest.mark.parametrize("work_columns", [0, 4])
def test_band_reduction_is_the_correctly_rounded_weighted_sum(NQuad, work_columns):
    import test_gpu_band as B
    res, (tot, up, (dd, dr)) = _band_reduced_and_full(NQuad, work_columns)
    worst = 0.0
    for key, (red, full) in res.items():
        nlev = B.L + 1 if key == "fetch" else 2
        for k in KEYS:
            assert red[k].shape == (B.P, B.K, nlev) and full[k].shape == (B.P * B.G, nlev)
            assert np.all(np.isfinite(full[k])) and np.max(np.abs(full[k])) > 0, (key, k)
            worst = max(worst, B.hold_reduced(red[k], full[k], B.WEIGHTS))
    assert tot.shape == (B.P, B.K, B.L + 1) and np.array_equal(tot, up + dd + dr)
    print(f"ACTINIC REDUCE NQuad {NQuad} work_columns {work_columns}: worst {worst:.3f} ulp of the exact weighted sum")


@pytest.mark.parametrize("NQuad", [8, 32])
def test_band_reduced_bits_do_not_depend_on_the_window(NQuad):
    a, b = _band_reduced_and_full(NQuad, 0)[0], _band_reduced_and_full(NQuad, 4)[0]
    for key in a:
        for k in KEYS:
            assert np.array_equal(a[key][0][k], b[key][0][k]), (key, k)


def test_streamed_band_agrees_with_the_evaluators():
    import pydisort_amd
    import test_gpu_band as B
    kw = B.band(8)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=B.WEIGHTS)
    ref = bsol.plan.evaluate_band(levels(bsol.plan.prep["tau"]), None, want=("flux", "act"))
    bsol.plan.close()
    out = pydisort_amd.solve_band_streamed(**kw, weights=B.WEIGHTS, chunk_columns=4, only_flux=True, actinic=True)
    plain = pydisort_amd.solve_band_streamed(**kw, weights=B.WEIGHTS, chunk_columns=4, only_flux=True)
    assert not any(k in plain for k in KEYS) and np.array_equal(plain["flux_up"], out["flux_up"])
    for k in KEYS:
        assert out[k].shape == (B.P, B.K, B.L + 1)
        assert np.max(np.abs(out[k] - ref[k])) <= TOL * np.max(np.abs(ref[k])), k  # (windows of 4, the fused evaluation: other kernels)
    one = pydisort_amd.solve_band_streamed(**kw, weights=B.WEIGHTS[1], levels=[0, B.L], only_flux=True, actinic=True)
    assert one[KEYS[0]].shape == (B.P, 2)


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
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=B.WEIGHTS, numeric_errors="nan")
    lev = levels(bsol.plan.prep["tau"])
    red = bsol.plan.evaluate_band(lev, None, want=("act",))
    full = bsol.plan.evaluate(lev, None, want=("act",))
    for k in KEYS:
        assert np.all(np.isnan(red[k][1])) and np.all(np.isnan(full[k][B.G:2 * B.G])), k
        assert np.all(np.isfinite(red[k][[0, 2]])), k
        B.hold_reduced(red[k], full[k], B.WEIGHTS, profiles=(0, 2))  # (the exact weighted sums of their own unreduced columns)
    assert np.all(np.isnan(bsol.actinic_flux()[1])) and np.all(np.isfinite(bsol.actinic_flux()[[0, 2]]))
    _, raising = pydisort_amd.pydisort_band(**kw, weights=B.WEIGHTS)
    with pytest.raises(pydisort_amd._lib.NumericalError):
        raising.actinic_flux()
    for s in (bsol, raising):
        s.plan.close()


# ---- 6. states ------------------------------------------------------------------------------------------------------------------------
def test_states_and_lazily_grown_buffers():
    import pydisort_amd
    cfg = batch(6)
    tau = points(cfg["tau_arr"])
    # (device_bytes counts the blocks as the library's pool of closed plans' memory hands them out, which may be larger than asked
    #  for: the pool is emptied before each of the two plans, so that both are carved from fresh blocks of the sizes they ask for)
    pydisort_amd.pool_trim()
    _, sol = pydisort_amd.pydisort_batch(**cfg, _defer_solve=True)
    with pytest.raises(RuntimeError, match="nothing to fetch"):
        sol.plan.fetch_actinic()
    sol.plan.solve()
    with pytest.raises(RuntimeError, match="nothing to fetch"):
        sol.plan.fetch_actinic()
    with pytest.raises(ValueError, match="set_band_weights"):
        sol.plan.fetch_band_actinic()
    with pytest.raises(ValueError):
        sol.flux_act_up(tau, True, is_derivative_wrt_tau=True)
    with pytest.raises(ValueError):
        sol.flux_act_down(tau, True, is_derivative_wrt_tau=True)
    with pytest.raises(ValueError):
        sol.plan.evaluate(tau, None, True, want=("act",), derivative=True)
    sol.flux_up(tau)
    pydisort_amd.pool_trim()
    _, twin = pydisort_amd.pydisort_batch(**cfg, _defer_solve=True)
    twin.plan.solve()
    twin.flux_up(tau)
    before = twin.plan.device_bytes()
    assert sol.plan.device_bytes() == before  # solved and evaluated without "act": nothing more is held
    sol.flux_act_up(tau)
    assert sol.plan.device_bytes() > before and twin.plan.device_bytes() == before
    sol.plan.set_eval_points(tau, np.array([0.0]))  # new points: the buffers hold no evaluation at them
    with pytest.raises(RuntimeError, match="nothing to fetch"):
        sol.plan.fetch_actinic()
    sol.plan.close()
    twin.plan.close()


def test_fetch_actinic_sizes_its_arrays_from_the_plans_own_points():
    """evaluate() without "act" moves the plan's points; a fetch_actinic() behind it returns arrays of THAT evaluation's ntau (not
    of the points stored earlier, and not of none), with the bits that want=("act",) gives at the same points -- after no stored
    points at all (pydisort_batch, flux_up) and after stored points of another count (set_eval_points(4), run()).  A caller's
    array of another shape, dtype or layout is refused before the library writes into it."""
    import pydisort_amd
    cfg = batch(6)
    tau = points(cfg["tau_arr"])  # 6 points
    lev = levels(cfg["tau_arr"])  # 4 points
    _, sol = pydisort_amd.pydisort_batch(**cfg)
    plan = sol.plan
    want = {k: v.copy() for k, v in plan.evaluate(tau, None, want=("act",)).items() if k in KEYS}
    want_d = {k: v.copy() for k, v in plan.evaluate(lev, None, want=("act",), derivative=True).items() if k in KEYS}
    _, fresh = pydisort_amd.pydisort_batch(**cfg)
    fresh.flux_up(tau)  # (no evaluation points were ever stored on this plan)
    got = fresh.plan.fetch_actinic()
    assert all(got[k].shape == (C, tau.shape[1]) and np.array_equal(got[k], want[k]) for k in KEYS)
    fresh.plan.close()
    plan.set_eval_points(lev, np.array([0.0]))
    plan.run()
    assert all(v.shape == (C, lev.shape[1]) for v in plan.fetch_actinic().values())
    plan.evaluate(tau, None, want=("u0",))  # 4 stored points, 6 evaluated
    got = plan.fetch_actinic()
    assert all(got[k].shape == (C, tau.shape[1]) and np.array_equal(got[k], want[k]) for k in KEYS)
    plan.evaluate(lev, None, want=("flux",), derivative=True)  # and back to fewer, in another order
    got = plan.fetch_actinic()
    assert all(got[k].shape == (C, lev.shape[1]) and np.array_equal(got[k], want_d[k]) for k in KEYS)
    # a caller's arrays: filled in place when they fit, refused when they do not
    mine = {KEYS[1]: np.full((C, lev.shape[1]), -7.0)}
    got = plan.fetch_actinic(mine)
    assert got[KEYS[1]] is mine[KEYS[1]] and np.array_equal(mine[KEYS[1]], want_d[KEYS[1]]) and np.array_equal(got[KEYS[0]], want_d[KEYS[0]])
    for bad in (np.zeros((C, tau.shape[1])), np.zeros((C, 0)), np.zeros((C, lev.shape[1]), np.float32),
                np.zeros((lev.shape[1], C)).T, np.zeros(C * lev.shape[1])):
        with pytest.raises(ValueError, match="out\\["):
            plan.fetch_actinic({KEYS[0]: bad})
    plan.close()
