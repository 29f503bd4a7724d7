"""Lambertian albedo sweeps on the device: ``pydisort_batch(..., lambert_sweep=True)``, ``pydisort_band(..., lambert_sweep=True)``,
``Plan.couple_lambert`` / ``couple_lambert_band`` (include/rtd.h: rtd_plan_couple_lambert, rtd_plan_couple_lambert_band,
rtd_lambert_kappa; kernels csrc/rtd_lambert.hip, arithmetic and rounding bound csrc/rtd_lambert.h).

Shapes: 6 columns x 3 layers at 6, 16 and 34 streams, and 6 columns x 1 layer at 6 streams; four depths per column including 0 and
the bottom; two azimuths; the albedos (0, 0.3, 0.95, 1), shared and per column; column 2 of every three-layer batch is the thick
near-conservative one (tau = 2, 12, 30; omega = 0.9999, 0.99999, 0.9999; g = 0.7), where 1 / (1 - s) = 7.6.  Bounds:

1. coupling: every coupled element against the EXACT rational coupling (fractions.Fraction) of the two plans' own fetched arrays and
   the host-held terms, within the bound derived in csrc/rtd_lambert.h -- 8 u (|a| + |kappa b|), kappa within 6 u; nothing measured;
2. the primary of a sweep has the bits of the same call without the keyword, and holds nothing more on the device;
3. end to end against the existing direct path (``surface=dict(model="lambert", params=A)``, with BTEMP and Kirchhoff's emissivity
   for the emitting case) and against the reference fixtures of tests/golden/lambert/: the project's 1e-9 of the field scale times
   the formula's own amplification 1 / (1 - A s); the measured distances are printed and recorded, the bound is not tightened to them;
4. identical bits: one window against windows of 4, a shared albedo list against the same list per column, one scratch chunk against
   several, the band entry against the batch entry fed with band_mix's arrays;
5. band: reduced coupled arrays against exact rational weighted sums of the unreduced coupled arrays, the house bound 1 ulp + 2^-90
   sum |w x|; a spectral albedo; a profile with a failed column is NaN, the others are kept;
6. byproducts: the spherical albedo and the upward total transmittance.

Figures seen on an MI355X (each test prints its own): coupled elements at worst 0.41 of the header's bound and kappa 0.41 of its own
(34 streams; 0.26 ... 0.31 at 6 and 16), kappa bit-identical to the host routine everywhere; against the direct path at worst 1.8e-14
x 1 / (1 - A s) of the field scale for values, derivatives and views (u0 at 34 streams) and 2.5e-11 for an antiderivative (flux_up,
6 streams x 3 layers: the thick column, whose antiderivative divides by a diffusion eigenvalue of 0.003); against the reference
fixtures 1.0e-14 (q6_l1) ... 1.6e-13 (16 streams), 1.0e-11 (q34_l3) and 1.7e-10 (q16_thick, its antiderivative fluxes), of the 1e-9
allowed; one window and windows of 4 held identical uncoupled arrays for 6 of 6 fields and so identical coupled bits; band
reduction of coupled arrays 0.500 ulp of the exact weighted sum, shared and spectral albedo alike."""
import functools
from math import pi

import numpy as np
import pytest

import lambert_cases as LC

pytestmark = pytest.mark.gpu

C = 6
ALB = np.array(LC.ALBEDOS)
PHI = np.array([0.0, 2.0])
MU = np.array([0.83, -0.41, -0.9])
ORDERS = (dict(), dict(is_antiderivative_wrt_tau=True), dict(is_derivative_wrt_tau=True))
SHAPES = [(6, 3), (6, 1), (16, 3), (34, 3)]


@functools.lru_cache(maxsize=None)
def columns(NQuad, L, thermal=False):
    """The batch of every test (built once per shape and left unchanged): keyword arguments of pydisort_batch over a black surface."""
    rng = np.random.default_rng(1000 + 10 * NQuad + L)
    nall = NQuad + 8
    g = rng.uniform(0.5, 0.85, (C, L, 1))
    kw = dict(tau_arr=np.cumsum(rng.uniform(0.1, 0.9, (C, L)), axis=1), omega_arr=rng.uniform(0.5, 0.99, (C, L)), NQuad=NQuad,
              Leg_coeffs_all=g ** np.arange(nall)[None, None, :], mu0=rng.uniform(0.3, 0.9, C), I0=rng.uniform(0.5, 3.0, C),
              phi0=rng.uniform(0.0, 2 * pi, C), b_neg=0.2)
    if L == 3:  # the amplified column
        kw["tau_arr"][2] = (2.0, 12.0, 30.0)
        kw["omega_arr"][2] = (0.9999, 0.99999, 0.9999)
        kw["Leg_coeffs_all"][2] = 0.7 ** np.arange(nall)[None, :]
    kw["f_arr"] = kw["Leg_coeffs_all"][:, :, NQuad].copy()
    if thermal:
        kw["thermal"] = dict(TEMPER=np.sort(rng.uniform(200.0, 300.0, (C, L + 1)), axis=1), WVNMLO=500.0, WVNMHI=900.0, TTEMP=60.0, TEMIS=0.8)
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return kw


def depths(kw):
    """[C, 4]: the top, an interior point, an interface (mid-layer of a one-layer column), the bottom."""
    t = kw["tau_arr"]
    return np.stack((np.zeros(C), 0.37 * t[:, -1], t[:, 0] if t.shape[1] > 1 else 0.5 * t[:, 0], t[:, -1]), axis=1)


def per_column_albedo():
    return np.ascontiguousarray(ALB[None, :] * np.linspace(0.4, 1.0, C)[:, None])


def hold_coupled(got, X, Y, alb, t, E):
    """got [C, A, ...] against the exact rational coupling of X [C, ...] and Y [C, ...] (Y without the azimuth axis when X has it);
    returns the worst error over the header's bound."""
    alb = np.broadcast_to(alb, (C, alb.shape[-1]))
    if Y.ndim < X.ndim:
        Y = Y[..., None]
    worst = 0.0
    for c in range(C):
        for a in range(alb.shape[1]):
            args = (alb[c, a], t["flux_down_bottom"][c], t["spherical_albedo"][c], 0.0 if E is None else np.broadcast_to(E, (C,))[c])
            r = LC.couple_ratio(got[c, a], X[c], Y[c], *args)
            assert r <= 1.0, (c, a, r)
            worst = max(worst, r)
            if LC.kappa_exact(*args)[0] == 0:
                assert np.array_equal(got[c, a], X[c])  # A = 0 without emission: the primary's array, bit for bit
    return worst


def hold_kappa(kappa, alb, t, E):
    alb = np.broadcast_to(alb, (C, alb.shape[-1]))
    worst, same = 0.0, True
    for c in range(C):
        for a in range(alb.shape[1]):
            args = (alb[c, a], t["flux_down_bottom"][c], t["spherical_albedo"][c], 0.0 if E is None else np.broadcast_to(E, (C,))[c])
            r = LC.kappa_ratio(kappa[c, a], *args)
            assert r <= 1.0, (c, a, r)
            worst, same = max(worst, r), same and kappa[c, a] == LC.kappa_model(*args)[0]
    return worst, same


# ---- 1. coupling against exact arithmetic -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("NT_cor", [True, False])
@pytest.mark.parametrize("NQuad,L", SHAPES)
def test_coupled_arrays_are_the_exact_coupling_of_the_two_plans_own_arrays(NQuad, L, NT_cor):
    import pydisort_amd
    kw = columns(NQuad, L)
    tau = depths(kw)
    forms = [dict()] + ([dict(work_columns=4, retain="full")] + ([dict(work_columns=4, retain="lean")] if NQuad >= 10 else []) if L == 3 else [])
    worst = worst_k = 0.0
    bits = True
    for i, form in enumerate(forms):
        _, sol = pydisort_amd.pydisort_batch(**kw, NT_cor=NT_cor, device_prepare=True, lambert_sweep=True, **form)
        below, t = sol.lit_from_below, sol.lambert_terms()
        assert sol.plan.windows()[1] == (2 if form else 1) and below.plan.windows() == sol.plan.windows()
        assert sol.plan.retained_form() == form.get("retain", "full") == below.plan.retained_form()
        assert np.all(np.isfinite(t["flux_down_bottom"])) and np.all((t["spherical_albedo"] > 0) & (t["spherical_albedo"] < 1))
        alb, E = (ALB, None) if i % 2 == 0 else (per_column_albedo(), np.linspace(0.0, 1.7, C))
        sw = sol.lambert(alb, emission=E)
        k, same = hold_kappa(sw.kappa, alb, t, E)
        worst_k, bits = max(worst_k, k), bits and same
        assert not np.any(sw.kappa_flag)
        for order in (ORDERS if i == 0 else ORDERS[i % 3:][:1]):  # every tau-order on the one-window plan, one each on the others
            fd, fdb = sol.flux_down(tau, **order), below.flux_down(tau, **order)
            got_fd = sw.flux_down(tau, **order)
            pairs = [(sw.u(tau, PHI, **order), sol.u(tau, PHI, **order), below.u0(tau, **order)),
                     (sw.u0(tau, **order), sol.u0(tau, **order), below.u0(tau, **order)),
                     (sw.flux_up(tau, **order), sol.flux_up(tau, **order), below.flux_up(tau, **order)),
                     (got_fd[0], fd[0], fdb[0]),
                     (sw.u0_at(MU, tau, **order), sol.u0_at(MU, tau, **order), below.u0_at(MU, tau, **order))]
            for mode in ("interpolated", "at_angles"):
                pairs.append((sw.u_at(MU, tau, PHI, corrections=mode, **order), sol.u_at(MU, tau, PHI, corrections=mode, **order),
                              below.u0_at(MU, tau, **order)))
            assert pairs[0][0].shape == (C, alb.shape[-1], NQuad, 4, 2) and pairs[-1][0].shape == (C, alb.shape[-1], 3, 4, 2)
            assert np.array_equal(got_fd[1], np.broadcast_to(fd[1][:, None, :], got_fd[1].shape))  # the direct flux: the primary's
            for got, X, Y in pairs:
                assert np.all(np.isfinite(got)) and np.max(np.abs(X)) > 0 and np.max(np.abs(Y)) > 0
                worst = max(worst, hold_coupled(got, X, Y, alb, t, E))
        if i == 0:  # through run: the stored points of both plans, then the plan-level call
            for plan, phi in ((sol.plan, PHI), (below.plan, np.zeros(1))):
                plan.set_eval_points(tau, phi)
                plan.run()
            X, Y = sol.plan.fetch(), below.plan.fetch()
            out = sol.plan.couple_lambert(below.plan, alb, t["flux_down_bottom"], t["spherical_albedo"], E)
            for key in ("u", "u0", "flux_up", "flux_down_diffuse"):
                worst = max(worst, hold_coupled(out[key], X[key], Y["u0" if key == "u" else key], alb, t, E))
        sol.plan.close()
        below.plan.close()
    print(f"LAMBERT coupling NQuad {NQuad} L {L} NT {NT_cor}: elements worst {worst:.3f} of the header's bound, kappa worst {worst_k:.3f} "
          f"of its bound, kappa {'bit-identical to' if bits else 'NOT bit-identical to'} the host routine")


# ---- 2. the primary is unchanged ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NQuad,L", [(16, 3), (6, 1)])
def test_the_primary_keeps_its_bits_and_holds_nothing_more(NQuad, L):
    import pydisort_amd
    kw = columns(NQuad, L)
    tau = depths(kw)
    _, plain = pydisort_amd.pydisort_batch(**kw, NT_cor=True, device_prepare=True)
    _, sol = pydisort_amd.pydisort_batch(**kw, NT_cor=True, device_prepare=True, lambert_sweep=True)

    def fields(s):
        fd = s.flux_down(tau)
        return dict(u=s.u(tau, PHI), u0=s.u0(tau), flux_up=s.flux_up(tau), flux_down_diffuse=fd[0], flux_down_direct=fd[1])
    want, got = fields(plain), fields(sol)
    for k in want:
        assert np.all(np.isfinite(want[k])) and np.array_equal(got[k], want[k]), k
    below = sol.lit_from_below
    below.u0(tau)  # (the companion's evaluation buffers at these points: grown by its own evaluator)
    held = sol.plan.device_bytes(), below.plan.device_bytes(), plain.plan.device_bytes()
    sw = sol.lambert(ALB, emission=0.4)
    sw.u(tau, PHI), sw.u0(tau), sw.flux_down(tau), sw.flux_up(tau, is_derivative_wrt_tau=True)
    assert (sol.plan.device_bytes(), below.plan.device_bytes(), plain.plan.device_bytes()) == held  # nothing of the sweep stays with a plan
    got = fields(sol)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# ---- 3. end to end against the direct path and the reference -------------------------------------------------------------------------
@pytest.mark.parametrize("NQuad,L,thermal", [(6, 3, False), (6, 1, False), (16, 3, False), (16, 3, True), (34, 3, False)])
def test_sweep_matches_the_direct_lambert_solves(NQuad, L, thermal):
    import pydisort_amd
    kw = columns(NQuad, L, thermal)
    tau = depths(kw)
    BTEMP = np.linspace(280.0, 310.0, C) if thermal else None
    _, sol = pydisort_amd.pydisort_batch(**kw, NT_cor=not thermal, lambert_sweep=True)
    s = sol.lambert_terms()["spherical_albedo"]
    sw = sol.lambert(ALB, BTEMP=BTEMP)
    fd = sw.flux_down(tau)
    got = dict(u=sw.u(tau, PHI), u0=sw.u0(tau), flux_up=sw.flux_up(tau), flux_down_diffuse=fd[0], flux_down_direct=fd[1],
               u_mu=sw.u_at(MU, tau, PHI), d_u0=sw.u0(tau, is_derivative_wrt_tau=True), a_flux_up=sw.flux_up(tau, True))
    worst = dict.fromkeys(got, 0.0)
    for a, A in enumerate(ALB):
        th = dict(kw["thermal"], BTEMP=BTEMP) if thermal else None  # (emissivity None: Kirchhoff's law on the device-formed mode)
        base = {k: v for k, v in kw.items() if k != "thermal"}
        _, ref = pydisort_amd.pydisort_batch(**base, NT_cor=not thermal, surface=dict(model="lambert", params=A), NBDRF=1, thermal=th)
        rfd = ref.flux_down(tau)
        want = dict(u=ref.u(tau, PHI), u0=ref.u0(tau), flux_up=ref.flux_up(tau), flux_down_diffuse=rfd[0], flux_down_direct=rfd[1],
                    u_mu=ref.u_at(MU, tau, PHI), d_u0=ref.u0(tau, is_derivative_wrt_tau=True), a_flux_up=ref.flux_up(tau, True))
        for k in want:
            for c in range(C):
                d = float(np.max(np.abs(got[k][c, a] - want[k][c])) / np.max(np.abs(want[k][c])))
                allowed = 1e-9 / (1.0 - A * s[c])
                worst[k] = max(worst[k], d / allowed)
                assert d <= allowed, (k, c, A, d, allowed)
        ref.plan.close()
    for k, v in worst.items():
        print(f"LAMBERT direct NQuad {NQuad} L {L} thermal {thermal} {k}: worst {v * 1e-9:.2e} x 1 / (1 - A s) of the field scale, of 1e-9 allowed")


@pytest.mark.parametrize("name", sorted(LC.cases()))
def test_sweep_matches_the_reference_fixtures(name):
    import pydisort_amd
    kw, E = LC.cases()[name]
    store = LC.load(name)
    tau, mu = store["tau"][None, :], store["mu"]
    batch = dict(tau_arr=kw["tau_arr"][None], omega_arr=kw["omega_arr"][None], NQuad=kw["NQuad"], Leg_coeffs_all=kw["Leg_coeffs_all"][None],
                 mu0=[kw["mu0"]], I0=[kw["I0"]], phi0=[kw["phi0"]], NLeg=kw.get("NLeg"), b_neg=kw.get("b_neg", 0), NT_cor=kw.get("NT_cor", False),
                 f_arr=kw.get("f_arr", 0), s_poly_coeffs=None if "s_poly_coeffs" not in kw else kw["s_poly_coeffs"][None])
    _, sol = pydisort_amd.pydisort_batch(**batch, lambert_sweep=True)
    s = sol.lambert_terms()["spherical_albedo"][0]
    F_ref, s_ref = LC.terms(store)
    assert abs(s - s_ref) <= 1e-9 and abs(sol.lambert_terms()["flux_down_bottom"][0] - F_ref) <= 1e-9 * abs(F_ref)
    sw = sol.lambert(ALB, emission=E)
    worst = 0.0
    for order in LC.orders_of(name):
        flag = order == "antider"
        fd = sw.flux_down(tau, flag)
        got = dict(flux_up=sw.flux_up(tau, flag), flux_down_diffuse=fd[0])
        if not flag:
            got.update(u=sw.u(tau, LC.PHI), u0=sw.u0(tau), u_mu=sw.u_at(mu, tau, LC.PHI), u0_mu=sw.u0_at(mu, tau))
        for field in LC.fields_of(order):
            for i, A in enumerate(LC.ALBEDOS):
                want = LC.get(store, f"direct{i}", order, field)
                d = float(np.max(np.abs(got[field][0, i] - want)) / np.max(np.abs(want)))
                allowed = 1e-9 / (1.0 - A * s)
                worst = max(worst, d / allowed)
                assert d <= allowed, (order, field, A, d, allowed)
    print(f"LAMBERT reference {name}: worst {worst * 1e-9:.2e} x 1 / (1 - A s) of the field scale, of 1e-9 allowed")


# ---- 4. identical bits --------------------------------------------------------------------------------------------------------------
def _sweep_fields(sw, tau):
    fd = sw.flux_down(tau)
    return dict(u=sw.u(tau, PHI), u0=sw.u0(tau), flux_up=sw.flux_up(tau), flux_down_diffuse=fd[0], u_mu=sw.u_at(MU, tau, PHI),
                u0_mu=sw.u0_at(MU, tau))


def test_bits_do_not_depend_on_windows_chunks_or_how_the_albedos_are_given(monkeypatch):
    import pydisort_amd
    kw = columns(16, 3)
    tau = depths(kw)
    _, one = pydisort_amd.pydisort_batch(**kw, NT_cor=True, device_prepare=True, lambert_sweep=True)
    _, win = pydisort_amd.pydisort_batch(**kw, NT_cor=True, device_prepare=True, lambert_sweep=True, work_columns=4)
    assert one.plan.windows()[1] == 1 and win.plan.windows() == (4, 2) and win.lit_from_below.plan.windows() == (4, 2)
    E = np.linspace(0.0, 1.7, C)
    want, windowed = _sweep_fields(one.lambert(ALB, emission=E), tau), _sweep_fields(win.lambert(ALB, emission=E), tau)

    def own(sol):  # what the coupling reads of a pair of plans, per coupled field
        fd, b = sol.flux_down(tau), sol.lit_from_below
        return dict(u=(sol.u(tau, PHI), b.u0(tau)), u0=(sol.u0(tau), b.u0(tau)), flux_up=(sol.flux_up(tau), b.flux_up(tau)),
                    flux_down_diffuse=(fd[0], b.flux_down(tau)[0]), u_mu=(sol.u_at(MU, tau, PHI), b.u0_at(MU, tau)),
                    u0_mu=(sol.u0_at(MU, tau), b.u0_at(MU, tau)))
    own_one, own_win = own(one), own(win)
    same_terms = all(np.array_equal(one.lambert_terms()[k], win.lambert_terms()[k]) for k in ("flux_down_bottom", "spherical_albedo"))
    same = 0
    for k in want:  # identical uncoupled arrays and terms -> identical coupled bits, whatever the windows
        if same_terms and all(np.array_equal(x, y) for x, y in zip(own_one[k], own_win[k])):
            assert np.array_equal(windowed[k], want[k]), k
            same += 1
        else:
            assert np.max(np.abs(windowed[k] - want[k])) <= 1e-9 * np.max(np.abs(want[k])), k
    print(f"LAMBERT bits: {same} of {len(want)} coupled fields read identical uncoupled arrays from one window and from windows of 4")
    rep = _sweep_fields(one.lambert(np.tile(ALB, (C, 1)), emission=E), tau)  # the same list repeated per column
    for k in want:
        assert np.array_equal(rep[k], want[k]), k
    monkeypatch.setenv("RTD_LAMBERT_BYTES", str(8 * 4 * 16 * 4 * 2 * 2))  # two columns of u per chunk: three chunks
    few = _sweep_fields(one.lambert(ALB, emission=E), tau)
    monkeypatch.setenv("RTD_LAMBERT_BYTES", "8")  # one column per chunk
    single = _sweep_fields(one.lambert(ALB, emission=E), tau)
    monkeypatch.delenv("RTD_LAMBERT_BYTES")
    for k in want:
        assert np.array_equal(few[k], want[k]) and np.array_equal(single[k], want[k]), k


def _band_kw(NQuad):
    from test_gpu_band import band
    return dict(band(NQuad), b_pos=0)


@pytest.mark.parametrize("NQuad", [8, 16, 32])
def test_band_entry_gives_the_bits_of_the_batch_entry(NQuad):
    import pydisort_amd
    from test_gpu_band import G, L, P, WEIGHTS
    kw = _band_kw(NQuad)
    tau, om, f, leg = pydisort_amd.band_mix(kw["dtau_abs"], kw["dtau_spec"], kw["omega_spec"], kw["Leg_spec"], NQuad, delta_M=True)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS, lambert_sweep=True)
    rep = lambda a: np.repeat(a, G, axis=0)  # noqa: E731
    _, sol = pydisort_amd.pydisort_batch(tau, om, NQuad, leg, rep(kw["mu0"]), kw["I0"].reshape(-1), rep(kw["phi0"]), f_arr=f, b_neg=kw["b_neg"],
                                         device_prepare=True, lambert_sweep=True)
    for k, v in sol.lambert_terms().items():
        assert np.array_equal(bsol.lambert_terms()[k].reshape(-1), v), k
    levels = np.concatenate((np.zeros((P * G, 1)), tau), axis=1)
    alb = np.ascontiguousarray(ALB[None, :] * np.linspace(0.5, 1.0, P * G)[:, None])
    want = sol.lambert(alb, emission=0.3)
    got = bsol.columns.lambert(alb, emission=0.3)  # the band's own two plans, column by column
    assert np.array_equal(got.kappa, want.kappa)
    for name, args in (("u", (levels, PHI)), ("u0", (levels,)), ("flux_up", (levels,)), ("u_at", (MU, levels, PHI)), ("u0_at", (MU, levels))):
        a, b = getattr(got, name)(*args), getattr(want, name)(*args)
        assert np.all(np.isfinite(b)) and np.array_equal(a, b), name
    assert L == 3


# ---- 5. the band --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spectral", [False, True])
def test_band_reduction_of_coupled_arrays_is_the_correctly_rounded_weighted_sum(spectral):
    import pydisort_amd
    from test_gpu_band import G, L, P, WEIGHTS, hold_reduced
    NQuad = 16
    _, bsol = pydisort_amd.pydisort_band(**_band_kw(NQuad), weights=WEIGHTS, lambert_sweep=True)
    alb = np.ascontiguousarray(ALB[None, None, :] * np.linspace(0.4, 1.0, P * G).reshape(P, G, 1)) if spectral else np.ascontiguousarray(
        ALB[None, :] * np.array([1.0, 0.8, 0.6])[:, None])
    E = np.linspace(0.0, 1.2, P * G)
    red = bsol.lambert(alb, emission=E)
    per_column = alb.reshape(P * G, -1) if spectral else np.repeat(alb, G, axis=0)
    full = bsol.columns.lambert(per_column, emission=E)
    assert np.array_equal(red.kappa.reshape(P * G, -1), full.kappa)
    from pydisort_amd.band import level_tau
    lev = [0, 1, L]
    tau = level_tau(bsol.plan.prep["tau"], lev)
    worst = 0.0
    fdr, fdf = red.flux_down(lev), full.flux_down(tau)
    for r, x in ((red.u(lev, PHI), full.u(tau, PHI)), (red.u0(lev), full.u0(tau)), (red.flux_up(lev), full.flux_up(tau)), (fdr[0], fdf[0]),
                 (red.u_at(MU, lev, PHI), full.u_at(MU, tau, PHI)), (red.u0_at(MU, lev), full.u0_at(MU, tau))):
        assert r.shape == (P, WEIGHTS.shape[0]) + x.shape[1:] and np.all(np.isfinite(x)) and np.max(np.abs(x)) > 0
        worst = max(worst, hold_reduced(r, x, WEIGHTS))
    assert np.array_equal(fdr[1], np.broadcast_to(bsol.flux_down(lev)[1][:, :, None, :], fdr[1].shape))  # the direct flux: the primary's band result
    print(f"LAMBERT band {'spectral albedo' if spectral else 'albedo per profile'}: worst {worst:.3f} ulp of the exact weighted sum")


def test_a_bad_profile_is_nan_and_the_others_keep_their_results():
    """The input of tests/test_gpu_band.py: species 1 has a first moment of 2.5, the eigen stage of Fourier mode 0 fails wherever it
    dominates, and only profile 1 contains it."""
    import pydisort_amd
    from test_gpu_band import G, P, WEIGHTS, hold_reduced
    NQuad = 8
    kw = _band_kw(NQuad)
    leg = kw["Leg_spec"].copy()
    leg[1, 1:] = 0.0
    leg[1, 1] = 2.5
    ds, om = kw["dtau_spec"].copy(), kw["omega_spec"].copy()
    ds[:, :, 1] = 0.0
    ds[1, :, 1] = 5.0
    om[1, :, 1] = 0.97
    kw.update(Leg_spec=leg, dtau_spec=ds, omega_spec=om)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS, numeric_errors="nan", lambert_sweep=True)
    st = bsol.plan.column_status()
    assert np.all(st[G:2 * G] & 0xFF) and not np.any(st[:G]) and not np.any(st[2 * G:])
    red, full = bsol.lambert(ALB), bsol.columns.lambert(ALB)
    from pydisort_amd.band import level_tau
    tau = level_tau(bsol.plan.prep["tau"])
    for r, x in ((red.u(None, PHI), full.u(tau, PHI)), (red.u0(), full.u0(tau)), (red.flux_up(), full.flux_up(tau))):
        assert np.all(np.isnan(r[1])) and np.all(np.isfinite(r[[0, 2]]))
        assert np.all(np.isnan(x[G:2 * G])) and np.all(np.isfinite(x[:G])) and np.all(np.isfinite(x[2 * G:]))
        hold_reduced(r, x, WEIGHTS, profiles=(0, 2))
    _, raising = pydisort_amd.pydisort_band(**kw, weights=WEIGHTS, numeric_errors="nan", lambert_sweep=True)
    raising.plan.numeric_errors = raising.columns.lit_from_below.plan.numeric_errors = "raise"
    with pytest.raises(pydisort_amd._lib.NumericalError):
        raising.lambert(ALB).flux_up()
    assert P == 3


# ---- 6. byproducts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NQuad,L", [(16, 3), (6, 1)])
def test_the_byproducts_are_the_atmospheric_correction_terms(NQuad, L):
    import pydisort_amd
    kw = columns(NQuad, L)
    _, sol = pydisort_amd.pydisort_batch(**kw, device_prepare=True, lambert_sweep=True)
    below, t = sol.lit_from_below, sol.lambert_terms()
    bottom = kw["tau_arr"][:, -1:]
    d = below.flux_down(bottom)
    assert np.array_equal(t["spherical_albedo"], (d[0][:, 0] + d[1][:, 0]) / np.pi) and np.all(d[1] == 0)
    fd = sol.flux_down(bottom)
    assert np.array_equal(t["flux_down_bottom"], fd[0][:, 0] + fd[1][:, 0])
    nodes = sol.mu_arr[:NQuad // 2]
    top = below.u0(np.zeros(1))
    trans = below.u0_at(nodes[[0, -1]], np.zeros(1))  # the upward total transmittance at two nodes: those rows of u0, bit for bit
    assert np.array_equal(trans[:, 0, 0], top[:, 0, 0]) and np.array_equal(trans[:, 1, 0], top[:, NQuad // 2 - 1, 0])
    assert np.all((top[:, :NQuad // 2, 0] > 0) & (top[:, :NQuad // 2, 0] < 1))  # a transmittance
    if L == 3:
        assert abs(t["spherical_albedo"][2] - 0.8687) < 2e-3  # the thick column: s = 0.869, 1 / (1 - s) = 7.6
