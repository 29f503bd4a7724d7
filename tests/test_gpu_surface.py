"""Parametric surface models on the device: ``surface=`` of the batch, streamed and band entry points, ``surface_reflectance``,
``Plan.get_bdrf`` (include/rtd.h: rtd_plan_request_surface, rtd_surface_samples, rtd_plan_get_bdrf).

* the samples of rtd_surface_samples_kernel against the 50-digit truth of tests/golden/surface (tools/surface_truth.py) at
  16 x np_dist_all[0] of the row's max |rho| -- the bound of tests/test_surface_cpu.py, whose docstring derives it;
* everything else is BIT identity: the request forms the tables the older paths form from the same numbers -- the samples of
  ``surface_reflectance`` through ``bdrf_samples``, an albedo through ``bdrf_q``, the tables of ``get_bdrf`` under Kirchhoff's law
  -- whatever the chunk size, the window size, shared or repeated parameters, the batch or the band entry;
* DISORT's Hapke problems 6d ... 6h through ``surface=``: the fluxes against the reference's goldens at the 1e-5 of
  test_device_bdrf_fourier_integration_hapke.

Shapes: 6 columns x 3 layers at 6 / 16 / 34 streams (N = 3, 8, 17: below, at and above a power of two of the padded tables), per-column
parameters and mu0, nphi = 24 / 44 / 80 (no multiple of the wavefront; 2 (NBDRF - 1) < nphi holds with NBDRF = NQuad)."""
import functools
import glob
import os
from math import pi

import numpy as np
import pytest

import goldens

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "surface", "*.npz")))
C, L = 6, 3
PHI = np.array([0.0, 2.0])
NAMES = {1: "hapke", 2: "rossli", 3: "rpv"}


@functools.lru_cache(maxsize=None)
def columns(NQuad, beam=True):
    """The batch of every test (built once per shape and left unchanged): keyword arguments of pydisort_batch."""
    rng = np.random.default_rng(300 + NQuad)
    leg = rng.uniform(0.3, 0.8, (C, L, 1)) ** np.arange(NQuad + 3)[None, None, :]
    kw = dict(tau_arr=np.cumsum(rng.uniform(0.1, 1.0, (C, L)), axis=1), omega_arr=rng.uniform(0.2, 0.95, (C, L)), NQuad=NQuad,
              Leg_coeffs_all=leg, mu0=rng.uniform(0.25, 0.95, C), I0=rng.uniform(0.5, 2.0, C) if beam else np.zeros(C),
              phi0=rng.uniform(0.0, 2 * pi, C), f_arr=leg[:, :, NQuad].copy(), b_neg=rng.uniform(0.0, 0.2, C))
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return kw


@functools.lru_cache(maxsize=None)
def parameters(model):
    rng = np.random.default_rng(7)
    if model == "hapke":
        p = np.stack((rng.uniform(0.2, 1.2, C), rng.uniform(0.04, 0.3, C), rng.uniform(0.3, 0.99, C)), axis=1)
    elif model == "rossli":
        p = np.stack((rng.uniform(0.05, 0.4, C), rng.uniform(0.0, 0.3, C), rng.uniform(0.0, 0.08, C)), axis=1)
    elif model == "rpv":
        p = np.stack((rng.uniform(0.05, 0.4, C), rng.uniform(0.6, 1.3, C), rng.uniform(-0.4, 0.3, C), rng.uniform(0.0, 1.0, C)), axis=1)
    else:
        p = rng.uniform(0.05, 0.9, (C, 1))
    p.setflags(write=False)
    return p


def fields(sol, tau):
    fd = sol.flux_down(tau)
    return dict(u=sol.u(tau, PHI), u0=sol.u0(tau), flux_up=sol.flux_up(tau), flux_down_diffuse=fd[0], flux_down_direct=fd[1])


def levels(kw):
    return np.concatenate((np.zeros((kw["tau_arr"].shape[0], 1)), kw["tau_arr"]), axis=1)


def same_bits(got, want, what=""):
    for k in want:
        assert np.all(np.isfinite(want[k])) and np.max(np.abs(want[k])) > 0, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, float(np.max(np.abs(got[k] - want[k]))))


def same_tables(plan_a, plan_b, what=""):
    qa, q0a = plan_a.get_bdrf()
    qb, q0b = plan_b.get_bdrf()
    assert np.all(np.isfinite(qa)) and np.max(np.abs(qa)) > 0
    assert np.array_equal(qa, qb) and np.array_equal(q0a, q0b), (what, float(np.max(np.abs(qa - qb))), float(np.max(np.abs(q0a - q0b))))
    return qa, q0a


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_device_samples_against_truth(path):
    import pydisort_amd
    d = np.load(path)
    tol = 16.0 * float(d["np_dist_all"][0])
    assert 1e-16 < tol < 1e-12
    npar = {1: 3, 2: 3, 3: 4}[int(d["model"])]
    got = pydisort_amd.surface_reflectance(NAMES[int(d["model"])], d["params"][:npar], d["mu"][:, None], d["mup"][None, :], int(d["nphi"]))
    assert got.shape == d["rho"].shape
    err = np.abs(got - d["rho"]) / d["scale"][:, :, None]
    print(f"{os.path.basename(path)}: tolerance {tol:.3e} of the row's max |rho|; worst on the device {err.max():.3e}")
    assert err.max() <= tol
    if int(d["model"]) == 2:
        assert np.all(got >= 0.0)


@pytest.mark.parametrize("NQuad", [6, 16, 34])
@pytest.mark.parametrize("model", ["hapke", "rossli", "rpv"])
def test_request_gives_the_bits_of_the_sampled_path(monkeypatch, model, NQuad):
    import pydisort_amd
    kw, par, nphi, N = columns(NQuad), parameters(model), 2 * NQuad + 12, NQuad // 2
    monkeypatch.delenv("RTD_SURFACE_BYTES", raising=False)
    mu_arr, sol = pydisort_amd.pydisort_batch(**kw, surface=dict(model=model, params=par, nphi=nphi))
    mu = mu_arr[:N]
    rho_qq = pydisort_amd.surface_reflectance(model, par[:, None, None, :], mu[None, :, None], mu[None, None, :], nphi)
    rho_q0 = pydisort_amd.surface_reflectance(model, par[:, None, :], mu[None, :], kw["mu0"][:, None], nphi)
    assert rho_qq.shape == (C, N, N, nphi) and rho_q0.shape == (C, N, nphi)
    _, ref = pydisort_amd.pydisort_batch(**kw, device_prepare=True, bdrf_samples=(rho_qq, rho_q0))
    q, q0 = same_tables(sol.plan, ref.plan, "request against samples")
    assert q.shape == (C, NQuad, N, N) and q0.shape == (C, NQuad, N) and np.max(np.abs(q0)) > 0
    want = fields(ref, levels(kw))
    same_bits(fields(sol, levels(kw)), want, "request against samples")
    # one column per chunk (the samples of one column: (N N + N) nphi doubles)
    monkeypatch.setenv("RTD_SURFACE_BYTES", str((N * N + N) * nphi * 8))
    _, one = pydisort_amd.pydisort_batch(**kw, surface=dict(model=model, params=par, nphi=nphi))
    monkeypatch.delenv("RTD_SURFACE_BYTES")
    same_tables(one.plan, ref.plan, "one column per chunk")
    same_bits(fields(one, levels(kw)), want, "one column per chunk")
    # shared parameters against the same row repeated
    _, shared = pydisort_amd.pydisort_batch(**kw, surface=dict(model=model, params=par[2], nphi=nphi))
    _, repeated = pydisort_amd.pydisort_batch(**kw, surface=dict(model=model, params=np.tile(par[2], (C, 1)), nphi=nphi))
    same_tables(shared.plan, repeated.plan, "shared against repeated")
    same_bits(fields(shared, levels(kw)), fields(repeated, levels(kw)), "shared against repeated")
    assert not np.array_equal(shared.plan.get_bdrf()[0], q)


@pytest.mark.parametrize("NQuad", [6, 16, 34])
def test_lambert_gives_the_bits_of_an_albedo_table(NQuad):
    import pydisort_amd
    kw, alb, N = columns(NQuad), parameters("lambert"), NQuad // 2
    _, sol = pydisort_amd.pydisort_batch(**kw, surface=dict(model="lambert", params=alb[:, 0]), NBDRF=1)
    _, ref = pydisort_amd.pydisort_batch(**kw, device_prepare=True, bdrf_q=np.broadcast_to(alb[:, :, None, None], (C, 1, N, N)),
                                         bdrf_q0=np.broadcast_to(alb[:, :, None], (C, 1, N)))
    same_tables(sol.plan, ref.plan, "lambert")
    same_bits(fields(sol, levels(kw)), fields(ref, levels(kw)), "lambert")
    # more modes than one: the higher ones are zero
    _, more = pydisort_amd.pydisort_batch(**kw, surface=dict(model="lambert", params=alb), NBDRF=3)
    q, q0 = more.plan.get_bdrf()
    assert np.all(q[:, 0] == alb[:, :, None]) and np.all(q0[:, 0] == alb) and np.all(q[:, 1:] == 0) and np.all(q0[:, 1:] == 0)


@pytest.mark.parametrize("model", ["rossli", "lambert"])
def test_kirchhoff_emissivity_uses_the_device_formed_mode(model):
    import pydisort_amd
    NQuad = 16
    kw, par = columns(NQuad), parameters(model)
    rng = np.random.default_rng(5)
    th = dict(TEMPER=np.sort(rng.uniform(200.0, 300.0, (C, L + 1)), axis=1), WVNMLO=500.0, WVNMHI=900.0, BTEMP=rng.uniform(280.0, 310.0, C),
              TTEMP=60.0, TEMIS=0.8)
    _, sol = pydisort_amd.pydisort_batch(**kw, surface=dict(model=model, params=par, nphi=48), thermal=th)
    q, q0 = sol.plan.get_bdrf()
    _, ref = pydisort_amd.pydisort_batch(**kw, device_prepare=True, bdrf_q=q, bdrf_q0=q0, thermal=th)
    same_tables(sol.plan, ref.plan, "kirchhoff")
    same_bits(fields(sol, levels(kw)), fields(ref, levels(kw)), "kirchhoff")
    # the emissivity did come from the mode: a black surface emits more
    _, black = pydisort_amd.pydisort_batch(**kw, thermal=th)
    assert np.all(black.flux_up(levels(kw))[:, -1] != sol.flux_up(levels(kw))[:, -1])


@pytest.mark.parametrize("NQuad", [8, 16, 32])
def test_band_entry_gives_the_bits_of_the_batch_entry(NQuad):
    import pydisort_amd
    import test_gpu_band as tb
    kw = tb.band(NQuad)
    P, G = tb.P, tb.G
    par = parameters("rossli")[:P]
    nphi = 2 * NQuad + 8
    tau, om, f, leg = pydisort_amd.band_mix(kw["dtau_abs"], kw["dtau_spec"], kw["omega_spec"], kw["Leg_spec"], NQuad, delta_M=True)
    rep = lambda a: np.repeat(a, G, axis=0)  # noqa: E731
    _, sol = pydisort_amd.pydisort_batch(tau, om, NQuad, leg, rep(kw["mu0"]), kw["I0"].reshape(-1), rep(kw["phi0"]), f_arr=f,
                                         b_pos=rep(kw["b_pos"]), b_neg=kw["b_neg"], surface=dict(model="rossli", params=rep(par), nphi=nphi))
    lev = np.concatenate((np.zeros((P * G, 1)), tau), axis=1)
    want = fields(sol, lev)
    for params, what in ((par, "per profile"), (rep(par).reshape(P, G, 3), "per column")):
        _, bsol = pydisort_amd.pydisort_band(**kw, weights=tb.WEIGHTS, surface=dict(model="rossli", params=params, nphi=nphi))
        assert np.array_equal(bsol.tau_arr.reshape(P * G, L), tau)
        same_tables(bsol.plan, sol.plan, what)
        same_bits(fields(bsol.columns, lev), want, what)
    got = pydisort_amd.solve_band_streamed(**kw, weights=tb.WEIGHTS, phi=PHI, chunk_columns=4, surface=dict(model="rossli", params=par, nphi=nphi))
    q, q0 = sol.plan.get_bdrf()  # the streamed band form: the request against the same tables uploaded per column
    ref = pydisort_amd.solve_band_streamed(**kw, weights=tb.WEIGHTS, phi=PHI, chunk_columns=4, bdrf_q=q, bdrf_q0=q0)
    keys = ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct")
    same_bits({k: got[k] for k in keys}, {k: ref[k] for k in keys}, "streamed band")


@pytest.mark.parametrize("NQuad", [6, 16, 34])
def test_streamed_windows_give_the_bits_of_one_window(NQuad):
    """solve_columns_streamed in windows of 4 (4 + 2 columns) against the one-window plan of pydisort_batch, both driven through
    run_fetch at the interfaces: the streamed form evaluates there inside the boundary-condition kernel, the evaluators of a
    BatchSolution in the evaluation kernel, and those two routes differ in rounding (3e-15) with or without a surface."""
    import pydisort_amd
    kw, par = columns(NQuad), parameters("rpv")
    sf = dict(model="rpv", params=par, nphi=2 * NQuad + 12)
    _, sol = pydisort_amd.pydisort_batch(**kw, surface=sf, _defer_solve=True)
    assert sol.plan.windows()[1] == 1
    sol.plan.set_eval_points(levels(kw), PHI)
    want = sol.plan.run_fetch()
    got = pydisort_amd.solve_columns_streamed(dict(kw, surface=sf), levels(kw), PHI, chunk_columns=4)
    same_bits({k: got[k] for k in want}, want, "windows of 4")
    # and the evaluators of the one-window batch agree with both to rounding
    assert np.max(np.abs(fields(sol, levels(kw))["u"] - got["u"])) <= 1e-12 * np.max(np.abs(got["u"]))


@pytest.mark.parametrize("test_id", ["6d", "6e", "6f", "6g", "6h"])
def test_hapke_problems_of_the_reference_through_the_request(test_id):
    """DISORT's test problem 6 with Hapke's surface (B0, HH, W) = (1, 0.06, 0.6), stated as three numbers: the fluxes against the
    reference's goldens at the 1e-5 that test_device_bdrf_fourier_integration_hapke holds the sampled path to (the reference
    integrates the modes adaptively; 4096 azimuths leave 6e-6 at the hot-spot cusp, profiles/surface.json)."""
    import pydisort_amd
    call = goldens.load(test_id)[0]
    kw = call["kwargs"]
    NQuad, N = kw["NQuad"], kw["NQuad"] // 2
    nb = len(kw["BDRF_Fourier_modes"])
    tau = np.atleast_1d(np.asarray(kw["tau_arr"], float))[None, :]
    nl = tau.shape[1]
    Leg = np.asarray(kw["Leg_coeffs_all"], float)
    Leg = np.broadcast_to(Leg if Leg.ndim == 2 else Leg[None, :], (nl, Leg.shape[-1]))[None]
    sp = kw.get("s_poly_coeffs")
    sp = None if sp is None or np.size(sp) == 0 else np.asarray(sp, float).reshape(1, nl, -1)
    only_flux = bool(kw.get("only_flux", False))

    def bc(b):
        return np.asarray(b, float) if np.ndim(b) == 0 else np.asarray(b, float).reshape(1, N, -1)[:, :, 0]

    _, sol = pydisort_amd.pydisort_batch(tau, np.atleast_1d(np.asarray(kw["omega_arr"], float))[None, :], NQuad, Leg, [float(kw["mu0"])],
                                         [float(kw["I0"])], [float(kw["phi0"])], only_flux=only_flux, b_pos=bc(kw.get("b_pos", 0)),
                                         b_neg=bc(kw.get("b_neg", 0)), s_poly_coeffs=sp, NBDRF=min(nb, 1 if only_flux else NQuad),
                                         surface=dict(model="hapke", params=(1, 0.06, 0.6), nphi=4096))
    q = sol.plan.get_bdrf()[0]
    for m in range(q.shape[1]):
        assert np.max(np.abs(q[0, m] - kw["BDRF_Fourier_modes"][m].tab)) < 1e-5
    checked = 0
    for ev in call["evals"]:
        if ev["name"] not in ("flux_up", "flux_down") or ev["kwargs"]:
            continue
        t = np.atleast_1d(np.asarray(ev["args"][0], float))[None, :]
        if ev["name"] == "flux_up":
            want = np.atleast_1d(ev["out"])
            assert np.max(np.abs(sol.flux_up(t)[0] - want)) <= 1e-5 * max(1.0, np.max(np.abs(want)))
        else:
            gd, gdir = sol.flux_down(t)
            wd, wdir = ev["out"]
            assert np.max(np.abs(gd[0] - np.atleast_1d(wd))) <= 1e-5 * max(1.0, np.max(np.abs(wd)))
            assert np.max(np.abs(gdir[0] - np.atleast_1d(wdir))) <= 1e-5 * max(1.0, np.max(np.abs(wdir)))
        checked += 1
    assert checked > 0


@pytest.mark.parametrize("model", ["hapke", "lambert"])
def test_without_a_beam_the_mu0_column_stays_zero(model):
    import pydisort_amd
    kw, par = columns(16, beam=False), parameters(model)
    rng = np.random.default_rng(9)
    _, sol = pydisort_amd.pydisort_batch(**kw, b_pos=rng.uniform(0.1, 0.4, C), surface=dict(model=model, params=par, nphi=44))
    q, q0 = sol.plan.get_bdrf()
    assert np.all(q0 == 0.0) and np.all(np.isfinite(q)) and np.all(q[:, 0] > 0)
    f = fields(sol, levels(kw))
    assert all(np.all(np.isfinite(v)) for v in f.values()) and np.max(f["flux_up"]) > 0 and np.all(f["flux_down_direct"] == 0)
