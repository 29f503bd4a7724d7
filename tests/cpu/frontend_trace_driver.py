#!/usr/bin/env python3
"""Driver of tests/test_frontend_trace_cpu.py: ONE scripted scenario of calls into the Python front end (pydisort_amd) over the real
host code of csrc/rtd_api.hip, the stand-in runtime of tests/cpu/fake_hip and the shadow launchers, built with -DFAKE_HIP_TRACE as a
plain shared library that RTD_LIB names (tests/host_program.py: build_trace_library).  One scenario per process, so that allocation
and stream ordinals start at zero.  After every front-end call it prints the mark line naming the call, the runtime calls the library
made for it (fake_trace_take), and what came back: `key shape dtype` per array, or `raises <Type>: <message>`.  Never an array's
values: the kernels rtd_api.hip defines itself do real arithmetic here, and values would tie the recording to a libm.

Usage: RTD_LIB=<trace library> FAKE_HIP_TOTAL=<bytes> python tests/cpu/frontend_trace_driver.py <scenario>"""
import ctypes
import gc
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path += [ROOT, os.path.join(ROOT, "pythonic-disort_amd")]  # appended: a package put on PYTHONPATH is the one that is traced
import pydisort_amd as amd  # noqa: E402
from pydisort_amd import _engine, _lib, synthetic  # noqa: E402
from pydisort_amd._engine import Plan  # noqa: E402
from pydisort_amd.band import level_tau as band_level_tau  # noqa: E402

LIB = _lib.load()
LIB.fake_trace_take.restype = ctypes.c_char_p
LIB.fake_trace_mark.argtypes = [ctypes.c_char_p]
PHI = np.array([0.0, 1.0, 2.5])
ORDERS = (("value", {}), ("antiderivative", dict(is_antiderivative_wrt_tau=True)), ("derivative", dict(is_derivative_wrt_tau=True)))


def describe(r, name="->"):
    if isinstance(r, dict):
        for k, v in r.items():
            describe(v, f"{name} {k}")
    elif isinstance(r, (tuple, list)):
        for i, v in enumerate(r):
            describe(v, f"{name} [{i}]")
    elif isinstance(r, (np.ndarray, np.generic)):
        print(name, tuple(r.shape), r.dtype)
    elif r is None or isinstance(r, (bool, int, str)):
        print(name, repr(r))
    else:
        print(name, type(r).__name__)


def call(label, fn, *args, **kwargs):
    """One front-end call: the mark, the runtime calls it made, what it returned or raised."""
    LIB.fake_trace_mark(label.encode())
    result, error = None, None
    try:
        result = fn(*args, **kwargs)
    except Exception as e:  # noqa: BLE001  (what is raised is what is recorded)
        error = f"raises {type(e).__name__}: {e}"
    sys.stdout.write(LIB.fake_trace_take().decode())
    if error is None:
        describe(result)
    else:
        print(error)
    sys.stdout.flush()
    return result


def close(label, plan):
    call(f"{label}.close()", plan.close)


def pts(cfg, fractions=(0.25, 0.75)):
    return cfg["tau_arr"][:, -1:] * np.asarray(fractions)[None, :]


def levels(cfg):
    return np.concatenate((np.zeros((cfg["tau_arr"].shape[0], 1)), cfg["tau_arr"]), axis=1)


def small(C=3, NQuad=8, first=0):
    return synthetic.cfg4_columns(C, first=first, L=3, NQuad=NQuad)


def thermal_dict(C, L, **over):
    th = dict(TEMPER=np.linspace(220.0, 290.0, L + 1), WVNMLO=500.0, WVNMHI=600.0, BTEMP=295.0, TTEMP=3.0, TEMIS=1.0)
    th.update(over)
    return th


def band_inputs(P=2, G=3, S=2, L=3, nleg=10):
    rng = np.random.default_rng(7)
    return dict(dtau_abs=rng.uniform(0.01, 0.5, (P, G, L)), dtau_spec=rng.uniform(0.05, 0.3, (P, L, S)),
                omega_spec=rng.uniform(0.5, 0.95, (P, L, S)), Leg_spec=np.array([0.7, 0.8])[:S, None] ** np.arange(nleg)[None, :],
                NQuad=8, mu0=0.6, I0=np.array([1.0, 2.0, 0.5])[:G], phi0=0.0)


def evaluators(name, sol, tau, mu):
    """Every BatchSolution evaluator in each of the three orders."""
    for what, kw in ORDERS:
        call(f"{name}.u {what}", sol.u, tau, PHI, **kw)
        call(f"{name}.u0 {what}", sol.u0, tau, **kw)
        call(f"{name}.flux_up {what}", sol.flux_up, tau, **kw)
        call(f"{name}.flux_down {what}", sol.flux_down, tau, **kw)
        call(f"{name}.flux_act_up {what}", sol.flux_act_up, tau, **kw)
        call(f"{name}.flux_act_down {what}", sol.flux_act_down, tau, **kw)
        call(f"{name}.u_at {what}", sol.u_at, mu, tau, PHI, **kw)
        call(f"{name}.u0_at {what}", sol.u0_at, mu, tau, **kw)


def plan_queries(name, plan):
    for m in ("retained", "retained_form", "windows", "device_bytes", "column_status", "max_sweeps", "pivoted_chains", "synchronize"):
        call(f"{name}.{m}()", getattr(plan, m))
    call(f"{name}.result_dev_ptrs() (bytes only)", lambda: tuple(b for _, b in plan.result_dev_ptrs()))


def throughput_form(name, plan, cfg):
    C = cfg["tau_arr"].shape[0]
    call(f"{name}.set_eval_points", plan.set_eval_points, levels(cfg), PHI)
    call(f"{name}.run()", plan.run)
    call(f"{name}.fetch()", plan.fetch)
    call(f"{name}.run_fetch()", plan.run_fetch)
    call(f"{name}.run_fetch(out: fluxes only)", plan.run_fetch, dict(flux_up=np.empty((C, 4)), flux_down_diffuse=np.empty((C, 4))))
    call(f"{name}.set_eval_order(-1)", plan.set_eval_order, -1)
    call(f"{name}.run_fetch() antiderivatives", plan.run_fetch)
    call(f"{name}.set_eval_order(0)", plan.set_eval_order, 0)
    call(f"{name}.fetch_actinic()", plan.fetch_actinic)
    call(f"{name}.fetch_actinic(out: one given)", plan.fetch_actinic, dict(flux_act_up=np.empty((C, 4))))
    call(f"{name}.set_view([nmu])", plan.set_view, [0.5, -0.5])
    call(f"{name}.fetch_view()", plan.fetch_view)
    call(f"{name}.fetch_view(u0, out given)", plan.fetch_view, ("u0",), dict(u0_mu=np.empty((C, 2, 4))))
    call(f"{name}.set_view(None)", plan.set_view, None)
    call(f"{name}.invalidate_tables()", plan.invalidate_tables)
    call(f"{name}.run() after invalidate_tables", plan.run)


def scenario_batch():
    cfg = small()
    sol = call("pydisort_batch host-prepared", amd.pydisort_batch, **cfg)[1]
    tau = pts(cfg)
    evaluators("sol", sol, tau, [0.3, -0.7])
    call("sol.u one tau row for all columns", sol.u, np.array([0.1, 0.2]), PHI)
    call("sol.u_at mu per column", sol.u_at, np.tile([0.3, -0.7, 1.0], (3, 1)), tau, PHI)
    call("sol.plan.evaluate want everything", sol.plan.evaluate, tau, PHI, want=("u", "u0", "flux", "ulast", "act", "view"))
    call("sol.plan.evaluate view_u alone, no azimuths", sol.plan.evaluate, tau, None, want=("view_u",))
    plan_queries("sol.plan", sol.plan)
    call("sol.plan.tensors(2)", sol.plan.tensors, 2)
    call("sol.plan.get_bdrf()", sol.plan.get_bdrf)
    call("sol.plan.enable_timing()", sol.plan.enable_timing)
    call("sol.plan.solve()", sol.plan.solve)
    call("sol.plan.timing()", sol.plan.timing)
    call("sol.plan.enable_timing(False)", sol.plan.enable_timing, False)
    throughput_form("sol.plan", sol.plan, cfg)
    close("sol.plan", sol.plan)
    nt = call("pydisort_batch host-prepared NT_cor", amd.pydisort_batch, NT_cor=True, **cfg)[1]
    call("nt.u", nt.u, tau, PHI)
    call("nt.plan.evaluate skip_nt", nt.plan.evaluate, tau, PHI, want=("u",), skip_nt=True)
    call("nt.plan.get_nt()", nt.plan.get_nt)
    call("nt.plan.clear_nt()", nt.plan.clear_nt)
    close("nt.plan", nt.plan)
    for shard in ((0, 3), (2, 3)):
        sh = call(f"pydisort_batch mode_shard={shard}", amd.pydisort_batch, mode_shard=shard, NT_cor=True, **cfg)[1]
        call("shard.u", sh.u, tau, PHI)
        call("shard.flux_up", sh.flux_up, tau)
        close("shard.plan", sh.plan)
    rng = np.random.default_rng(1)
    sm = call("pydisort_batch bdrf_samples", amd.pydisort_batch, bdrf_samples=(rng.uniform(0.1, 0.3, (3, 4, 4, 12)), rng.uniform(0.1, 0.3, (3, 4, 12))),
              NBDRF=3, **cfg)[1]
    call("samples.u", sm.u, tau, PHI)
    call("samples.plan.get_bdrf()", sm.plan.get_bdrf)
    close("samples.plan", sm.plan)
    first = call("pydisort_batch first of two batches", amd.pydisort_batch, **cfg)[1]
    cfg_b = small(first=50)
    second = call("pydisort_batch second batch, solve deferred", amd.pydisort_batch, _defer_solve=True, **cfg_b)[1]
    call("first.plan.set_columns(second)", first.plan.set_columns, second.prep)
    call("first.plan.solve()", first.plan.solve)
    call("first.plan.evaluate", first.plan.evaluate, pts(cfg_b), PHI)
    close("second.plan", second.plan)
    close("first.plan", first.plan)
    thermal = synthetic.cfg3_columns(3, big=False)  # (thermal polynomials: set_columns takes s_local)
    th = call("pydisort_batch host-prepared with s_poly and tables", amd.pydisort_batch, **thermal)[1]
    call("s_poly.u", th.u, pts(thermal), PHI)
    close("s_poly.plan", th.plan)
    ls = call("pydisort_batch for layer shards", amd.pydisort_batch, _defer_solve=True, **cfg)[1]
    call("layers.plan.solve_layers(0, 2)", ls.plan.solve_layers, 0, 2)
    call("layers.plan.solve_layers(2, 1)", ls.plan.solve_layers, 2, 1)
    call("layers.plan.solve_bc()", ls.plan.solve_bc)
    call("layers.plan.evaluate", ls.plan.evaluate, tau, PHI)
    close("layers.plan", ls.plan)
    prep = amd.pydisort_batch(_defer_solve=True, **cfg)[1]
    close("prep.plan", prep.plan)
    call("solve_batch_once", _engine.solve_batch_once, prep.prep, tau, PHI)
    call("solve_tensors_once", _engine.solve_tensors_once, prep.prep, 1)
    call("planck_band", _engine.planck_band, np.array([250.0, 300.0]), 500.0, 600.0)
    call("device_count", _engine.device_count)
    for m in ("pool_bytes", "pool_trim", "free_device_bytes", "pool_set_limit"):
        call(f"Plan.{m}()", getattr(Plan, m))


def scenario_raw():
    cfg = synthetic.cfg5_columns(5, L=3, NQuad=8)  # (two BDRF modes, a thermal polynomial, a boundary source)
    tau = pts(cfg)
    for retain in (False, "full", "lean"):
        name = f"raw[{retain}]"
        sol = call(f"pydisort_batch device_prepare NT_cor windows of 2 retain={retain!r}", amd.pydisort_batch, device_prepare=True, NT_cor=True,
                   work_columns=2, retain=retain, **cfg)[1]
        plan_queries(name + ".plan", sol.plan)
        call(name + ".u", sol.u, tau, PHI)
        call(name + ".u derivative", sol.u, tau, PHI, is_derivative_wrt_tau=True)
        call(name + ".flux_down", sol.flux_down, tau)
        call(name + ".flux_act_up", sol.flux_act_up, tau)
        call(name + ".u0_at", sol.u0_at, [0.2], tau)
        call(name + ".plan.get_nt()", sol.plan.get_nt)
        call(name + ".plan.get_bdrf()", sol.plan.get_bdrf)
        call(name + ".plan.tensors(4)", sol.plan.tensors, 4)
        if retain == "full":
            throughput_form(name + ".plan", sol.plan, cfg)
            call(name + ".plan.request_nt(0)", sol.plan.request_nt, 0)
            call(name + ".plan.set_columns_raw again", sol.plan.set_columns_raw, sol.prep["raw"])
            call(name + ".plan.solve()", sol.plan.solve)
            call(name + ".plan.get_nt() after the request is withdrawn", sol.plan.get_nt)
        close(name + ".plan", sol.plan)
    one = call("pydisort_batch device_prepare one window only_flux", amd.pydisort_batch, device_prepare=True, only_flux=True, NT_cor=True, **cfg)[1]
    call("one.flux_up", one.flux_up, tau)
    call("one.plan.tensors(0)", one.plan.tensors, 0)
    close("one.plan", one.plan)


def scenario_thermal():
    cfg = small()
    C, L, N = 3, 3, 4
    tau = pts(cfg)
    rng = np.random.default_rng(3)
    cases = (("scalars", thermal_dict(C, L, emissivity=0.9)),
             ("per column", thermal_dict(C, L, TEMPER=np.tile(np.linspace(220.0, 290.0, L + 1), (C, 1)), WVNMLO=np.full(C, 500.0), WVNMHI=np.full(C, 600.0),
                                         BTEMP=np.full(C, 295.0), TTEMP=np.full(C, 3.0), TEMIS=np.full(C, 0.5), emissivity=np.full(C, 0.9))),
             ("emissivity [C, N]", thermal_dict(C, L, emissivity=rng.uniform(0.8, 1.0, (C, N)))),
             ("no boundary emission", thermal_dict(C, L, BTEMP=None, TTEMP=None, TEMIS=None)))
    for what, th in cases:
        sol = call(f"pydisort_batch thermal {what}", amd.pydisort_batch, thermal=th, **cfg)[1]
        call("thermal.u", sol.u, tau, PHI)
        call("thermal.flux_up derivative", sol.flux_up, tau, is_derivative_wrt_tau=True)
        if what == "scalars":
            call("thermal.plan.set_columns_thermal again", sol.plan.set_columns_thermal, sol.prep["raw"], sol.prep["thermal"])
            call("thermal.plan.solve()", sol.plan.solve)
            call("thermal.u0", sol.u0, tau)
        close("thermal.plan", sol.plan)
    surfaces = (("lambert, Kirchhoff", dict(model="lambert", params=0.3), thermal_dict(C, L), 1),
                ("hapke", dict(model="hapke", params=[1.0, 0.06, 0.6]), None, 3),
                ("ocean per column", dict(model="ocean", params=np.array([[5.0, 1.34, 0.01], [7.0, 1.34, 0.0], [3.0, 1.33, 0.02]])), None, 2))
    for what, sf, th, nb in surfaces:
        sol = call(f"pydisort_batch surface {what}", amd.pydisort_batch, surface=sf, thermal=th, NBDRF=nb, **cfg)[1]
        call("surface.u", sol.u, tau, PHI)
        call("surface.plan.get_bdrf()", sol.plan.get_bdrf)
        if what == "hapke":
            call("surface.plan.request_surface(rpv by id, per column)", sol.plan.request_surface, 3, np.tile([0.2, 0.8, -0.1, 0.2], (C, 1)), 64)
            call("surface.plan.set_columns_raw under the new request", sol.plan.set_columns_raw, sol.prep["raw"])
            call("surface.plan.solve()", sol.plan.solve)
            call("surface.plan.request_surface(None)", sol.plan.request_surface, None)
        close("surface.plan", sol.plan)


def band_evaluators(name, sol):
    call(f"{name}.flux_up()", sol.flux_up)
    call(f"{name}.flux_down([0, 3])", sol.flux_down, [0, 3])
    call(f"{name}.u0(1)", sol.u0, 1)
    call(f"{name}.u", sol.u, [0, 2], PHI)
    call(f"{name}.flux_act_up()", sol.flux_act_up)
    call(f"{name}.flux_act_down()", sol.flux_act_down)
    call(f"{name}.actinic_flux()", sol.actinic_flux)
    call(f"{name}.u_at mu [nmu]", sol.u_at, [0.4, -0.4], [0, 3], PHI)
    call(f"{name}.u0_at mu per profile", sol.u0_at, np.array([[0.4, -0.4], [0.5, -0.5]]))
    call(f"{name}.net_flux_convergence()", sol.net_flux_convergence)
    call(f"{name}.columns.u", sol.columns.u, np.array([0.05, 0.1]), PHI)


def scenario_band():
    b = band_inputs()
    w1, w2 = np.array([0.2, 0.5, 0.3]), np.array([[0.2, 0.5, 0.3], [1.0, 0.0, 2.0]])
    sol = call("pydisort_band weights [G], NT_cor", amd.pydisort_band, weights=w1, NT_cor=True, **b)[1]
    band_evaluators("band", sol)
    call("band.plan.get_nt()", sol.plan.get_nt)
    plan, lev = sol.plan, band_level_tau(sol.plan.prep["tau"])
    call("band.plan.evaluate_band want everything", plan.evaluate_band, lev, PHI, want=("u", "u0", "flux", "act", "view"))
    call("band.plan.evaluate_band derivative, flux only", plan.evaluate_band, lev, None, want=("flux",), derivative=True)
    call("band.plan.set_eval_points", plan.set_eval_points, lev, PHI)
    call("band.plan.run()", plan.run)
    call("band.plan.fetch_band()", plan.fetch_band)
    call("band.plan.fetch_band(u0)", plan.fetch_band, ("u0",))
    call("band.plan.fetch_band_actinic()", plan.fetch_band_actinic)
    call("band.plan.fetch_band_view(u0)", plan.fetch_band_view, ("u0",))
    call("band.plan.fetch()", plan.fetch)
    call("band.plan.set_band_weights [2, G]", plan.set_band_weights, w2)
    call("band.plan.fetch_band() under the new weights", plan.fetch_band)
    call("band.plan.set_band_weights(None)", plan.set_band_weights, None)
    call("band.plan.set_columns_band again", plan.set_columns_band, plan.prep["band"], plan.prep["cols"])
    close("band.plan", plan)
    P, L = 2, 3
    th = dict(TEMPER=np.array([np.linspace(220.0, 290.0, L + 1), np.linspace(230.0, 300.0, L + 1)]), WVNMLO=500.0, WVNMHI=600.0, BTEMP=np.array([295.0, 305.0]),
              TTEMP=3.0, TEMIS=1.0)
    sol = call("pydisort_band weights [2, G], thermal and surface per profile", amd.pydisort_band, weights=w2, thermal=th,
               surface=dict(model="lambert", params=np.array([0.1, 0.3])), NBDRF=1, b_pos=0.1, b_neg=np.array([0.0, 0.05]), **b)[1]
    band_evaluators("band2", sol)
    call("band2.plan.get_bdrf()", sol.plan.get_bdrf)
    close("band2.plan", sol.plan)
    sol = call("pydisort_band tables per profile, only_flux", amd.pydisort_band, weights=w1, only_flux=True, bdrf_q=np.full((P, 1, 4, 4), 0.2),
               bdrf_q0=np.full((P, 1, 4), 0.2), **b)[1]
    call("band3.flux_up()", sol.flux_up)
    close("band3.plan", sol.plan)
    call("band_mix", amd.band_mix, b["dtau_abs"], b["dtau_spec"], b["omega_spec"], b["Leg_spec"], 8)


def scenario_streamed():
    cfg = synthetic.cfg5_columns(5, L=3, NQuad=8)
    C, Q, tau = 5, 8, levels(cfg)
    call("solve_columns_streamed out=None, default window", amd.solve_columns_streamed, cfg, tau, PHI)
    call("solve_columns_streamed windows of 2", amd.solve_columns_streamed, cfg, tau, PHI, chunk_columns=2)
    out = dict(flux_up=np.empty((C, 4)), flux_down_diffuse=np.empty((C, 4)), flux_down_direct=np.empty((C, 4)), u=np.empty((C, Q, 4, 3)),
               flux_act_up=np.empty((C, 4)), u0_mu=np.empty((C, 2, 4)))
    call("solve_columns_streamed partial out, actinic, mu per column", amd.solve_columns_streamed, cfg, tau, PHI, chunk_columns=2, out=out,
         actinic=True, mu=np.tile([0.3, -0.3], (C, 1)))
    call("solve_columns_streamed mu shared, u left on the device", amd.solve_columns_streamed, cfg, tau, PHI,
         out=dict(u0=np.empty((C, Q, 4)), flux_up=np.empty((C, 4)), flux_down_diffuse=np.empty((C, 4)), flux_down_direct=np.empty((C, 4))), mu=[0.3])
    for order in (-1, 0, 1):
        call(f"solve_columns_streamed tau_order={order}", amd.solve_columns_streamed, cfg, tau, PHI, chunk_columns=2, tau_order=order)
    call("solve_columns_streamed only_flux, actinic, mu", amd.solve_columns_streamed, cfg, tau, PHI, only_flux=True, actinic=True, mu=[0.3, -0.3])
    nt = dict(small(C), NT_cor=True)
    call("solve_columns_streamed NT_cor, surface in cfg", amd.solve_columns_streamed, dict(nt, surface=dict(model="lambert", params=0.2), NBDRF=2),
         levels(nt), PHI, chunk_columns=2)
    b = band_inputs()
    w2 = np.array([[0.2, 0.5, 0.3], [1.0, 0.0, 2.0]])
    call("solve_band_streamed", amd.solve_band_streamed, weights=w2[0], phi=PHI, **b)
    call("solve_band_streamed actinic, mu, levels, windows of 4", amd.solve_band_streamed, weights=w2, levels=[0, 3], phi=PHI, chunk_columns=4, actinic=True,
         mu=[0.4, -0.4], **b)
    call("solve_band_streamed only_flux, mu per profile, NT_cor", amd.solve_band_streamed, weights=w2, only_flux=True, mu=np.array([[0.4], [0.5]]), NT_cor=True, **b)


def scenario_single():
    shapes = [synthetic.column_kwargs(small(1, nq, first=k), 0) for k, nq in enumerate((8, 16, 8, 16))]
    tau = np.array([0.1, 0.2])
    for k, kw in enumerate(shapes):  # (`res` is rebound: the closures of the call before go, and their plan serves the next call of its shape)
        res = call(f"pydisort() call {k}, NT_cor on", amd.pydisort, NT_cor=True, **kw)
        call("u", res[4], tau, PHI)
        call("u with return_Fourier_error, return_tau_arr", res[4], tau, PHI, False, True, True)
        call("u derivative", res[4], tau, PHI, is_derivative_wrt_tau=True)
        call("u derivative with return_Fourier_error", res[4], tau, PHI, return_Fourier_error=True, is_derivative_wrt_tau=True)
        call("u0 antiderivative with the reclassification term", res[3], tau, True, True, True)
        call("flux_up scalar tau", res[1], 0.1)
        call("flux_down", res[2], tau, return_tau_arr=True)
        call("flux_down outside the atmosphere", res[2], 1e9)
    res = call("pydisort() NT_cor off on a plan that had it (clear_nt)", amd.pydisort, **shapes[0])
    call("u", res[4], tau, PHI)
    res = call("pydisort() only_flux", amd.pydisort, only_flux=True, **shapes[1])
    call("flux_up", res[1], tau)
    call("u0", res[3], tau)
    call("the call's plan: fetch_actinic()", res[3].__self__.plan.fetch_actinic)
    del res
    for lst in list(sys.modules["pydisort_amd.pydisort"]._IDLE.values()):  # the plans that wait for a next call of their shape
        for p in lst:
            close("idle plan", p)


def scenario_refused():
    cfg = small()
    C, L, N = 3, 3, 4
    tau = pts(cfg)
    host = amd.pydisort_batch(**cfg)[1]
    plan = host.plan
    LIB.fake_trace_take()
    other = amd.pydisort_batch(_defer_solve=True, **small(5))[1]
    call("set_columns of another size", plan.set_columns, other.prep)
    close("other.plan", other.plan)
    nobeam = amd.pydisort_batch(_defer_solve=True, **dict(cfg, I0=0.0, b_neg=1.0))[1]
    call("set_columns with a beam on a plan without", nobeam.plan.set_columns, host.prep)
    close("nobeam.plan", nobeam.plan)
    call("evaluate antiderivative and derivative", plan.evaluate, tau, PHI, antiderivative=True, derivative=True)
    call("sol.u antiderivative and derivative", host.u, tau, PHI, True, is_derivative_wrt_tau=True)
    call("sol.u outside the atmosphere", host.u, np.array([1e9]), PHI)
    plan.set_eval_points(tau, PHI)
    LIB.fake_trace_take()
    call("fetch_band without weights", plan.fetch_band)
    call("get_nt without Nakajima-Tanaka inputs (the library refuses)", plan.get_nt)
    call("evaluate_band without weights", plan.evaluate_band, tau)
    call("fetch_band_actinic without weights", plan.fetch_band_actinic)
    call("fetch_band_view without weights", plan.fetch_band_view)
    call("fetch_view without a view", plan.fetch_view)
    call("evaluate view without a view", plan.evaluate, tau, PHI, want=("view",))
    call("set_view mu [2, nmu] on 3 columns", plan.set_view, np.zeros((2, 2)))
    call("set_view |mu| > 1", plan.set_view, [1.5])
    call("set_view empty", plan.set_view, np.zeros((0,)))
    call("set_eval_order(2)", plan.set_eval_order, 2)
    call("set_band_weights [G]", plan.set_band_weights, np.ones(3))
    call("set_band_weights G not dividing C", plan.set_band_weights, np.ones((1, 2)))
    call("set_bdrf_samples rho_qq of a wrong shape", plan.set_bdrf_samples, np.zeros((C, N, 3, 8)))
    call("set_bdrf_samples rho_q0 of a wrong shape", plan.set_bdrf_samples, np.zeros((C, N, N, 8)), np.zeros((C, N, 7)))
    call("request_surface unknown model", plan.request_surface, "snow", [0.1])
    call("request_surface five parameters", plan.request_surface, "rpv", np.zeros(5))
    plan.evaluate(tau, PHI)
    plan.set_view([0.5, -0.5])
    LIB.fake_trace_take()
    shape = (C, 2)
    bad = (("of a wrong shape", np.empty((C, 3))), ("float32", np.empty(shape, dtype=np.float32)), ("not contiguous", np.empty((2, C)).T),
           ("a list", [[0.0] * 2] * C))
    ro = np.empty(shape)
    ro.flags.writeable = False
    for what, a in bad + (("read-only", ro),):
        call(f"fetch_actinic out {what}", plan.fetch_actinic, dict(flux_act_down_direct=a))
    ro = np.empty((C, 2, 2))
    ro.flags.writeable = False
    for what, a in (("of a wrong shape", np.empty((C, 2, 2, 4))), ("read-only", ro), ("not contiguous", np.empty((C, 2, 4))[:, :, ::2])):
        call(f"fetch_view out {what}", plan.fetch_view, ("u", "u0"), dict(u_mu=a if a.ndim == 4 else None, u0_mu=a if a.ndim == 3 else None))
    close("host.plan", plan)

    rsol = amd.pydisort_batch(device_prepare=True, _defer_solve=True, **synthetic.cfg5_columns(C, L=3, NQuad=8))[1]
    rplan, raw = rsol.plan, rsol.prep["raw"]
    LIB.fake_trace_take()
    call("set_columns_raw without tau_arr", rplan.set_columns_raw, dict(raw, tau_arr=None))
    call("set_columns_raw without s_poly (Ns = 2)", rplan.set_columns_raw, dict(raw, s_poly=None))
    call("set_columns_raw without bdrf_q0 (NBDRF = 2)", rplan.set_columns_raw, dict(raw, bdrf_q0=None))
    call("set_columns_raw without leg", rplan.set_columns_raw, dict(raw, leg=None))
    call("set_columns_raw leg with too few moments", rplan.set_columns_raw, dict(raw, leg=raw["leg"][:, :, :4]))
    call("set_columns_raw omega_arr of a wrong shape", rplan.set_columns_raw, dict(raw, omega_arr=np.zeros((C, L + 1))))
    call("set_columns_raw b_pos of a wrong shape", rplan.set_columns_raw, dict(raw, b_pos=np.zeros((C, N))))
    call("set_columns_thermal with s_poly", rplan.set_columns_thermal, raw, thermal_dict(C, L))
    call("request_surface on the plan", rplan.request_surface, "lambert", [0.2])
    call("set_columns_raw with tables under a surface request", rplan.set_columns_raw, raw)
    close("raw.plan", rplan)
    nb = amd.pydisort_batch(device_prepare=True, _defer_solve=True, **dict(cfg, I0=0.0, b_neg=1.0))[1]
    call("set_columns_raw with a beam on a plan without", nb.plan.set_columns_raw, dict(nb.prep["raw"], I0=np.ones(C)))
    call("set_columns_thermal on a plan with Ns = 0", nb.plan.set_columns_thermal, nb.prep["raw"], thermal_dict(C, L))
    close("nobeam raw.plan", nb.plan)

    tsol = amd.pydisort_batch(thermal=thermal_dict(C, L, emissivity=0.9), _defer_solve=True, **cfg)[1]
    tplan, traw, th = tsol.plan, tsol.prep["raw"], tsol.prep["thermal"]
    LIB.fake_trace_take()
    for k in ("TEMPER", "WVNMLO", "WVNMHI"):
        call(f"set_columns_thermal without {k}", tplan.set_columns_thermal, traw, dict(th, **{k: None}))
    call("set_columns_thermal BTEMP of a wrong shape", tplan.set_columns_thermal, traw, dict(th, BTEMP=np.zeros(2)))
    call("set_columns_thermal emissivity [C]", tplan.set_columns_thermal, traw, dict(th, emissivity=np.ones(C)))
    call("set_columns_raw on a thermal plan without s_poly", tplan.set_columns_raw, traw)
    close("thermal.plan", tplan)

    b = band_inputs()
    w = np.array([0.2, 0.5, 0.3])
    bsol = amd.pydisort_band(weights=w, _defer_solve=True, **b)[1]
    bplan, band, cols = bsol.plan, bsol.plan.prep["band"], bsol.plan.prep["cols"]
    LIB.fake_trace_take()
    call("set_mode_shard on a band plan", bplan.set_mode_shard, 0, 2, 8)
    call("set_mode_shard (0, 1, M) on a band plan", bplan.set_mode_shard, 0, 1, 8)
    call("comm_init on a band plan", bplan.comm_init, b"", 0, 1)
    call("set_view mu differing within a profile", bplan.set_view, np.linspace(-0.6, 0.6, 12).reshape(6, 2))
    call("set_columns_band without leg_spec", bplan.set_columns_band, dict(band, leg_spec=None), cols)
    call("set_columns_band dtau_abs with P G != C", bplan.set_columns_band, dict(band, dtau_abs=band["dtau_abs"][:1]), cols)
    call("set_columns_band dtau_abs with another L", bplan.set_columns_band, dict(band, dtau_abs=band["dtau_abs"][:, :, :2]), cols)
    call("set_columns_band omega_spec of a wrong shape", bplan.set_columns_band, dict(band, omega_spec=band["omega_spec"][:, :, :1]), cols)
    call("set_columns_band leg_spec with too few moments", bplan.set_columns_band, dict(band, leg_spec=band["leg_spec"][:, :8]), cols)
    call("set_columns_band without mu0", bplan.set_columns_band, band, dict(cols, mu0=None))
    call("set_columns_band b_neg of a wrong shape", bplan.set_columns_band, band, dict(cols, b_neg=np.zeros((6, 4))))
    call("set_columns_band thermal on a plan with Ns = 0", bplan.set_columns_band, band, cols, thermal_dict(6, L))
    call("request_surface on the band plan (NBDRF = 0: the library refuses)", bplan.request_surface, "lambert", [0.2])
    close("band.plan", bplan)
    nbb = amd.pydisort_band(weights=w, _defer_solve=True, **dict(b, I0=0.0, b_neg=1.0))[1]
    call("set_columns_band with a beam on a plan without", nbb.plan.set_columns_band, band, cols)
    close("nobeam band.plan", nbb.plan)
    tb = amd.pydisort_band(weights=w, _defer_solve=True, thermal=thermal_dict(6, L), surface=dict(model="lambert", params=0.1), NBDRF=1, **b)[1]
    tband, tcols, tth = tb.plan.prep["band"], tb.plan.prep["cols"], tb.plan.prep["thermal"]
    LIB.fake_trace_take()
    call("set_columns_band without thermal on a plan with Ns = 2", tb.plan.set_columns_band, tband, tcols)
    call("set_columns_band thermal without WVNMLO", tb.plan.set_columns_band, tband, tcols, dict(tth, WVNMLO=None))
    call("set_columns_band thermal TEMPER of a wrong shape", tb.plan.set_columns_band, tband, tcols, dict(tth, TEMPER=np.zeros((6, L))))
    call("set_columns_band with tables under a surface request", tb.plan.set_columns_band, tband, dict(tcols, bdrf_q=np.zeros((6, 1, 4, 4)), bdrf_q0=np.zeros((6, 1, 4))), tth)
    call("request_surface(None) on the band plan", tb.plan.request_surface, None)
    call("set_columns_band without tables (NBDRF = 1, no request)", tb.plan.set_columns_band, tband, tcols, tth)
    close("thermal band.plan", tb.plan)
    shard = amd.pydisort_batch(mode_shard=(1, 2), _defer_solve=True, **cfg)[1]
    LIB.fake_trace_take()
    call("set_band_weights on a mode shard", shard.plan.set_band_weights, np.ones((1, 3)))
    call("set_columns_band on a mode shard", shard.plan.set_columns_band, band, cols)
    close("shard.plan", shard.plan)

    s5 = synthetic.cfg5_columns(5, L=3, NQuad=8)
    t5, Q = levels(s5), 8
    full = lambda: dict(u=np.empty((5, Q, 4, 3)), u0=np.empty((5, Q, 4)), flux_up=np.empty((5, 4)), flux_down_diffuse=np.empty((5, 4)),  # noqa: E731
                        flux_down_direct=np.empty((5, 4)))
    call("solve_columns_streamed tau_order=2", amd.solve_columns_streamed, s5, t5, PHI, tau_order=2)
    call("solve_columns_streamed mu of a wrong shape", amd.solve_columns_streamed, s5, t5, PHI, mu=np.zeros((4, 2)))
    call("solve_columns_streamed |mu| > 1", amd.solve_columns_streamed, s5, t5, PHI, mu=[2.0])
    call("solve_columns_streamed tau outside the atmosphere", amd.solve_columns_streamed, s5, t5 * 2, PHI)
    o = full()
    del o["u0"]
    call("solve_columns_streamed out without u0", amd.solve_columns_streamed, s5, t5, PHI, out=o)
    call("solve_columns_streamed out u of a wrong shape", amd.solve_columns_streamed, s5, t5, PHI, out=dict(full(), u=np.empty((5, Q, 4, 2))))
    call("solve_columns_streamed out flux_up float32", amd.solve_columns_streamed, s5, t5, PHI, out=dict(full(), flux_up=np.empty((5, 4), dtype=np.float32)))
    call("solve_columns_streamed out flux_up not contiguous", amd.solve_columns_streamed, s5, t5, PHI, out=dict(full(), flux_up=np.empty((4, 5)).T))
    ro = np.empty((5, 4))
    ro.flags.writeable = False
    call("solve_columns_streamed actinic out read-only", amd.solve_columns_streamed, s5, t5, PHI, out=dict(full(), flux_act_up=ro), actinic=True)
    call("solve_columns_streamed actinic out of a wrong shape", amd.solve_columns_streamed, s5, t5, PHI, out=dict(full(), flux_act_up=np.empty((5, 3))), actinic=True)
    call("solve_columns_streamed view out of a wrong shape", amd.solve_columns_streamed, s5, t5, PHI, out=dict(full(), u0_mu=np.empty((5, 2, 4))), mu=[0.3])
    call("solve_columns_streamed numeric_errors", amd.solve_columns_streamed, s5, t5, PHI, numeric_errors="ignore")
    call("solve_columns_streamed NQuad odd", amd.solve_columns_streamed, dict(s5, NQuad=7), t5, PHI)
    call("solve_columns_streamed NLeg > NQuad", amd.solve_columns_streamed, dict(s5, NLeg=9), t5, PHI)
    call("solve_band_streamed mu of a wrong shape", amd.solve_band_streamed, weights=w, mu=np.zeros((3, 2)), **b)
    call("solve_band_streamed |mu| > 1", amd.solve_band_streamed, weights=w, mu=[-1.5], **b)
    call("solve_band_streamed numeric_errors", amd.solve_band_streamed, weights=w, numeric_errors="ignore", **b)
    call("solve_band_streamed NQuad odd", amd.solve_band_streamed, weights=w, **dict(b, NQuad=7))
    call("solve_band_streamed NFourier > NLeg", amd.solve_band_streamed, weights=w, NLeg=4, NFourier=6, **b)
    call("solve_band_streamed weights of a wrong shape", amd.solve_band_streamed, weights=np.ones(4), **b)


def scenario_unset():
    cfg = small()
    sol = amd.pydisort_batch(**cfg)[1]
    plan = sol.plan
    LIB.fake_trace_take()
    LIB.fake_trace_mark(b"recorded AFTER the front end's fold: before it these calls raised AttributeError or TypeError by accident")
    call("fetch before set_eval_points", plan.fetch)
    call("run_fetch before set_eval_points", plan.run_fetch)
    call("fetch_gathered_results before comm_init", plan.fetch_gathered_results)
    call("fetch_gathered_columns before comm_init", plan.fetch_gathered_columns, 0, 0, 1)
    call("fetch_gathered before comm_init", plan.fetch_gathered)
    call("set_eval_points", plan.set_eval_points, pts(cfg), PHI)
    call("fetch_gathered_results after set_eval_points, before comm_init", plan.fetch_gathered_results)
    call("fetch_gathered after set_eval_points, before comm_init", plan.fetch_gathered)
    call("run()", plan.run)
    call("fetch()", plan.fetch)
    call("fetch_actinic()", plan.fetch_actinic)
    close("plan", plan)
    bsol = amd.pydisort_band(weights=np.array([0.2, 0.5, 0.3]), **band_inputs())[1]
    LIB.fake_trace_take()
    call("fetch_band before set_eval_points", bsol.plan.fetch_band)
    close("band.plan", bsol.plan)


if __name__ == "__main__":
    for k in ("RTD_POOL_BYTES", "RTD_WORK_BYTES", "RTD_NO_PIPELINE", "RTD_RCCL_STUB"):
        assert k not in os.environ, k
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        globals()["scenario_" + sys.argv[1]]()
    gc.collect()
    sys.stdout.write(LIB.fake_trace_take().decode())
    print(f"FRONTEND TRACE {sys.argv[1]} OK")
