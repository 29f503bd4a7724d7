#!/usr/bin/env python3
"""Driver of tests/test_lambert_frontend_cpu.py: ``lambert_sweep=True`` of the Python front end over the real host code of
csrc/rtd_api.hip, the stand-in runtime of tests/cpu/fake_hip and the shadow launchers, as the plain shared library that RTD_LIB names
(tests/host_program.py: build_trace_library).  Values are the shadow launchers' constants; what is printed, one line per step, is
shapes, finiteness, the exceptions with their messages, and -- from the library's call trace -- which kernels of the sweep each step
launched.

Usage: RTD_LIB=<library> FAKE_HIP_TOTAL=<bytes> python tests/cpu/lambert_frontend_driver.py"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path += [ROOT, os.path.join(ROOT, "pythonic-disort_amd")]
import pydisort_amd as amd  # noqa: E402
from pydisort_amd import _lib, synthetic  # noqa: E402

PHI = np.array([0.0, 1.0])
MU = np.array([0.3, -0.5, 1.0])
ALB = np.array([0.0, 0.3, 0.95, 1.0])


def trace():
    """The library's call trace since the last look -> (launches of the sweep's kernels, launches of any other kernel, solves)."""
    take = _lib.load().fake_trace_take
    take.restype = ctypes.c_char_p
    lines = take().decode().splitlines()
    launches = [line.split()[1] for line in lines if line.startswith("launch ")]
    mine = [k for k in launches if "lambert" in k]
    return (f"kappa {sum('kappa' in k for k in mine)} couple {sum('couple' in k for k in mine)} reduce {launches.count('rtd_band_reduce_kernel')} "
            f"solves {sum(line.startswith('bc ') or line.startswith('bc_small ') for line in lines)}")


def step(label, fn, *a, **k):
    trace()
    try:
        r = fn(*a, **k)
        if isinstance(r, tuple) and all(isinstance(v, np.ndarray) for v in r):
            print(label, "->", " ".join(f"{tuple(v.shape)}{'' if np.all(np.isfinite(v)) else ' NONFINITE'}" for v in r), "|", trace())
        elif isinstance(r, dict):
            r = {key: v for key, v in r.items() if v is not None}
            print(label, "->", " ".join(f"{key}{tuple(v.shape)}{'' if np.all(np.isfinite(v)) else ' NONFINITE'}" for key, v in sorted(r.items())), "|", trace())
        elif isinstance(r, np.ndarray):
            print(label, "->", tuple(r.shape), "finite" if np.all(np.isfinite(r)) else "NONFINITE", "|", trace())
        else:
            print(label, "->", type(r).__name__, "|", trace())
        return r
    except Exception as e:  # noqa: BLE001
        print(label, "raises", type(e).__name__ + ":", e)


def main():
    C = 6
    cfg = synthetic.cfg4_columns(C, L=3, NQuad=8)
    kw = dict(cfg, f_arr=cfg["Leg_coeffs_all"][:, :, 8].copy(), NT_cor=True, device_prepare=True)
    tau = cfg["tau_arr"][:, -1:] * np.array([0.0, 0.4, 1.0])[None, :]
    # a batch that never asks: nothing of the sweep is launched
    _, plain = amd.pydisort_batch(**kw)
    step("plain u", plain.u, tau, PHI)
    step("plain lambert", plain.lambert, ALB)
    step("plain lambert_terms", plain.lambert_terms)
    plain.plan.close()
    for extra in (dict(), dict(work_columns=4, retain="full")):
        trace()
        _, sol = amd.pydisort_batch(**kw, **extra, lambert_sweep=True)
        print("made", trace())
        below = sol.lit_from_below
        print("windows", sol.plan.windows(), below.plan.windows(), "retained", sol.plan.retained_form(), below.plan.retained_form())
        print("companion", below.plan.M, below.plan.prep["beam"], below.plan.prep["Ns"], below.plan.prep["NBDRF"], below.plan.prep["raw"]["leg"].shape)
        step("lambert_terms", sol.lambert_terms)
        sw = step("lambert", sol.lambert, ALB)
        print("kappa", sw.kappa.shape, sw.kappa_flag.shape)
        step("u", sw.u, tau, PHI)
        for order in (dict(is_antiderivative_wrt_tau=True), dict(is_derivative_wrt_tau=True)):
            step(f"u0 {sorted(order)}", sw.u0, tau, **order)
        step("u both orders", sw.u, tau, PHI, True, is_derivative_wrt_tau=True)
        step("flux_up", sw.flux_up, tau)
        step("flux_down", sw.flux_down, tau)
        step("u_at", sw.u_at, MU, tau, PHI)
        step("u_at at_angles", sw.u_at, MU, tau, PHI, corrections="at_angles")
        step("u0_at per column", sw.u0_at, np.tile(MU, (C, 1)), tau)
        step("below u0_at", below.u0_at, MU, np.zeros(1))
        step("tau out of range", sw.u0, tau + 100.0)
        per = step("lambert per column", sol.lambert, np.tile(ALB, (C, 1)) * np.linspace(0.5, 1.0, C)[:, None], emission=np.linspace(0.0, 2.0, C))
        step("per column flux_up", per.flux_up, tau)
        step("lambert scalar emission", sol.lambert, ALB, emission=1.7)
        step("lambert bad albedo", lambda: sol.lambert(np.array([0.2, 1.5])).u0(tau))
        step("lambert bad rows", lambda: sol.lambert(np.zeros((C + 1, 2))).u0(tau))
        step("lambert bad emission", lambda: sol.lambert(ALB, emission=-1.0).u0(tau))
        step("lambert BTEMP without thermal", sol.lambert, ALB, BTEMP=300.0)
        # the plan level: the companion must be a plan of the same shape; want names what is formed
        sol.plan.evaluate_resident(tau, PHI, keep_u=True)
        below.plan.evaluate_resident(tau)
        t = sol.lambert_terms()
        step("Plan.couple_lambert", sol.plan.couple_lambert, below.plan, ALB, t["flux_down_bottom"], t["spherical_albedo"], want=("u", "flux"))
        step("Plan.couple_lambert itself", sol.plan.couple_lambert, sol.plan, ALB, t["flux_down_bottom"], t["spherical_albedo"])
        step("Plan.couple_lambert_band without weights", sol.plan.couple_lambert_band, below.plan, ALB, t["flux_down_bottom"], t["spherical_albedo"])
        sol.plan.close()
        below.plan.close()
    # thermal: the band of thermal= serves BTEMP
    th = dict(TEMPER=np.linspace(220.0, 290.0, 4), WVNMLO=600.0, WVNMHI=700.0)
    kwt = {k: v for k, v in kw.items() if k not in ("NT_cor",)}
    _, sol = amd.pydisort_batch(**kwt, thermal=th, lambert_sweep=True)
    sw = step("thermal lambert BTEMP", sol.lambert, ALB, BTEMP=300.0)
    print("emission", None if sw is None else np.shape(sw.emission))
    step("thermal flux_up", sw.flux_up, tau)
    step("emission and BTEMP", sol.lambert, ALB, emission=1.0, BTEMP=300.0)
    sol.plan.close()
    sol.lit_from_below.plan.close()
    # a band
    rng = np.random.default_rng(11)
    P, G, S, L = 2, 3, 2, 3
    bkw = dict(dtau_abs=rng.uniform(0.01, 0.5, (P, G, L)), dtau_spec=rng.uniform(0.05, 0.4, (P, L, S)), omega_spec=rng.uniform(0.1, 0.95, (P, L, S)),
               Leg_spec=np.array([0.7, 0.3])[:, None] ** np.arange(11)[None, :], NQuad=8, mu0=0.6, I0=1.0, phi0=0.0, weights=np.full((2, G), 0.2))
    trace()
    _, band = amd.pydisort_band(**bkw, lambert_sweep=True)
    print("band made", trace())
    step("band lambert_terms", band.lambert_terms)
    for label, alb in (("[A]", ALB), ("[P, A]", np.tile(ALB, (P, 1))), ("[P, G, A]", np.tile(ALB, (P, G, 1)) * 0.9)):
        bs = step(f"band lambert {label}", band.lambert, alb)
        print("band kappa", bs.kappa.shape)
        step(f"band flux_up {label}", bs.flux_up)
        step(f"band u {label}", bs.u, [0, 3], PHI)
    step("band flux_down", bs.flux_down, [0, 1, 3])
    step("band u_at", bs.u_at, MU, [0, 3], PHI)
    step("band u0_at per profile", bs.u0_at, np.tile(MU, (P, 1)))
    step("band lambert bad shape", band.lambert, np.zeros((P + 1, 2)))
    step("band lambert bad spectral shape", band.lambert, np.zeros((P, G + 1, 2)))
    band.plan.close()
    band.columns.lit_from_below.plan.close()
    print("LAMBERT FRONTEND DONE")


if __name__ == "__main__":
    main()
