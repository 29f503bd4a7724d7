#!/usr/bin/env python3
"""Driver of tests/test_nt_view_frontend_cpu.py: the `corrections=` keyword of the Python front end over the real host code of
csrc/rtd_api.hip, the stand-in runtime of tests/cpu/fake_hip and the shadow launchers, as the plain shared library that RTD_LIB names
(tests/host_program.py: build_trace_library).  Values are the shadow launchers' constants; what is printed, one line per step, is
shapes, finiteness and the exceptions with their messages.

Usage: RTD_LIB=<library> FAKE_HIP_TOTAL=<bytes> python tests/cpu/nt_view_frontend_driver.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path += [ROOT, os.path.join(ROOT, "pythonic-disort_amd")]
import pydisort_amd as amd  # noqa: E402
from pydisort_amd import synthetic  # noqa: E402

PHI = np.array([0.0, 1.0])
MU = np.array([0.3, -0.5, 1.0, -1.0])


def step(label, fn, *a, **k):
    try:
        r = fn(*a, **k)
        if isinstance(r, dict):
            r = {key: v for key, v in r.items() if v is not None}
            print(label, "->", " ".join(f"{key}{tuple(v.shape)}{'' if np.all(np.isfinite(v)) else ' NONFINITE'}" for key, v in sorted(r.items())))
        elif isinstance(r, np.ndarray):
            print(label, "->", tuple(r.shape), "finite" if np.all(np.isfinite(r)) else "NONFINITE")
        else:
            print(label, "->", type(r).__name__)
        return r
    except Exception as e:  # noqa: BLE001
        print(label, "raises", type(e).__name__ + ":", e)


def main():
    C = 6
    cfg = synthetic.cfg4_columns(C, L=3, NQuad=8)
    nall = cfg["Leg_coeffs_all"].shape[2]
    assert nall > 8
    kw = dict(cfg, f_arr=cfg["Leg_coeffs_all"][:, :, 8].copy(), NT_cor=True)
    tau = cfg["tau_arr"][:, -1:] * np.array([0.0, 0.4, 1.0])[None, :]
    for extra in (dict(device_prepare=True), dict(work_columns=4, device_prepare=True, retain=False)):
        _, sol = amd.pydisort_batch(**kw, **extra)
        plan = sol.plan
        print("windows", plan.windows())
        for order in (dict(), dict(is_antiderivative_wrt_tau=True), dict(is_derivative_wrt_tau=True)):
            step(f"u_at at_angles {sorted(order)}", sol.u_at, MU, tau, PHI, corrections="at_angles", **order)
        step("u_at per column", sol.u_at, np.tile(MU, (C, 1)), tau, PHI, corrections="at_angles")
        step("u_at interpolated takes mu = 0", sol.u_at, np.array([0.0, 0.5]), tau, PHI, corrections="interpolated")
        step("u_at default", sol.u_at, MU, tau, PHI)
        step("u_at unknown", sol.u_at, MU, tau, PHI, corrections="exact")
        step("u_at at_angles mu = 0", sol.u_at, np.array([0.5, -0.0]), tau, PHI, corrections="at_angles")
        step("u_at positional", sol.u_at, MU, tau, PHI, False, "at_angles")
        step("u0_at", sol.u0_at, MU, tau)
        # a request made after the evaluation
        step("evaluate", plan.evaluate, tau, PHI, want=("u",))
        step("set_view at_angles after the evaluation", plan.set_view, MU, corrections="at_angles")
        step("fetch_view u", plan.fetch_view, ("u",))
        step("fetch_view u0", plan.fetch_view, ("u0",))
        step("evaluate view", plan.evaluate, tau, PHI, want=("view_u",))
        step("set_view None", plan.set_view, None)
        plan.close()
    out = step("streamed at_angles", amd.solve_columns_streamed, kw, tau, PHI, chunk_columns=4, mu=MU, view_corrections="at_angles")
    assert out is not None and "u_mu" in out
    step("streamed unknown", amd.solve_columns_streamed, kw, tau, PHI, mu=MU, view_corrections="no")
    step("streamed mu = 0", amd.solve_columns_streamed, kw, tau, PHI, mu=np.array([0.0]), view_corrections="at_angles")
    print("NT VIEW FRONTEND DONE")


if __name__ == "__main__":
    main()
