#!/usr/bin/env python3
"""Where the thermal sources of a throughput batch are formed: on the host (the reference's way) or on the device.

Batch: C = 10^5 cfg4 columns (20 layers, 32 streams; pydisort_amd.synthetic.cfg4_columns_block), a temperature per level
(2.1 M), bottom and top boundary temperatures per column, one shared band 300 ... 800 cm^-1.  Two paths, host arrays in ->
host arrays out (pydisort_amd.solve_columns_streamed, the end-to-end form of bench.py):

  (a) host:   s_poly_coeffs, b_pos, b_neg from pydisort_amd.subroutines (blackbody_contrib_to_BCs = scipy.integrate.quad_vec over
              all temperatures at once -- possible only because the band is shared -- and the linear spline in NumPy), then the
              batch with those arrays (device_prepare=True);
  (b) device: the batch with thermal=dict(TEMPER, WVNMLO, WVNMHI, BTEMP, TTEMP).

The BUILD of the sources is timed apart from the SOLVE: for (a) it is the host helpers; for (b) it happens inside the call, so it
is reported twice -- as the difference of the two calls' times, and stand-alone as pydisort_amd.planck_band over the same
2.3 M temperatures, host to host.  Also reported: the largest difference of the two paths' fluxes over their scale.

Usage: python tools/thermal_prepare_timing.py [--columns 100000] [--out profiles/thermal_prepare.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pythonic-disort_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=100_000)
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thermal_prepare.json"))
    a = ap.parse_args()
    import pydisort_amd
    from pydisort_amd import subroutines as S, synthetic

    C, L, NQ, lo, hi = a.columns, 20, 32, 300.0, 800.0
    cfg = synthetic.cfg4_columns_block(C, first=0)
    rng = np.random.default_rng(7)
    temper = np.sort(rng.uniform(200.0, 300.0, (C, L + 1)), axis=1)
    btemp, ttemp = rng.uniform(280.0, 320.0, C), rng.uniform(50.0, 120.0, C)
    tau = np.concatenate((np.zeros((C, 1)), cfg["tau_arr"]), axis=1)
    phi = np.array([0.0, np.pi / 2, np.pi])

    def run(extra, n):
        times, res = [], None
        with pydisort_amd.pooled():
            for _ in range(n):
                t0 = time.perf_counter()
                res = pydisort_amd.solve_columns_streamed(dict(cfg, **extra), tau, phi, chunk_columns=a.window)
                times.append(time.perf_counter() - t0)
        return times, res

    # (a) build on the host
    t0 = time.perf_counter()
    E = S.blackbody_contrib_to_BCs(np.concatenate((temper.ravel(), btemp, ttemp)), lo, hi)
    t_quad = time.perf_counter() - t0
    t0 = time.perf_counter()
    Elev = E[:C * (L + 1)].reshape(C, L + 1)
    x = tau
    slope = np.diff(Elev, axis=1) / np.diff(x, axis=1)
    s_poly = np.stack((Elev[:, :-1] - slope * x[:, :-1], slope), axis=2)
    b_pos, b_neg = E[C * (L + 1):C * (L + 1) + C], E[C * (L + 1) + C:]
    t_spline = time.perf_counter() - t0
    host = dict(s_poly_coeffs=s_poly, b_pos=b_pos, b_neg=b_neg)
    thermal = dict(thermal=dict(TEMPER=temper, WVNMLO=lo, WVNMHI=hi, BTEMP=btemp, TTEMP=ttemp))

    nw = min(C, 2 * a.window)
    small = {k: (v[:nw] if isinstance(v, np.ndarray) and v.shape[:1] == (C,) else v) for k, v in cfg.items()}
    pydisort_amd.solve_columns_streamed(dict(small, s_poly_coeffs=s_poly[:nw], b_pos=b_pos[:nw], b_neg=b_neg[:nw]), tau[:nw], phi,
                                        chunk_columns=a.window)  # warm-up
    ta, ra = run(host, a.calls)
    fa = {k: ra[k].copy() for k in ("flux_up", "flux_down_diffuse")}
    del ra
    tb, rb = run(thermal, a.calls)
    diff = max(float(np.max(np.abs(rb[k] - fa[k])) / np.max(np.abs(fa[k]))) for k in fa)

    # the device build alone, host to host
    temps = np.concatenate((temper.ravel(), btemp, ttemp))
    pydisort_amd.planck_band(temps[:1000], lo, hi)
    tp = []
    for _ in range(3):
        t0 = time.perf_counter()
        Ed = pydisort_amd.planck_band(temps, lo, hi)
        tp.append(time.perf_counter() - t0)
    out = dict(
        what="thermal sources of a 10^5-column cfg4 batch (20 layers, 32 streams, 2.1 M level temperatures + 2 boundary temperatures per "
             "column, shared band 300-800 cm^-1): built on the host by the SciPy helpers (a) or on the device (b); solve = "
             "solve_columns_streamed host to host, seconds",
        columns=C, layers=L, nquad=NQ, integrals=int(temps.size),
        a_host_build_seconds=dict(quad_vec=round(t_quad, 4), spline=round(t_spline, 4)),
        a_solve_seconds_per_call=[round(t, 4) for t in ta],
        b_thermal_call_seconds_per_call=[round(t, 4) for t in tb],
        b_build_inside_call_seconds=round(min(tb) - min(ta), 4),
        b_planck_band_alone_seconds_per_call=[round(t, 4) for t in tp],
        a_total_seconds=round(t_quad + t_spline + min(ta), 4), b_total_seconds=round(min(tb), 4),
        flux_difference_over_scale=diff,
        planck_band_vs_host_quadrature_max_rel=float(np.max(np.abs(Ed - E) / E)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
