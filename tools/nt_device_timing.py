#!/usr/bin/env python3
"""What the Nakajima-Tanaka corrections cost when the device forms their inputs (rtd_plan_request_nt).

  (a) a k-distribution band of P = 6 250 profiles x G = 16 spectral points = 10^5 columns, S = 3 species with `--moments` Legendre
      coefficients each, 20 layers, 32 streams, results at 21 levels x 3 azimuths: pydisort_amd.solve_band_streamed with and
      without NT_cor.  The difference is the corrections: the weighted phase function of P profiles, the IMS constants of P G
      columns and above all rtd_nt_apply_kernel's Legendre series at every (column, level, stream, azimuth).
  (b) `--columns` = 10^4 columns with `--moments` = 128 moments per layer, whose host arrays fit comfortably: the host-prepared
      pydisort_batch(NT_cor=True) (NumPy preparation, _nt.nt_inputs, upload, solve, u at the levels) against
      solve_columns_streamed with NT_cor in cfg (everything formed on the device); both host arrays in -> host array u out.

Best of two alternating calls after a warm-up.  No threshold: the figures are recorded as they come.

Usage: python tools/nt_device_timing.py [--profiles 6250] [--columns 10000] [--out profiles/nt_device.json]
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
    ap.add_argument("--profiles", type=int, default=6250)
    ap.add_argument("--gpoints", type=int, default=16)
    ap.add_argument("--columns", type=int, default=10000)
    ap.add_argument("--moments", type=int, default=128)
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nt_device.json"))
    a = ap.parse_args()
    import pydisort_amd

    S, L, NQ, nall = 3, 20, 32, a.moments
    rng = np.random.default_rng(12)
    k = np.arange(nall)
    rayleigh = np.zeros(nall)
    rayleigh[0], rayleigh[2] = 1.0, 0.1
    leg_spec = np.stack((0.85 ** k, 0.6 ** k, rayleigh))
    phi = np.array([0.0, np.pi / 2, np.pi])

    def band_inputs(P, G):
        w = rng.uniform(0.0, 1.0, G)
        return dict(dtau_abs=rng.uniform(0.01, 0.4, (P, G, L)) * 10.0 ** rng.uniform(-1.5, 0.5, (P, G, 1)),
                    dtau_spec=rng.uniform(0.01, 0.3, (P, L, S)), omega_spec=rng.uniform(0.6, 0.999, (P, L, S)), Leg_spec=leg_spec,
                    NQuad=NQ, mu0=rng.uniform(0.2, 0.95, P), I0=rng.uniform(0.5, 2.0, G), phi0=rng.uniform(0.0, 2 * np.pi, P),
                    weights=w / w.sum(), phi=phi, chunk_columns=a.window)

    def columns(C):
        g = rng.uniform(0.6, 0.9, (C, L, 1))
        leg = g ** k[None, None, :]
        return dict(tau_arr=np.cumsum(rng.uniform(0.02, 0.5, (C, L)), axis=1), omega_arr=rng.uniform(0.6, 0.999, (C, L)), NQuad=NQ,
                    Leg_coeffs_all=leg, f_arr=leg[:, :, NQ].copy(), mu0=rng.uniform(0.2, 0.95, C), I0=rng.uniform(0.5, 2.0, C),
                    phi0=rng.uniform(0.0, 2 * np.pi, C), NT_cor=True)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def band_call(kw, nt):
        return lambda: pydisort_amd.solve_band_streamed(**kw, NT_cor=nt)["u"]

    def host_call(cfg, tau):
        def run():
            # the plan driven as solve_columns_streamed drives its own: one pass of the window pipeline, no second solve
            _, sol = pydisort_amd.pydisort_batch(work_columns=a.window, _defer_solve=True, **cfg)
            sol.plan.set_eval_points(tau, phi)
            u = sol.plan.run_fetch()["u"]
            sol.plan.close()
            return u
        return run

    def device_call(cfg, tau):
        return lambda: pydisort_amd.solve_columns_streamed(cfg, tau, phi, chunk_columns=a.window)["u"]

    def best_of_two(f, g):
        tf, tg, rf, rg = [], [], None, None
        for _ in range(2):  # alternating
            t, rf = timed(f)
            tf.append(t)
            t, rg = timed(g)
            tg.append(t)
        return tf, tg, rf, rg

    small, cs = band_inputs(32, a.gpoints), columns(256)
    ts = np.concatenate((np.zeros((256, 1)), cs["tau_arr"]), axis=1)
    for warm in (band_call(small, True), band_call(small, False), host_call(cs, ts), device_call(cs, ts)):
        warm()
    with pydisort_amd.pooled():
        kw = band_inputs(a.profiles, a.gpoints)
        t_on, t_off, u_on, u_off = best_of_two(band_call(kw, True), band_call(kw, False))
        band_effect = float(np.max(np.abs(u_on - u_off)) / np.max(np.abs(u_off)))
        del u_on, u_off
        cfg = columns(a.columns)
        tau = np.concatenate((np.zeros((a.columns, 1)), cfg["tau_arr"]), axis=1)
        t_host, t_dev, u_host, u_dev = best_of_two(host_call(cfg, tau), device_call(cfg, tau))
        t0 = time.perf_counter()
        from pydisort_amd import _nt
        _nt.nt_inputs(dict(tau=cfg["tau_arr"], I0=np.ones(a.columns)), cfg["omega_arr"], cfg["f_arr"], cfg["Leg_coeffs_all"], NQ, cfg["mu0"])
        t_inputs = time.perf_counter() - t0
        diff = float(np.max(np.abs(u_host - u_dev)) / np.max(np.abs(u_host)))
    out = dict(
        what="Nakajima-Tanaka corrections with device-formed inputs, seconds, host arrays in -> host arrays out, best of two alternating "
             "calls after a warm-up.  (a) solve_band_streamed of P profiles x G spectral points (S = 3 species, 20 layers, 32 streams, 21 "
             "levels x 3 azimuths) with and without NT_cor; (b) host-prepared pydisort_batch(NT_cor=True) + u at the levels against "
             "solve_columns_streamed with NT_cor",
        moments=nall, layers=L, nquad=NQ, window=a.window,
        a_profiles=a.profiles, a_gpoints=a.gpoints, a_columns=a.profiles * a.gpoints,
        a_with_nt_seconds_per_call=[round(t, 4) for t in t_on], a_without_nt_seconds_per_call=[round(t, 4) for t in t_off],
        a_with_nt_seconds=round(min(t_on), 4), a_without_nt_seconds=round(min(t_off), 4),
        a_correction_over_u_scale=band_effect,
        b_columns=a.columns, b_host_prepared_seconds_per_call=[round(t, 4) for t in t_host],
        b_device_seconds_per_call=[round(t, 4) for t in t_dev], b_host_prepared_seconds=round(min(t_host), 4),
        b_device_seconds=round(min(t_dev), 4), b_host_nt_inputs_alone_seconds=round(t_inputs, 4), b_u_difference_over_scale=diff)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
