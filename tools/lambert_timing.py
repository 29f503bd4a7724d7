#!/usr/bin/env python3
"""What a Lambertian albedo sweep costs against one direct solve per albedo, host arrays in -> host arrays out.

Batch: 10^5 benchmark columns (synthetic.cfg4_columns_block: 20 layers, NQuad = NLeg = 32, all 32 Fourier modes), 8 albedos per
column; wanted: u at tau = 0 with one azimuth, flux_up and the diffuse flux_down there.  Band: P = 6 250 profiles x G = 16 spectral
points of the band of tools/view_timing.py, 8 albedos per profile, K = 1 weight set, the same fields at level 0.

  direct:  eight calls of the streamed form with ``surface=dict(model="lambert", params=A_k)`` -- the path a caller has without the
           sweep: one full solve, all modes, per albedo (solve_columns_streamed / solve_band_streamed);
  sweep:   ``pydisort_batch(..., lambert_sweep=True)`` (``pydisort_band``): the solve over a black surface, the lit-from-below
           companion (one mode), both evaluated at the bottom; then both evaluated at tau = 0 on the device and ONE coupling call
           for the eight albedos (``Plan.evaluate_resident``, ``Plan.couple_lambert`` / ``couple_lambert_band``).  `--retain` names
           the retention form of the two plans (default "lean", with `--retain-bytes`); "none" leaves them unretained, and every
           evaluation then solves the windows again.

Best of `--calls` calls each after a warm-up, the two sides alternating, on one box.  Nothing is gated: the numbers are recorded as
they come, with the largest difference of the two sides over the direct arrays' scale (one scale for the two fluxes) times
(1 - A s) -- the formula's own amplification taken out.  The register counts of the two kernels are read from the code-object metadata (tools/kernel_resources.py).

Usage: python tools/lambert_timing.py [--columns 100000] [--profiles 6250] [--out profiles/lambert.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pythonic-disort_amd"), os.path.join(ROOT, "tools")]
FIELDS = ("u", "flux_up", "flux_down_diffuse")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=100_000)
    ap.add_argument("--profiles", type=int, default=6250)
    ap.add_argument("--gpoints", type=int, default=16)
    ap.add_argument("--albedos", type=int, default=8)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--retain", default="lean", choices=("lean", "full", "none"))
    ap.add_argument("--retain-bytes", type=int, default=64 << 30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lambert.json"))
    a = ap.parse_args()
    import kernel_resources
    import pydisort_amd
    from pydisort_amd import synthetic
    from pydisort_amd.batch import _default_window
    from pydisort_amd.band import level_tau

    C, L, NQ, NA = a.columns, 20, 32, a.albedos
    window = a.window or _default_window(False, None, None, NQ)
    retain = dict(retain=False) if a.retain == "none" else dict(retain=a.retain, retain_bytes=a.retain_bytes)
    rng = np.random.default_rng(11)
    cfg = synthetic.cfg4_columns_block(C, first=0)
    alb = np.sort(rng.uniform(0.0, 1.0, (C, NA)), axis=1)
    phi = np.array([0.0])
    P, G, S = a.profiles, a.gpoints, 3
    k = np.arange(NQ + 1)
    rayleigh = np.zeros(NQ + 1)
    rayleigh[0], rayleigh[2] = 1.0, 0.1
    band = dict(dtau_abs=rng.uniform(0.01, 0.4, (P, G, L)) * 10.0 ** rng.uniform(-1.5, 0.5, (P, G, 1)),
                dtau_spec=rng.uniform(0.01, 0.3, (P, L, S)), omega_spec=rng.uniform(0.6, 0.999, (P, L, S)),
                Leg_spec=np.stack((0.85 ** k, 0.6 ** k, rayleigh)), NQuad=NQ, mu0=rng.uniform(0.2, 0.95, P), I0=rng.uniform(0.5, 2.0, G),
                phi0=rng.uniform(0.0, 2 * np.pi, P))
    w = rng.uniform(0.0, 1.0, G)
    band["weights"] = w / w.sum()
    balb = np.sort(rng.uniform(0.0, 1.0, (P, NA)), axis=1)

    def columns_direct(cfg, alb):
        t0 = time.perf_counter()
        tau = np.zeros((len(alb), 1))
        outs = [pydisort_amd.solve_columns_streamed(dict(cfg, surface=dict(model="lambert", params=alb[:, j:j + 1]), NBDRF=1), tau, phi,
                                                    chunk_columns=window) for j in range(alb.shape[1])]
        res = {f: np.stack([o[f] for o in outs], axis=1) for f in FIELDS}
        return res, time.perf_counter() - t0

    def columns_sweep(cfg, alb):
        t0 = time.perf_counter()
        _, sol = pydisort_amd.pydisort_batch(**cfg, device_prepare=True, work_columns=window, lambert_sweep=True, **retain)
        t1 = time.perf_counter()
        below, t = sol.lit_from_below, sol.lambert_terms()
        tau = np.zeros((len(alb), 1))
        sol.plan.evaluate_resident(tau, phi, keep_u=True)
        below.plan.evaluate_resident(tau)
        res = sol.plan.couple_lambert(below.plan, alb, t["flux_down_bottom"], t["spherical_albedo"], want=("u", "flux"))
        form = (sol.plan.retained_form(), sol.plan.windows()[1])
        sol.plan.close()
        below.plan.close()
        t2 = time.perf_counter()
        return res, dict(total=t2 - t0, solves_and_terms=t1 - t0, evaluate_and_couple=t2 - t1), t["spherical_albedo"], form

    def band_direct(bkw, alb):
        t0 = time.perf_counter()
        outs = [pydisort_amd.solve_band_streamed(**bkw, levels=[0], phi=phi, chunk_columns=window, surface=dict(model="lambert", params=alb[:, j:j + 1]),
                                                 NBDRF=1) for j in range(alb.shape[1])]
        res = {f: np.stack([o[f] for o in outs], axis=1) for f in FIELDS}
        return res, time.perf_counter() - t0

    def band_sweep(bkw, alb):
        t0 = time.perf_counter()
        _, bsol = pydisort_amd.pydisort_band(**bkw, work_columns=window, lambert_sweep=True, **retain)
        t1 = time.perf_counter()
        plan, below, t = bsol.plan, bsol.columns.lit_from_below.plan, bsol.columns.lambert_terms()
        tau = level_tau(plan.prep["tau"], [0])
        plan.evaluate_resident(tau, phi, keep_u=True)
        below.evaluate_resident(tau)
        res = plan.couple_lambert_band(below, alb, t["flux_down_bottom"], t["spherical_albedo"], want=("u", "flux"))
        res = {f: res[f][:, 0] for f in FIELDS}  # (K = 1)
        plan.close()
        below.close()
        t2 = time.perf_counter()
        return res, dict(total=t2 - t0, solves_and_terms=t1 - t0, evaluate_and_couple=t2 - t1), t["spherical_albedo"]

    def distance(got, want, amp):
        """max |got - want| (1 - A s) over the scale of `want`, per field; amp [rows, A] = 1 - A s.  The two fluxes share one scale, the
        larger of theirs: at tau = 0 the diffuse downward flux is the top boundary's, zero or rounding noise for these inputs."""
        out = {}
        flux_scale = max(np.max(np.abs(want["flux_up"])), np.max(np.abs(want["flux_down_diffuse"])))
        for f in FIELDS:
            d = np.abs(got[f] - want[f]) * amp.reshape(amp.shape + (1,) * (want[f].ndim - 2))
            out[f] = float(np.max(d) / (np.max(np.abs(want[f])) if f == "u" else flux_scale))
        return out

    def rounded(t):
        return {kk: round(v, 4) for kk, v in t.items()}

    # warm-up: a small batch and a small band through every path
    scfg = {kk: (v[:512] if isinstance(v, np.ndarray) else v) for kk, v in cfg.items()}
    sband = {kk: (v[:32] if isinstance(v, np.ndarray) and v.shape[:1] == (P,) else v) for kk, v in band.items()}
    columns_direct(scfg, alb[:512, :2])
    columns_sweep(scfg, alb[:512])
    band_direct(sband, balb[:32, :2])
    band_sweep(sband, balb[:32])

    ks = kernel_resources.kernels_of(os.path.join(ROOT, "pythonic-disort_amd", "pydisort_amd", "librtd.so"))
    out = dict(
        what="Lambertian albedo sweep against one direct solve per albedo, host arrays in, host arrays out, seconds: u at tau = 0 with one "
             "azimuth, flux_up and the diffuse flux_down there; direct = eight streamed solves with surface=lambert; sweep = the black "
             "solve, the one-mode companion, their evaluation at the bottom, one evaluation of both at tau = 0 and one coupling call; best "
             "of the calls listed, the two sides alternating, after a warm-up; no threshold set",
        columns=C, profiles=P, gpoints=G, layers=L, nquad=NQ, albedos=NA, window=window, retain=a.retain, retain_bytes=a.retain_bytes,
        kernels={n: r for n, r in ks.items() if "rtd_lambert" in n})
    with pydisort_amd.pooled():
        td, ts = [], []
        columns_sweep(cfg, alb)  # (one full-size call: the pool holds the blocks of this size from here on)
        for _ in range(a.calls):
            rd, t = columns_direct(cfg, alb)
            td.append(t)
            rs, t, s, form = columns_sweep(cfg, alb)
            ts.append(t)
        best = min(ts, key=lambda v: v["total"])
        out["batch"] = dict(direct_seconds_per_call=[round(v, 4) for v in td], sweep_seconds_per_call=[rounded(v) for v in ts],
                              direct_seconds=round(min(td), 4), sweep_seconds=round(best["total"], 4), sweep_parts=rounded(best),
                              direct_over_sweep=round(min(td) / best["total"], 3), retained_form=form[0], windows=form[1],
                              difference_over_scale_times_1_minus_As=distance(rs, rd, 1.0 - alb * s[:, None]))
        print("batch", json.dumps(out["batch"]), flush=True)
        del rd, rs
        td, ts = [], []
        band_sweep(band, balb)
        for _ in range(a.calls):
            rd, t = band_direct(band, balb)
            td.append(t)
            rs, t, s = band_sweep(band, balb)
            ts.append(t)
        best = min(ts, key=lambda v: v["total"])
        smax = s.reshape(P, G).max(axis=1)  # (a band result mixes the points: the largest amplification of the profile)
        out["band"] = dict(direct_seconds_per_call=[round(v, 4) for v in td], sweep_seconds_per_call=[rounded(v) for v in ts],
                           direct_seconds=round(min(td), 4), sweep_seconds=round(best["total"], 4), sweep_parts=rounded(best),
                           direct_over_sweep=round(min(td) / best["total"], 3),
                           difference_over_scale_times_1_minus_As=distance(rs, rd, 1.0 - balb * smax[:, None]))
        print("band", json.dumps(out["band"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
