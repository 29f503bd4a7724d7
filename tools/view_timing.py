#!/usr/bin/env python3
"""What radiances at user polar angles cost, host arrays in -> host arrays out.

Batch: 10^5 benchmark columns (synthetic.cfg4_columns_block: 20 layers, NQuad = NLeg = 32, all Fourier modes); band: P = 6 250
profiles x G = 16 spectral points of the band of tools/actinic_timing.py, all Fourier modes, K = 1 weight set.  Two requests:
  "toa":  one angle at tau = 0 (level 0) with one azimuth;
  "grid": 3 angles x the L + 1 = 21 levels x 3 azimuths.

  (a) columns: pydisort_amd.solve_columns_streamed with u [C, 32, ntau, nphi] fetched and the arithmetic of
      subroutines.interpolate on the host -- scipy.interpolate.BarycentricInterpolator, one column at a time, each hemisphere on
      its own -- against the mu= form with u left on the device (`out` without "u");
  (b) band: solve_band_streamed, whose reduced u [P, K, 32, nlev, nphi] is what a caller can interpolate today, and the same SciPy
      loop over the P profiles, against mu=.  (Interpolation and the spectral sum are both linear, so the two orders agree.)

Best of `--calls` calls each after a warm-up, the two sides of a comparison alternating, on one box.  Nothing is gated: the numbers
are recorded as they come, with the largest difference of the two sides over the arrays' scale.

Usage: python tools/view_timing.py [--columns 100000] [--profiles 6250] [--out profiles/view.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pythonic-disort_amd"))


def host_interpolate(x, mu, u):
    """u [R, 2N, ...] -> [R, nmu, ...]: the reference's interpolate, row by row."""
    import scipy.interpolate
    N = len(x)
    up, dn = scipy.interpolate.BarycentricInterpolator(x), scipy.interpolate.BarycentricInterpolator(-x)
    pos = mu > 0
    out = np.empty((u.shape[0], len(mu)) + u.shape[2:])
    for r in range(u.shape[0]):
        if np.any(pos):
            up.set_yi(u[r, :N])
            out[r, pos] = up(mu[pos])
        if np.any(~pos):
            dn.set_yi(u[r, N:])
            out[r, ~pos] = dn(mu[~pos])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=100_000)
    ap.add_argument("--profiles", type=int, default=6250)
    ap.add_argument("--gpoints", type=int, default=16)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view.json"))
    a = ap.parse_args()
    import pydisort_amd
    from pydisort_amd import synthetic
    from pydisort_amd._prepare import double_gauss
    from pydisort_amd.band import level_tau

    C, L, NQ = a.columns, 20, 32
    x = np.asarray(double_gauss(NQ // 2)[0], float)
    cfg = synthetic.cfg4_columns_block(C, first=0)
    requests = {"toa": (np.array([0.8]), [0], np.array([0.0])),
                "grid": (np.array([0.8, 0.35, -0.6]), list(range(L + 1)), np.array([0.0, 1.0, np.pi]))}
    P, G, S = a.profiles, a.gpoints, 3
    rng = np.random.default_rng(11)
    k = np.arange(NQ + 1)
    rayleigh = np.zeros(NQ + 1)
    rayleigh[0], rayleigh[2] = 1.0, 0.1
    band = dict(dtau_abs=rng.uniform(0.01, 0.4, (P, G, L)) * 10.0 ** rng.uniform(-1.5, 0.5, (P, G, 1)),
                dtau_spec=rng.uniform(0.01, 0.3, (P, L, S)), omega_spec=rng.uniform(0.6, 0.999, (P, L, S)),
                Leg_spec=np.stack((0.85 ** k, 0.6 ** k, rayleigh)), NQuad=NQ, mu0=rng.uniform(0.2, 0.95, P), I0=rng.uniform(0.5, 2.0, G),
                phi0=rng.uniform(0.0, 2 * np.pi, P))
    w = rng.uniform(0.0, 1.0, G)
    band["weights"] = w / w.sum()

    def columns_host(cfg, tau, mu, phi):
        t0 = time.perf_counter()
        res = pydisort_amd.solve_columns_streamed(cfg, tau, phi, chunk_columns=a.window)
        t1 = time.perf_counter()
        out = host_interpolate(x, mu, res["u"])
        t2 = time.perf_counter()
        return out, dict(solve_and_fetch=t1 - t0, scipy=t2 - t1, total=t2 - t0)

    def columns_device(cfg, tau, mu, phi, keep):
        t0 = time.perf_counter()
        out = pydisort_amd.solve_columns_streamed(cfg, tau, phi, chunk_columns=a.window, mu=mu, out=keep)
        return out["u_mu"], dict(total=time.perf_counter() - t0)

    def band_host(bkw, mu, lev, phi):
        t0 = time.perf_counter()
        res = pydisort_amd.solve_band_streamed(**bkw, levels=lev, phi=phi, chunk_columns=a.window)
        t1 = time.perf_counter()
        out = host_interpolate(x, mu, res["u"])
        t2 = time.perf_counter()
        return out, dict(solve_and_fetch=t1 - t0, scipy=t2 - t1, total=t2 - t0)

    def band_device(bkw, mu, lev, phi):
        t0 = time.perf_counter()
        out = pydisort_amd.solve_band_streamed(**bkw, levels=lev, phi=phi, chunk_columns=a.window, mu=mu)
        return out["u_mu"], dict(total=time.perf_counter() - t0)

    def keep_arrays(n, nmu, nt):
        keep = {kk: np.empty((n, nt)) for kk in ("flux_up", "flux_down_diffuse", "flux_down_direct")}
        keep.update(u0=np.empty((n, NQ, nt)), u0_mu=np.empty((n, nmu, nt)))
        return keep

    def rounded(t):
        return {kk: round(v, 4) for kk, v in t.items()}

    # warm-up: a small batch and a small band through every path
    scfg = {kk: (v[:512] if isinstance(v, np.ndarray) else v) for kk, v in cfg.items()}
    sband = {kk: (v[:32] if isinstance(v, np.ndarray) and v.shape[:1] == (P,) else v) for kk, v in band.items()}
    for mu, lev, phi in requests.values():
        tau = level_tau(scfg["tau_arr"], lev)
        columns_host(scfg, tau, mu, phi)
        columns_device(scfg, tau, mu, phi, keep_arrays(512, len(mu), len(lev)))
        band_host(sband, mu, lev, phi)
        band_device(sband, mu, lev, phi)

    out = dict(
        what="radiances at user polar angles, host arrays in, host arrays out, seconds: (a) solve_columns_streamed of the benchmark "
             "columns (20 layers, 32 streams, all modes) with u fetched and scipy's BarycentricInterpolator per column and hemisphere "
             "on the host, against mu= with u left on the device; (b) solve_band_streamed with the reduced u interpolated per profile "
             "on the host, against mu=; toa: one angle, tau = 0, one azimuth; grid: 3 angles x 21 levels x 3 azimuths; best of the "
             "calls listed, the two sides alternating, after a warm-up; no threshold set",
        columns=C, profiles=P, gpoints=G, layers=L, nquad=NQ, window=a.window)
    with pydisort_amd.pooled():
        for name, (mu, lev, phi) in requests.items():
            tau = level_tau(cfg["tau_arr"], lev)
            keep = keep_arrays(C, len(mu), len(lev))
            th, td, bh, bd = [], [], [], []
            columns_device(cfg, tau, mu, phi, keep)  # (one full-size call: the pool holds the blocks of this size from here on)
            for _ in range(a.calls):
                rh, t = columns_host(cfg, tau, mu, phi)
                th.append(t)
                rd, t = columns_device(cfg, tau, mu, phi, keep)
                td.append(t)
            diff = float(np.max(np.abs(rd - rh)) / np.max(np.abs(rh)))
            del rh
            band_device(band, mu, lev, phi)
            for _ in range(a.calls):
                bh_r, t = band_host(band, mu, lev, phi)
                bh.append(t)
                bd_r, t = band_device(band, mu, lev, phi)
                bd.append(t)
            bdiff = float(np.max(np.abs(bd_r - bh_r)) / np.max(np.abs(bh_r)))
            best = min(th, key=lambda v: v["total"])
            bbest = min(bh, key=lambda v: v["total"])
            out[name] = dict(
                nmu=len(mu), ntau=len(lev), nphi=len(phi),
                columns_host_seconds_per_call=[rounded(v) for v in th], columns_device_seconds_per_call=[round(v["total"], 4) for v in td],
                columns_host_seconds=round(best["total"], 4), columns_host_scipy_part_seconds=round(min(v["scipy"] for v in th), 4),
                columns_device_seconds=round(min(v["total"] for v in td), 4), columns_difference_over_scale=diff,
                band_host_seconds_per_call=[rounded(v) for v in bh], band_device_seconds_per_call=[round(v["total"], 4) for v in bd],
                band_host_seconds=round(bbest["total"], 4), band_host_scipy_part_seconds=round(min(v["scipy"] for v in bh), 4),
                band_device_seconds=round(min(v["total"] for v in bd), 4), band_difference_over_scale=bdiff)
            print(name, json.dumps(out[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
