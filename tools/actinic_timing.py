#!/usr/bin/env python3
"""What the actinic fluxes cost, host arrays in -> host arrays out.

Batch: P = 6 250 profiles x G = 16 spectral points = 10^5 columns (BASELINE's count), S = 3 scatterer species, 20 layers,
NQuad = NLeg = 32, fluxes only (one Fourier mode), results at the L + 1 = 21 levels, K = 1 weight set.

  (a) band:    pydisort_amd.solve_band_streamed(only_flux=True) without and with actinic=True (three more [P, K, 21] arrays);
  (b) columns: the band mixed on the host once (not timed), then pydisort_amd.solve_columns_streamed(only_flux=True) with u0
               [C, 32, 21] fetched and the three actinic arrays formed from it with NumPy (the weighted sums and the delta-M
               reclassification term from a host copy of the scaling) -- against actinic=True with u0 left on the device.

Best of `--calls` calls each after a warm-up, the two sides of a comparison alternating, on one box.  Nothing is gated: the numbers
are recorded as they come.  Also reported: the largest difference of (b)'s two sides over the arrays' scale.

Usage: python tools/actinic_timing.py [--profiles 6250] [--out profiles/actinic.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pythonic-disort_amd"))
ACT = ("flux_act_up", "flux_act_down_diffuse", "flux_act_down_direct")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profiles", type=int, default=6250)
    ap.add_argument("--gpoints", type=int, default=16)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actinic.json"))
    a = ap.parse_args()
    import pydisort_amd
    from pydisort_amd._prepare import double_gauss

    P, G, S, L, NQ = a.profiles, a.gpoints, 3, 20, 32
    C, N = P * G, NQ // 2
    rng = np.random.default_rng(11)
    k = np.arange(NQ + 1)
    rayleigh = np.zeros(NQ + 1)
    rayleigh[0], rayleigh[2] = 1.0, 0.1
    leg_spec = np.stack((0.85 ** k, 0.6 ** k, rayleigh))
    band = dict(dtau_abs=rng.uniform(0.01, 0.4, (P, G, L)) * 10.0 ** rng.uniform(-1.5, 0.5, (P, G, 1)),
                dtau_spec=rng.uniform(0.01, 0.3, (P, L, S)), omega_spec=rng.uniform(0.6, 0.999, (P, L, S)), Leg_spec=leg_spec)
    mu0, phi0 = rng.uniform(0.2, 0.95, P), rng.uniform(0.0, 2 * np.pi, P)
    I0 = rng.uniform(0.5, 2.0, G)
    w = rng.uniform(0.0, 1.0, G)
    w /= w.sum()

    def band_call(actinic):
        t0 = time.perf_counter()
        out = pydisort_amd.solve_band_streamed(**band, NQuad=NQ, mu0=mu0, I0=I0, phi0=phi0, weights=w, only_flux=True,
                                               chunk_columns=a.window, actinic=actinic)
        return out, time.perf_counter() - t0

    # (b): the columns of the same band, mixed on the host once
    t = band["omega_spec"] * band["dtau_spec"]
    sca = t.sum(axis=2)
    dtau = band["dtau_spec"].sum(axis=2)[:, None, :] + band["dtau_abs"]
    leg = np.einsum("pls,sk->plk", t, leg_spec) / sca[:, :, None]
    leg[:, :, 0] = 1.0
    cfg = dict(tau_arr=np.cumsum(dtau, axis=2).reshape(C, L), omega_arr=(sca[:, None, :] / dtau).reshape(C, L),
               f_arr=np.repeat(leg[:, :, NQ], G, axis=0), Leg_coeffs_all=np.repeat(leg[:, :, :NQ], G, axis=0), NQuad=NQ,
               mu0=np.repeat(mu0, G), I0=np.tile(I0, P), phi0=np.repeat(phi0, G))
    tau = np.concatenate((np.zeros((C, 1)), cfg["tau_arr"]), axis=1)
    W = double_gauss(N)[1]
    # host copy of the delta-M scaling at the levels (pydisort.py:316-329)
    taus = np.concatenate((np.zeros((C, 1)), np.cumsum((1.0 - cfg["omega_arr"] * cfg["f_arr"]) * dtau.reshape(C, L), axis=1)), axis=1)

    def columns_numpy():
        t0 = time.perf_counter()
        res = pydisort_amd.solve_columns_streamed(cfg, tau, None, chunk_columns=a.window, only_flux=True)
        t1 = time.perf_counter()
        u0 = res["u0"]
        direct = cfg["I0"][:, None] * np.exp(-tau / cfg["mu0"][:, None])
        out = dict(flux_act_up=2 * np.pi * np.einsum("i,cit->ct", W, u0[:, :N]),
                   flux_act_down_diffuse=2 * np.pi * np.einsum("i,cit->ct", W, u0[:, N:])
                   + cfg["I0"][:, None] * np.exp(-taus / cfg["mu0"][:, None]) - direct, flux_act_down_direct=direct)
        t2 = time.perf_counter()
        return out, dict(solve_and_fetch=t1 - t0, numpy=t2 - t1, total=t2 - t0)

    keep = {kk: np.empty((C, L + 1)) for kk in ACT + ("flux_up", "flux_down_diffuse", "flux_down_direct")}

    def columns_device():
        t0 = time.perf_counter()
        out = pydisort_amd.solve_columns_streamed(cfg, tau, None, chunk_columns=a.window, only_flux=True, actinic=True, out=keep)
        return out, dict(total=time.perf_counter() - t0)

    # warm-up: a small band through every path
    small = {kk: v[:32] for kk, v in band.items() if kk != "Leg_spec"}
    for act in (False, True):
        pydisort_amd.solve_band_streamed(**small, Leg_spec=leg_spec, NQuad=NQ, mu0=mu0[:32], I0=I0, phi0=phi0[:32], weights=w,
                                         only_flux=True, chunk_columns=a.window, actinic=act)
    scfg = {kk: (v[:512] if isinstance(v, np.ndarray) else v) for kk, v in cfg.items()}
    pydisort_amd.solve_columns_streamed(scfg, tau[:512], None, chunk_columns=a.window, only_flux=True, actinic=True)
    plain, withact, tn, td = [], [], [], []
    with pydisort_amd.pooled():
        band_call(True)  # (one full-size call: the pool holds the blocks of this size from here on)
        for _ in range(a.calls):
            plain.append(band_call(False)[1])
            withact.append(band_call(True)[1])
        for _ in range(a.calls):
            rn, tt = columns_numpy()
            tn.append(tt)
            rd, tt = columns_device()
            td.append(tt)
    diff = max(float(np.max(np.abs(rd[kk] - rn[kk])) / np.max(np.abs(rn[kk]))) for kk in ACT)
    best_n = min(tn, key=lambda x: x["total"])
    out = dict(
        what="actinic fluxes of P profiles x G spectral points (S = 3 species, 20 layers, 32 streams, fluxes only, 21 levels, one "
             "weight set), host arrays in, host arrays out, seconds: (a) solve_band_streamed without and with actinic=True; (b) "
             "solve_columns_streamed with u0 fetched and the actinic fluxes formed with NumPy, against actinic=True with u0 left on "
             "the device; best of the calls listed, the two sides alternating, after a warm-up",
        profiles=P, gpoints=G, columns=C, layers=L, nquad=NQ, window=a.window,
        band_plain_seconds_per_call=[round(v, 4) for v in plain], band_actinic_seconds_per_call=[round(v, 4) for v in withact],
        band_plain_seconds=round(min(plain), 4), band_actinic_seconds=round(min(withact), 4),
        columns_numpy_seconds_per_call=[{kk: round(v, 4) for kk, v in x.items()} for x in tn],
        columns_device_seconds_per_call=[round(x["total"], 4) for x in td],
        columns_numpy_seconds=round(best_n["total"], 4), columns_numpy_host_part_seconds=round(min(x["numpy"] for x in tn), 4),
        columns_device_seconds=round(min(x["total"] for x in td), 4), columns_difference_over_scale=diff)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
