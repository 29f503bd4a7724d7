#!/usr/bin/env python3
"""Where a k-distribution band is mixed and spectrally integrated: on the host (NumPy) or on the device.

Batch: P = 6 250 profiles x G = 16 spectral points = 10^5 columns (BASELINE's count), S = 3 scatterer species, 20 layers,
NQuad = NLeg = NFourier = 32, K = 1 weight set; results at the L + 1 levels and 3 azimuths.  Two paths, host arrays in -> host
arrays out:

  (a) host:   the species mixed into tau_arr, omega_arr, f_arr, Leg_coeffs_all [C, L, NLeg] with NumPy, then
              pydisort_amd.solve_columns_streamed, then the P G results weighted and summed over g with NumPy;
  (b) device: pydisort_amd.solve_band_streamed.

Best of `--calls` calls each on one box; the host mixing and the host weighting are also reported alone.  Nothing is gated: the
numbers are recorded as they come, (b) faster or not.  Also reported: the largest difference of the two paths' band fluxes over
their scale.

Usage: python tools/band_prepare_timing.py [--profiles 6250] [--out profiles/band_prepare.json]
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
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_prepare.json"))
    a = ap.parse_args()
    import pydisort_amd

    P, G, S, L, NQ = a.profiles, a.gpoints, 3, 20, 32
    C = P * G
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
    phi = np.array([0.0, np.pi / 2, np.pi])
    keys = ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct")

    def host_mix():
        t = band["omega_spec"] * band["dtau_spec"]
        sca = t.sum(axis=2)
        dtau = band["dtau_spec"].sum(axis=2)[:, None, :] + band["dtau_abs"]
        leg = np.einsum("pls,sk->plk", t, leg_spec) / sca[:, :, None]
        leg[:, :, 0] = 1.0
        return dict(tau_arr=np.cumsum(dtau, axis=2).reshape(C, L), omega_arr=(sca[:, None, :] / dtau).reshape(C, L),
                    f_arr=np.repeat(leg[:, :, NQ], G, axis=0), Leg_coeffs_all=np.repeat(leg[:, :, :NQ], G, axis=0), NQuad=NQ,
                    mu0=np.repeat(mu0, G), I0=np.tile(I0, P), phi0=np.repeat(phi0, G))

    def path_a():
        t0 = time.perf_counter()
        cfg = host_mix()
        t1 = time.perf_counter()
        tau = np.concatenate((np.zeros((C, 1)), cfg["tau_arr"]), axis=1)
        res = pydisort_amd.solve_columns_streamed(cfg, tau, phi, chunk_columns=a.window)
        t2 = time.perf_counter()
        out = {kk: np.einsum("g,pg...->p...", w, res[kk].reshape((P, G) + res[kk].shape[1:])) for kk in keys}
        t3 = time.perf_counter()
        return out, dict(mix=t1 - t0, solve=t2 - t1, weight=t3 - t2, total=t3 - t0)

    def path_b():
        t0 = time.perf_counter()
        out = pydisort_amd.solve_band_streamed(**band, NQuad=NQ, mu0=mu0, I0=I0, phi0=phi0, weights=w, phi=phi, chunk_columns=a.window)
        return out, dict(total=time.perf_counter() - t0)

    # warm-up: a small band through both paths
    small = {kk: v[:32] for kk, v in band.items() if kk != "Leg_spec"}
    pydisort_amd.solve_band_streamed(**small, Leg_spec=leg_spec, NQuad=NQ, mu0=mu0[:32], I0=I0, phi0=phi0[:32], weights=w, phi=phi,
                                     chunk_columns=a.window)
    ta, tb, ra, rb = [], [], None, None
    with pydisort_amd.pooled():
        for _ in range(a.calls):
            ra, t = path_a()
            ta.append(t)
        fa = {kk: ra[kk] for kk in ("flux_up", "flux_down_diffuse", "flux_down_direct")}
        del ra
        for _ in range(a.calls):
            rb, t = path_b()
            tb.append(t)
    diff = max(float(np.max(np.abs(rb[kk] - fa[kk])) / np.max(np.abs(fa[kk]))) for kk in fa)
    best_a = min(ta, key=lambda t: t["total"])
    out = dict(
        what="a k-distribution band of P profiles x G spectral points (S = 3 species, 20 layers, 32 streams, results at 21 levels x 3 "
             "azimuths, one weight set): mixed and weighted on the host around solve_columns_streamed (a) or on the device by "
             "solve_band_streamed (b); host arrays in, host arrays out, seconds",
        profiles=P, gpoints=G, columns=C, species=S, layers=L, nquad=NQ, window=a.window,
        a_seconds_per_call=[{kk: round(v, 4) for kk, v in t.items()} for t in ta],
        b_seconds_per_call=[round(t["total"], 4) for t in tb],
        a_total_seconds=round(best_a["total"], 4), a_host_mix_seconds=round(min(t["mix"] for t in ta), 4),
        a_host_weight_seconds=round(min(t["weight"] for t in ta), 4), b_total_seconds=round(min(t["total"] for t in tb), 4),
        band_flux_difference_over_scale=diff)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
