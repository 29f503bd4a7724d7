#!/usr/bin/env python3
"""What evaluating the Nakajima-Tanaka corrections at the viewing angles themselves (Plan.set_view(corrections="at_angles");
csrc/rtd_nt_view.hip) gains and costs, written to profiles/nt_view.json.  Nothing is gated: the numbers are recorded as they come.

accuracy  One column with the phase function of the cloud fixture (tests/golden/make_nt_truth_goldens.py: q32_L20_cloud -- 20
          layers, Henyey-Greenstein g = 0.9 ... 0.945 per layer, 300 moments, mu0 = 0.6), solved with 16 and with 32 streams.
          Downward radiance at the bottom and in the middle of the atmosphere, in the principal plane (phi = phi0), from the solar
          aureole to 30 degrees off the sun: mu = -cos(theta0 + delta), delta = 0, 0.5, 1, 2, 5, 10, 20, 30 degrees.  Both modes
          against a 128-stream solve with the corrections at the same angles; the figure is |u - u_128| / u_128 per angle.
cost      10^5 benchmark columns as a band of 6 250 profiles x 16 spectral points (the band of tools/view_timing.py, 20 layers, 32
          streams, all modes) with NT_cor, host arrays in -> host arrays out through solve_band_streamed, once at one angle (tau = 0,
          one azimuth) and once at 3 angles x 21 levels x 3 azimuths: view_corrections="at_angles" against "interpolated", best of
          `--calls` alternating calls after a warm-up, as tools/view_timing.py takes it.
resources VGPRs, spills and LDS of the two kernels from the code-object metadata (tools/kernel_resources.py): NOT measured, read.

Usage: python tools/nt_view_timing.py [--profiles 6250] [--calls 2] [--out profiles/nt_view.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pythonic-disort_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def accuracy(amd):
    k = np.arange(20)
    tau_arr = np.cumsum(0.1 + 0.25 * np.sin(0.7 * k) ** 2)
    omega = 0.7 + 0.29 * np.cos(0.41 * k) ** 2
    g = 0.9 + 0.045 * np.sin(0.3 * k) ** 2
    leg = g[:, None] ** np.arange(300)[None, :]
    mu0, phi0 = 0.6, 0.5
    delta = np.array([0.0, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 30.0])
    mu = -np.cos(np.arccos(mu0) + np.radians(delta))
    tau = np.array([[tau_arr[9], tau_arr[-1]]])
    phi = np.array([phi0])

    def solve(NQuad, corrections):
        _, sol = amd.pydisort_batch(tau_arr[None], omega[None], NQuad, leg[None], np.array([mu0]), np.array([3.0]), np.array([phi0]),
                                    f_arr=leg[None, :, NQuad], NT_cor=True)
        u = sol.u_at(mu, tau, phi, corrections=corrections)[0, :, :, 0]  # [nmu, ntau]
        sol.plan.close()
        return u

    ref = solve(128, "at_angles")
    out = dict(what="one cloud column (20 layers, 300 moments, mu0 = 0.6): downward radiance in the principal plane at delta degrees off the "
                    "sun, |u - u_128| / u_128 with u_128 a 128-stream solve with the corrections at the angles; rows: mid-atmosphere, bottom",
               degrees_off_the_sun=delta.tolist(), mu=mu.tolist(), tau=tau[0].tolist(), u_128_streams=ref.T.tolist())
    for NQuad in (16, 32):
        for mode in ("interpolated", "at_angles"):
            u = solve(NQuad, mode)
            out[f"{NQuad}_streams_{mode}_relative_error"] = (np.abs(u - ref) / np.abs(ref)).T.tolist()
    return out


def cost(amd, P, G, calls, window):
    from pydisort_amd.band import level_tau  # noqa: F401
    L, NQ, S = 20, 32, 3
    rng = np.random.default_rng(11)
    k = np.arange(NQ + 1)
    rayleigh = np.zeros(NQ + 1)
    rayleigh[0], rayleigh[2] = 1.0, 0.1
    band = dict(dtau_abs=rng.uniform(0.01, 0.4, (P, G, L)) * 10.0 ** rng.uniform(-1.5, 0.5, (P, G, 1)),
                dtau_spec=rng.uniform(0.01, 0.3, (P, L, S)), omega_spec=rng.uniform(0.6, 0.999, (P, L, S)),
                Leg_spec=np.stack((0.85 ** k, 0.6 ** k, rayleigh)), NQuad=NQ, NLeg=NQ, mu0=rng.uniform(0.2, 0.95, P), I0=rng.uniform(0.5, 2.0, G),
                phi0=rng.uniform(0.0, 2 * np.pi, P))
    w = rng.uniform(0.0, 1.0, G)
    band["weights"] = w / w.sum()
    requests = {"toa": (np.array([0.8]), [0], np.array([0.0])),
                "grid": (np.array([0.8, 0.35, -0.6]), list(range(L + 1)), np.array([0.0, 1.0, np.pi]))}

    def call(bkw, mu, lev, phi, mode):
        t0 = time.perf_counter()
        res = amd.solve_band_streamed(**bkw, levels=lev, phi=phi, chunk_columns=window, NT_cor=True, mu=mu, view_corrections=mode)
        return res["u_mu"], time.perf_counter() - t0

    small = {kk: (v[:32] if isinstance(v, np.ndarray) and v.shape[:1] == (P,) else v) for kk, v in band.items()}
    for mu, lev, phi in requests.values():
        for mode in ("interpolated", "at_angles"):
            call(small, mu, lev, phi, mode)
    out = dict(what="solve_band_streamed(NT_cor=True, mu=...) host arrays in -> host arrays out, seconds, view_corrections at_angles against "
                    "interpolated; best of the calls listed, alternating, after a warm-up; no threshold set",
               profiles=P, gpoints=G, columns=P * G, layers=L, nquad=NQ, window=window)
    with amd.pooled():
        for name, (mu, lev, phi) in requests.items():
            call(band, mu, lev, phi, "at_angles")  # (one full-size call: the pool holds the blocks of this size from here on)
            t_off, t_on = [], []
            for _ in range(calls):
                a, t = call(band, mu, lev, phi, "interpolated")
                t_off.append(round(t, 4))
                b, t = call(band, mu, lev, phi, "at_angles")
                t_on.append(round(t, 4))
            out[name] = dict(nmu=len(mu), nlev=len(lev), nphi=len(phi), interpolated_seconds_per_call=t_off, at_angles_seconds_per_call=t_on,
                             interpolated_seconds=min(t_off), at_angles_seconds=min(t_on),
                             at_angles_over_interpolated=round(min(t_on) / min(t_off), 4),
                             largest_difference_of_the_two_modes_over_scale=float(np.max(np.abs(a - b)) / np.max(np.abs(a))))
            print(name, json.dumps(out[name]), flush=True)
    return out


def resources():
    import kernel_resources
    ks = kernel_resources.kernels_of(os.path.join(ROOT, "pythonic-disort_amd", "pydisort_amd", "librtd.so"))
    return {n: r for n, r in ks.items() if "rtd_nt_view" in n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profiles", type=int, default=6250)
    ap.add_argument("--gpoints", type=int, default=16)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nt_view.json"))
    a = ap.parse_args()
    import pydisort_amd
    out = dict(tool="tools/nt_view_timing.py", measured="accuracy and cost on one MI355X; resources read from the code object, not measured")
    out["resources"] = resources()
    out["accuracy"] = accuracy(pydisort_amd)
    print("accuracy", json.dumps(out["accuracy"]), flush=True)
    out["cost"] = cost(pydisort_amd, a.profiles, a.gpoints, a.calls, a.window)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["resources"]))


if __name__ == "__main__":
    main()
