#!/usr/bin/env python3
"""What device-formed surface modes cost, host arrays in -> host arrays out.

10^5 benchmark columns (synthetic.cfg4_columns_block: 20 layers, NQuad = NLeg = NFourier = 32) with Ross-Li kernel weights per column;
NBDRF = 8 and 32 modes from nphi = 256 and 1024 azimuths:

  (a) pydisort_amd.solve_columns_streamed with surface=dict(model="rossli", params=[C, 3], nphi=...) -- rtd_surface_samples_kernel and
      rtd_bdrf_modes_kernel per chunk of columns (RTD_SURFACE_BYTES) ahead of the solve -- against the SAME call with a one-mode
      Lambert table bdrf_q [C, 1, N, N]: what the surface adds to a batch (more modes also cost the solve its reflection terms);
  (b) the host route of today per column: subroutines.sample_BDRF of a NumPy Ross-Li closure + bdrf_samples, on 256 columns, in
      seconds per column (sampling alone, and the whole pydisort_batch call).

Fluxes at the top and the bottom of every column are fetched.  Best of `--calls` calls each after a warm-up, the two sides of (a)
alternating, on one box.  Nothing is gated: the numbers are recorded as they come, under "timing" of profiles/surface.json (the
"convergence" entry of tools/surface_truth.py is kept).

Usage: python tools/surface_timing.py [--columns 100000] [--out profiles/surface.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=100_000)
    ap.add_argument("--host-columns", type=int, default=256)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface.json"))
    a = ap.parse_args()
    import pydisort_amd
    from pydisort_amd import subroutines as sub, synthetic
    from surface_truth import rho_numpy

    C, NQ = a.columns, 32
    N = NQ // 2
    cfg = synthetic.cfg4_columns_block(C, first=0)
    rng = np.random.default_rng(21)
    par = np.stack((rng.uniform(0.05, 0.4, C), rng.uniform(0.0, 0.3, C), rng.uniform(0.0, 0.08, C)), axis=1)
    tau = np.stack((np.zeros(C), cfg["tau_arr"][:, -1]), axis=1)
    phi = np.array([0.0])
    lam_q, lam_q0 = np.broadcast_to(par[:, :1, None, None], (C, 1, N, N)).copy(), np.broadcast_to(par[:, :1, None], (C, 1, N)).copy()

    def device(n, nb, nphi):
        c = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in cfg.items()}
        t0 = time.perf_counter()
        out = pydisort_amd.solve_columns_streamed(dict(c, surface=dict(model="rossli", params=par[:n], nphi=nphi), NBDRF=nb), tau[:n], phi,
                                                  chunk_columns=a.window)
        return out, time.perf_counter() - t0

    def lambert(n):
        c = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in cfg.items()}
        t0 = time.perf_counter()
        out = pydisort_amd.solve_columns_streamed(dict(c, bdrf_q=lam_q[:n], bdrf_q0=lam_q0[:n]), tau[:n], phi, chunk_columns=a.window)
        return out, time.perf_counter() - t0

    def host(n, nb, nphi):
        """sample_BDRF per column + bdrf_samples: (seconds sampling, seconds of the whole route), per column"""
        c = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in cfg.items()}
        t0 = time.perf_counter()
        qq, q0 = np.empty((n, N, N, nphi)), np.empty((n, N, nphi))
        for i in range(n):
            f = lambda mu, mup, dphi, p=par[i]: rho_numpy("rossli", p, mu, mup, np.cos(dphi), np.sin(dphi))  # noqa: E731
            qq[i], q0[i] = sub.sample_BDRF(f, NQ, float(cfg["mu0"][i]), nphi=nphi)
        t1 = time.perf_counter()
        _, sol = pydisort_amd.pydisort_batch(**c, device_prepare=True, bdrf_samples=(qq, q0), NBDRF=nb)
        sol.flux_up(tau[:n])
        t2 = time.perf_counter()
        return (t1 - t0) / n, (t2 - t0) / n

    device(512, 8, 256)
    lambert(512)
    out = dict(what="solve_columns_streamed of the benchmark columns (20 layers, 32 streams, all modes), fluxes at top and bottom fetched, "
                    "seconds: surface=Ross-Li per column with NBDRF modes from nphi azimuths against the same call with a one-mode "
                    "Lambert table; best of the calls listed, the two sides alternating, after a warm-up; host route = sample_BDRF of "
                    "a NumPy closure per column + bdrf_samples, seconds per column on host_columns columns; no threshold set",
               columns=C, host_columns=a.host_columns, nquad=NQ, layers=20, window=a.window, cases={})
    with pydisort_amd.pooled():
        lambert(C)  # (one full-size call: the pool holds the blocks of this size from here on)
        for nb in (8, 32):
            for nphi in (256, 1024):
                td, tl = [], []
                for _ in range(a.calls):
                    td.append(device(C, nb, nphi)[1])
                    tl.append(lambert(C)[1])
                hs, ht = host(a.host_columns, nb, nphi)
                case = dict(nbdrf=nb, nphi=nphi, surface_seconds_per_call=[round(v, 4) for v in td], lambert_seconds_per_call=[round(v, 4) for v in tl],
                            surface_seconds=round(min(td), 4), lambert_seconds=round(min(tl), 4), added_seconds=round(min(td) - min(tl), 4),
                            samples_formed=int(C * (N * N + N) * nphi), host_sampling_seconds_per_column=round(hs, 6),
                            host_route_seconds_per_column=round(ht, 6), device_added_seconds_per_column=(min(td) - min(tl)) / C)
                out["cases"][f"nbdrf{nb}_nphi{nphi}"] = case
                print(json.dumps(case), flush=True)
    prof = json.load(open(a.out)) if os.path.exists(a.out) else {}
    prof["timing"] = out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(prof, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
