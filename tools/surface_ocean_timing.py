#!/usr/bin/env python3
"""What the ocean's device-formed modes cost, host arrays in -> fluxes out.

10^5 benchmark columns (synthetic.cfg4_columns_block: 20 layers, NQuad = NLeg = NFourier = 32) with a wind speed per column
(n = 1.34, rho_w = 0.01); NBDRF = 8 and 32 modes from nphi = 512 nodes of the clustered azimuth grid (rtd_surface_ocean_kernel: one
pass per pair of cosines, no scratch block), through pydisort_amd.solve_columns_streamed.  Beside it the SAME call with a one-mode
Lambert table bdrf_q [C, 1, N, N] and with surface=Ross-Li at nphi = 256 (the uniform-grid route: rtd_surface_samples_kernel +
rtd_bdrf_modes_kernel per chunk of columns).  More modes also cost the solve its reflection terms, whichever route formed them.

Fluxes at the top and the bottom of every column are fetched.  Best of `--calls` calls each after a warm-up, the three sides
alternating, on one box.  Nothing is gated: the numbers are recorded as they come, under "timing" of profiles/surface_ocean.json
(the "convergence" entry of tools/surface_ocean_truth.py is kept).

Usage: python tools/surface_ocean_timing.py [--columns 100000] [--out profiles/surface_ocean.json]
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
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_ocean.json"))
    a = ap.parse_args()
    import pydisort_amd
    from pydisort_amd import synthetic

    C, NQ = a.columns, 32
    N = NQ // 2
    cfg = synthetic.cfg4_columns_block(C, first=0)
    rng = np.random.default_rng(22)
    ocean = np.stack((rng.uniform(0.0, 15.0, C), np.full(C, 1.34), np.full(C, 0.01)), axis=1)
    rossli = np.stack((rng.uniform(0.05, 0.4, C), rng.uniform(0.0, 0.3, C), rng.uniform(0.0, 0.08, C)), axis=1)
    tau = np.stack((np.zeros(C), cfg["tau_arr"][:, -1]), axis=1)
    phi = np.array([0.0])
    lam_q, lam_q0 = np.full((C, 1, N, N), 0.06), np.full((C, 1, N), 0.06)

    def call(n, extra):
        c = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in cfg.items()}
        t0 = time.perf_counter()
        out = pydisort_amd.solve_columns_streamed(dict(c, **extra), tau[:n], phi, chunk_columns=a.window)
        return out, time.perf_counter() - t0

    sides = {
        "ocean": lambda n, nb: dict(surface=dict(model="ocean", params=ocean[:n], nphi=512), NBDRF=nb),
        "rossli_nphi256": lambda n, nb: dict(surface=dict(model="rossli", params=rossli[:n], nphi=256), NBDRF=nb),
        "lambert_table": lambda n, nb: dict(bdrf_q=lam_q[:n], bdrf_q0=lam_q0[:n]),
    }
    for name, mk in sides.items():
        call(512, mk(512, 8))
    out = dict(what="solve_columns_streamed of the benchmark columns (20 layers, 32 streams, all modes), fluxes at top and bottom fetched, "
                    "seconds: surface=ocean per column (U per column) with NBDRF modes from nphi = 512 clustered nodes, beside the same call "
                    "with Ross-Li at nphi = 256 (uniform grid) and with a one-mode Lambert table; best of the calls listed, the sides "
                    "alternating, after a warm-up; no threshold set",
               columns=C, nquad=NQ, layers=20, window=a.window, cases={})
    with pydisort_amd.pooled():
        call(C, sides["lambert_table"](C, 1))  # (one full-size call: the pool holds the blocks of this size from here on)
        for nb in (8, 32):
            t = {k: [] for k in sides}
            for _ in range(a.calls):
                for name, mk in sides.items():
                    t[name].append(call(C, mk(C, nb))[1])
            case = dict(nbdrf=nb, seconds_per_call={k: [round(x, 4) for x in v] for k, v in t.items()}, seconds={k: round(min(v), 4) for k, v in t.items()},
                        ocean_added_seconds=round(min(t["ocean"]) - min(t["lambert_table"]), 4),
                        rossli_added_seconds=round(min(t["rossli_nphi256"]) - min(t["lambert_table"]), 4),
                        ocean_samples_evaluated=int(C * (N * N + N) * (512 // 2 + 1)))
            out["cases"][f"nbdrf{nb}"] = case
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
