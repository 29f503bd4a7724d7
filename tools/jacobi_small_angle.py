#!/usr/bin/env python3
"""NumPy replay of the eigen kernel's one-sided Jacobi iteration on cfg4 problems (CPU; no GPU needed): how many of the steps
a wavefront executes are SMALL-ANGLE steps -- every pair of every problem of the wavefront has |t| below a threshold, so
that fma(t, t, 1.0) is 1.0 and the rotation needs neither c nor the products by it (PairStep in
csrc/rtd_eig.hip).  The prediction that HISTORY.md sets beside the measured counters.

Built from tools/jacobi_convergence.py (the same F = L^T R and the same stop rule) with three things closer to the device:
the pairs meet in the kernel's butterfly order (tools/jacobi_schedule.py, `JSched`), t comes from float arithmetic as in
the kernel, and the layers are grouped four (64 / NP) to a wavefront in the kernel's layer order, ascending
omega* / (1 - g*): a wavefront sweeps until its slowest problem is done and takes the small-angle form of a step only
when all of its problems are below the threshold in that step.  `--round-robin` replays the pair order and the double t
of jacobi_convergence.py instead.

Prints the share of small-angle steps among the executed ones by threshold and by Fourier mode, and the change in vector
instructions per wavefront it predicts at 2^-27 from the static census of the shipped `rtd_eigen_kernel<16,2>` (HISTORY.md,
"Small-angle steps ..."): a sweep that takes the general form in every step is 1 426 VALU instructions where the parent's
was 1 398 (15 compares and 13 selects more), and each small-angle step among the 12 of 15 that hand on Y everywhere
is 23 fewer (the 3 steps that hand on X in some slots keep the general form with c = 1 by selects: no saving).

Usage: python3 tools/jacobi_small_angle.py [columns] [--round-robin]      (default 6 columns; about 15 s)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pythonic-disort_amd"), os.path.join(ROOT, "tools")]
from pydisort_amd import synthetic  # noqa: E402
from jacobi_convergence import F_of_column  # noqa: E402
from jacobi_schedule import build as jsched  # noqa: E402

TOL = 1e-14            # RTD_JAC_TOL
THRESHOLDS = (-20, -24, -27, -30, -34)   # log2 of the bound on |t|; the kernel's is 2^-27
SAVED_SW0, SAVED_SWX, ADDED_PER_SWEEP = 23, 0, 28


def step_maxima(W, sweeps=10, butterfly=True):
    """Per sweep, step and problem: max over the pairs of |t| and of cos^2 before the rotation: two arrays [sweeps, N - 1, n]."""
    n, N, _ = W.shape
    W = W.copy()
    H = N // 2
    sw, mk = jsched(N)
    X, Y = np.arange(H), np.arange(H, N)
    rr = list(range(N))
    tmax, cmax = np.zeros((sweeps, N - 1, n)), np.zeros((sweeps, N - 1, n))
    for k in range(sweeps):
        for s in range(N - 1):
            a, b = (X, Y) if butterfly else (np.array(rr[:H]), np.array(rr[H:][::-1]))
            x, y = W[:, :, a], W[:, :, b]
            gam, ax, ay = np.sum(x * y, 1), np.sum(x * x, 1), np.sum(y * y, 1)
            cmax[k, s] = np.max(gam * gam / (ax * ay), 1)
            delta, g2 = ay - ax, 2 * gam
            if butterfly:  # the kernel's float angle (PairStep)
                df, gf = delta.astype(np.float32), g2.astype(np.float32)
                r2 = df * df + (gf * gf + np.float32(1e-36))
                t = (gf / (df + np.copysign(np.sqrt(r2), df))).astype(np.float64)
            else:
                t = g2 / (delta + np.copysign(np.sqrt(delta * delta + g2 * g2 + 1e-280), delta))
            tmax[k, s] = np.max(np.abs(t), 1)
            c = 1 / np.sqrt(1 + t * t)
            sn = t * c
            W[:, :, a], W[:, :, b] = c[:, None, :] * x - sn[:, None, :] * y, sn[:, None, :] * x + c[:, None, :] * y
            if butterfly:
                swp = (np.arange(H) & sw[s]) != 0
                X, Y = np.where(swp, Y, X), np.where(swp, X, Y)
                Y = Y[np.arange(H) ^ mk[s]]
            else:
                rr = [rr[0]] + [rr[-1]] + rr[1:-1]
    return tmax, cmax


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    butterfly = "--round-robin" not in sys.argv
    C = int(args[0]) if args else 6
    cfg = synthetic.cfg4_columns(C)
    Fs, om, g = [], [], []
    for i in range(C):
        F, p = F_of_column(synthetic.column_kwargs(cfg, i))
        Fs.append(F)
        om.append(p["omega_s"])
        g.append(p["wleg"][:, 1] / 3)
    M, L, N = Fs[0].shape[0], Fs[0].shape[1], Fs[0].shape[2]
    GPW = 64 // N
    nst = N - 1
    sw_sched, _ = jsched(N)
    hands_on_x = np.array(sw_sched) != 0
    tmax, cmax = step_maxima(np.concatenate([F.reshape(-1, N, N) for F in Fs]), butterfly=butterfly)
    S = tmax.shape[0]
    tmax = tmax.reshape(S, nst, C, M, L)
    last = np.argmax(cmax.max(1) <= TOL, axis=0).reshape(C, M, L)  # the first sweep whose pairs were all below the tolerance
    # wavefronts: GPW consecutive layers of the kernel's order; a short last group repeats the last layer, as the kernel does
    nwf = -(-L // GPW)
    executed = np.zeros(M)
    small = np.zeros((len(THRESHOLDS), M))
    saved = np.zeros(M)
    for c in range(C):
        order = np.argsort(om[c] / np.maximum(1 - g[c], 1e-6), kind="stable")
        order = np.concatenate((order, np.repeat(order[-1:], nwf * GPW - L))).reshape(nwf, GPW)
        for m in range(M):
            for grp in order:
                ns = last[c, m, grp].max() + 1
                t = tmax[:ns, :, c, m, :][:, :, grp].max(2)  # [sweeps executed, steps]: the wavefront's largest |t|
                executed[m] += t.size
                for k, e in enumerate(THRESHOLDS):
                    small[k, m] += np.count_nonzero(t < 2.0 ** e)
                sm = t < 2.0 ** -27
                saved[m] += SAVED_SW0 * np.count_nonzero(sm[:, ~hands_on_x]) + SAVED_SWX * np.count_nonzero(sm[:, hands_on_x])
    nwave = C * M * nwf
    print(f"{C} cfg4 columns, {C * M * L} problems, {nwave} wavefronts of {GPW} layers; pair order: "
          f"{'butterfly, float t' if butterfly else 'round robin, double t'}")
    print(f"executed per wavefront: {executed.sum() / nwave / nst:.2f} sweeps = {executed.sum() / nwave:.1f} steps")
    print("share of the executed steps in which every pair of the wavefront has |t| below the threshold:")
    for k, e in enumerate(THRESHOLDS):
        print(f"  2^{e}: {100 * small[k].sum() / executed.sum():5.1f} %   ({small[k].sum() / nwave:5.1f} steps per wavefront)"
              + ("   <- the kernel's threshold" if e == -27 else ""))
    k27 = THRESHOLDS.index(-27)
    print("by Fourier mode at 2^-27 (steps executed per wavefront / small-angle steps among them):")
    for m0 in range(0, M, 8):
        print("  m = %2d..%2d: " % (m0, min(m0 + 8, M) - 1)
              + "  ".join(f"{executed[m] * M / nwave:5.1f}/{small[k27, m] * M / nwave:4.1f}" for m in range(m0, min(m0 + 8, M))))
    added = ADDED_PER_SWEEP * executed.sum() / nst
    print(f"vector instructions per wavefront at 2^-27: {saved.sum() / nwave:.0f} saved ({SAVED_SW0} / {SAVED_SWX} per step) - "
          f"{added / nwave:.0f} added ({ADDED_PER_SWEEP} per sweep) = {(saved.sum() - added) / nwave:.0f} fewer")


if __name__ == "__main__":
    main()
