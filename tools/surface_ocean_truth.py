#!/usr/bin/env python3
"""Truth of the ocean surface model (RTD_SURFACE_OCEAN, csrc/rtd_surface.h) and of its clustered azimuth rule
(csrc/rtd_surface_ocean.hip), and the fixtures tests/golden/surface_ocean/*.npz.  In the manner of tools/surface_truth.py.

1. rho_U<U>_n<streams>.npz -- the reflectance in 50 digits (mpmath) FROM THE FLOAT64 INPUTS the routine takes: par, mu, mu', c, s.
   c and s are taken as they are given (cos and sin of an angle, rounded: the truth does not know the angle), so the distance of a
   float64 evaluation from this truth is rounding alone and not the conditioning of the glint in dphi.  mu: the double-Gauss nodes
   of 6 / 16 / 34 / 64 streams and 1; mu': the nodes, 1 and two random values; per pair the azimuths 0, pi/2, pi (exact c, s), the
   glint's own scale delta x (0.3, 1, 2, 4) and three random angles; U = 0, 1, 5, 15 m/s, n = 1.34, rho_w = 0.02.  `scale` is the
   row's max |rho| (a row: one pair of cosines over its azimuths); `np_dist_all[0]` the worst distance of a plain NumPy float64
   evaluation from the truth over all files, of `scale`.  The tests allow 16 x that, as tests/test_surface_cpu.py does.
   `albedo` is Sum_j 2 mu_j w_j q^0(mu_i, mu_j) at every node with rho_w = 0, q^0 by the rule below at 4096 nodes (float64).

2. modes_n<streams>.npz -- the modes OF THE SAME QUADRATURE RULE in 50 digits, for the columns the GPU and the host tests solve:
       b = rtd_ocean_cluster_b (float64 -> float32, as the header defines it; taken from the float64 formula here), a = 1 - b,
       psi_p = 2 pi p / nphi,  dphi_p = b psi_p + a (psi_p - sin psi_p),  w_p = e_p (b + 2 a sin^2(psi_p / 2)),  p = 0 ... nphi / 2,
       q^m = (2 - delta_m0) (2 / nphi) Sum_p w_p rho(mu, mu', dphi_p) cos(m dphi_p),
   nodes, weights and rho in 50 digits from b and the float64 cosines and parameters.  THE BOUND a float64 evaluation of the rule is
   held to, of (2 - delta_m0) q^0 of the pair (rho >= 0: q^0 is the rule's sum of |terms|):
       tol_m = 16 np_dist_modes + (52 m + 104 + nphi / 2 + 8) u,   u = 2^-53 .
   The second part is derived in csrc/rtd_surface_ocean.hip from the loop as written (the factors cos(m dphi) by blocks of eight,
   the summation).  The first covers what the rounding of dphi_p, of its cosine and sine and of rho does to a sample: it is 16 x the
   distance of a NumPy float64 evaluation of the same rule (direct cosines) from the truth, measured here and stored -- the glint is
   a Gaussian in dphi / delta, so a rounding of dphi by u pi moves a sample by up to (6 / delta) u pi of itself, which no float64
   evaluation avoids; 16 leaves room for another libm, as in item 1.
   `q_conv` / `q0_conv`: the CONVERGED integrals, the same rule at 4096 nodes in float64.  `conv_fig`: the worst distance of the
   file's nphi from them over the file's pairs and modes, of each pair's own max_m |q^m| -- the figure the GPU test allows, times
   its stated margin, between the device's tables and the converged integrals.
   `adaptive`: for a few pairs, scipy's adaptive quadrature of the uniform-dphi integral (float64, epsabs 1e-13), next to q_conv.

3. --convergence: the convergence table of the rule for EVERY mode up to NBDRF = 64, nphi = 256 and 512 against 4096, at 6 / 16 /
   34 / 64 streams and U = 0, 1, 5, 15 -> profiles/surface_ocean.json ("convergence").  The default nphi = 512 of the front end
   follows this table.

Usage: python tools/surface_ocean_truth.py [--convergence] [--only-convergence]"""
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "surface_ocean")
PROFILE = os.path.join(ROOT, "profiles", "surface_ocean.json")
WINDS = (0.0, 1.0, 5.0, 15.0)
N_REFR, RHO_W = 1.34, 0.02
STREAMS = (6, 16, 34, 64)
MODE_CASES = {6: (6, 256), 16: (6, 256), 34: (6, 512), 64: (1, 512)}  # streams -> (columns, nphi); NBDRF = streams
U64 = 2.0 ** -53


def double_gauss(N):
    x, w = np.polynomial.legendre.leggauss(N)
    o = np.argsort(x)
    return (x[o] + 1) / 2, w[o] / 2


def erfc_np(v):
    from scipy.special import erfc
    return erfc(v)


def lambda_np(x, sig):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = x / (sig * np.sqrt((1 - x) * (1 + x)))
        lam = np.maximum(0.0, 0.5 * (np.exp(-v * v) / (np.sqrt(np.pi) * v) - erfc_np(v)))
    return np.where(x < 1.0, lam, 0.0)


def rho_numpy(par, mu, mup, c, s):
    """The ocean of csrc/rtd_surface.h in NumPy float64 (broadcasting); par = (U, n, rho_w) (arrays allowed)."""
    U, n, rw = par
    sm, sp = np.sqrt((1 - mu) * (1 + mu)), np.sqrt((1 - mup) * (1 + mup))
    ss, sm_, b = sm * s, mu + mup, sm * c - sp
    g = 0.5 * (b * b + ss * ss + sm_ * sm_)
    n2, sig2 = n * n, 0.003 + 0.00512 * U
    sig = np.sqrt(sig2)
    cw, r = np.sqrt(0.5 * g), np.sqrt(n2 - (1 - 0.5 * g))
    fs, fp = (cw - r) / (cw + r), (n2 * cw - r) / (n2 * cw + r)
    F = 0.5 * (fs * fs + fp * fp)
    mun2 = sm_ * sm_ / (2 * g)
    tan2 = (b * b + ss * ss) / (sm_ * sm_)
    S = 1 / (1 + lambda_np(mu, sig) + lambda_np(mup, sig))
    return F * np.exp(-tan2 / sig2) * S / (4 * sig2 * mu * mup * mun2 * mun2) + rw


def cluster_b(U, mu, mup):
    """rtd_ocean_cluster_b: float32(min(1, 2 delta)) held in [2^-20, 1]; 1 when sm sp = 0."""
    mu, mup, U = np.broadcast_arrays(np.asarray(mu, float), np.asarray(mup, float), np.asarray(U, float))
    q = np.sqrt((1 - mu) * (1 + mu)) * np.sqrt((1 - mup) * (1 + mup))
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = 2.0 * np.sqrt(0.003 + 0.00512 * U) * (mu + mup) / np.sqrt(q)
    ok = (q > 0) & (d2 < 1.0)
    b = np.maximum(np.where(ok, d2, 1.0).astype(np.float32).astype(np.float64), 2.0 ** -20)
    return np.where(ok, b, 1.0)


def rule_numpy(par, mu, mup, nphi, nb):
    """The rule in NumPy float64 with direct cosines: mu, mup and the entries of par broadcast to a common shape S -> q [nb] + S."""
    U, n, rw = [np.asarray(v, float) for v in par]
    b = cluster_b(U, mu, mup)[..., None]
    a = 1.0 - b
    p = np.arange(nphi // 2 + 1)
    x = 2.0 * p / nphi
    psi = np.pi * x
    # sin psi, sin(psi / 2) with the argument reduced as sinpi does
    spsi = np.sin(np.pi * np.where(x > 0.5, 1.0 - x, x))
    sh = np.where(p * 4 <= nphi, np.sin(np.pi * p / nphi), np.cos(np.pi * (0.5 - p / nphi)))
    dphi = b * psi + a * (psi - spsi)
    e = np.where((p == 0) | (p == nphi // 2), 0.5, 1.0)
    w = e * (b + 2 * a * sh * sh)
    rho = rho_numpy((U[..., None], n[..., None], rw[..., None]), np.asarray(mu)[..., None], np.asarray(mup)[..., None], np.cos(dphi), np.sin(dphi))
    v = w * rho
    q = np.stack([np.sum(v * np.cos(m * dphi), axis=-1) * (1.0 if m == 0 else 2.0) * 2.0 / nphi for m in range(nb)])
    return q


# ---- 50 digits ----
def _mp():
    import mpmath as mp
    mp.mp.dps = 50
    return mp


_LAM = {}


def lambda_mp(mp, x, sig2):
    key = (float(x), float(sig2))
    if key not in _LAM:
        x_, s2 = mp.mpf(float(x)), mp.mpf(float(sig2)) if not isinstance(sig2, mp.mpf) else sig2
        if x_ >= 1:
            _LAM[key] = mp.mpf(0)
        else:
            v = x_ / (mp.sqrt(s2) * mp.sqrt(1 - x_ * x_))
            lam = (mp.exp(-v * v) / (mp.sqrt(mp.pi) * v) - mp.erfc(v)) / 2
            _LAM[key] = lam if lam > 0 else mp.mpf(0)
    return _LAM[key]


def rho_mp(mp, par, mu, mup, c, s):
    """One sample in mpmath from the formulas as include/rtd.h states them; par, mu, mup float64, c and s mpf."""
    mpf = mp.mpf
    U, n, rw = [mpf(float(v)) for v in par]
    m, mq = mpf(float(mu)), mpf(float(mup))
    sm, sp = mp.sqrt(1 - m * m), mp.sqrt(1 - mq * mq)
    sig2 = mpf("0.003") + mpf("0.00512") * U
    g = ((sm * c - sp) ** 2 + (sm * s) ** 2 + (m + mq) ** 2) / 2
    cw, sw2 = mp.sqrt(g / 2), 1 - g / 2
    r = mp.sqrt(n * n - sw2)
    F = (((cw - r) / (cw + r)) ** 2 + ((n * n * cw - r) / (n * n * cw + r)) ** 2) / 2
    mun2 = (m + mq) ** 2 / (2 * g)
    tan2 = ((sm * c - sp) ** 2 + (sm * s) ** 2) / (m + mq) ** 2
    S = 1 / (1 + lambda_mp(mp, mu, sig2) + lambda_mp(mp, mup, sig2))
    return F * mp.exp(-tan2 / sig2) * S / (4 * sig2 * m * mq * mun2 * mun2) + rw


def _rho_row(job):
    """(par, mu, mup [M], c [M][K], s [M][K]) -> rho [M][K] as float64 of the 50-digit value and the NumPy distance numerators"""
    par, mu, mups, c, s = job
    mp = _mp()
    out = np.empty(c.shape)
    dist = np.empty(c.shape)
    got = rho_numpy(par, mu, mups[:, None], c, s)
    for j, mq in enumerate(mups):
        for k in range(c.shape[1]):
            t = rho_mp(mp, par, mu, mq, mp.mpf(float(c[j, k])), mp.mpf(float(s[j, k])))
            out[j, k] = float(t)
            dist[j, k] = float(abs(mp.mpf(float(got[j, k])) - t))
    return out, dist


def make_rho_case(pool, U, nquad):
    N = nquad // 2
    nodes, wts = double_gauss(N)
    rng = np.random.default_rng(1000 * nquad + int(U))
    mu = np.concatenate((nodes, [1.0]))
    mup = np.concatenate((nodes, [1.0], rng.uniform(0.01, 1.0, 2)))
    par = (U, N_REFR, RHO_W)
    sig = np.sqrt(0.003 + 0.00512 * U)
    sm, sp = np.sqrt((1 - mu) * (1 + mu))[:, None], np.sqrt((1 - mup) * (1 + mup))[None, :]
    with np.errstate(divide="ignore"):
        delta = np.minimum(1.0, sig * (mu[:, None] + mup[None, :]) / np.sqrt(sm * sp))
    K = 10
    ang = np.empty((len(mu), len(mup), K))
    ang[..., 0], ang[..., 1], ang[..., 2] = 0.0, np.pi / 2, np.pi
    for k, f in enumerate((0.3, 1.0, 2.0, 4.0)):
        ang[..., 3 + k] = np.minimum(f * delta, 3.0)
    ang[..., 7:] = rng.uniform(0.0, np.pi, (len(mu), len(mup), 3))
    c, s = np.cos(ang), np.sin(ang)
    c[..., 0], s[..., 0], c[..., 1], s[..., 1], c[..., 2], s[..., 2] = 1.0, 0.0, 0.0, 1.0, -1.0, 0.0
    res = pool.map(_rho_row, [(par, mu[i], mup, c[i], s[i]) for i in range(len(mu))])
    rho = np.array([r[0] for r in res])
    scale = np.max(np.abs(rho), axis=2)
    d = float(np.max(np.array([r[1] for r in res]) / scale[:, :, None]))
    # hemispherical albedo at every node, glint alone (rho_w = 0), by the rule at 4096 nodes
    q0 = rule_numpy((U, N_REFR, 0.0), nodes[:, None], nodes[None, :], 4096, 1)[0]
    albedo = np.sum(2 * nodes[None, :] * wts[None, :] * q0, axis=1)
    return dict(params=np.array([U, N_REFR, RHO_W, 0.0]), mu=mu, mup=mup, c=c, s=s, rho=rho, scale=scale, np_dist=np.array([d]), albedo=albedo)


def _mode_row(job):
    """One pair of cosines: (par, mu, mup, b, nphi, nb) -> [nb] modes of the rule in 50 digits, rounded once"""
    par, mu, mup, b, nphi, nb = job
    mp = _mp()
    mpf = mp.mpf
    bb = mpf(float(b))
    a = 1 - bb
    acc = [mpf(0)] * nb
    half = nphi // 2
    for p in range(half + 1):
        psi = 2 * mp.pi * p / nphi
        dphi = bb * psi + a * (psi - mp.sin(psi))
        w = (bb + 2 * a * mp.sin(psi / 2) ** 2) * (mpf("0.5") if p in (0, half) else 1)
        c, s = mp.cos(dphi), mp.sin(dphi)
        v = w * rho_mp(mp, par, mu, mup, c, s)
        t0, t1 = mpf(1), c  # (Chebyshev recurrence in 50 digits: its m^2 growth is of 1e-50)
        acc[0] += v
        for m in range(1, nb):
            acc[m] += v * t1
            t0, t1 = t1, 2 * c * t1 - t0
    return [float(acc[m] * (1 if m == 0 else 2) * 2 / nphi) for m in range(nb)]


def mode_columns(nquad):
    """The columns of tests/test_gpu_surface_ocean.py at `nquad` streams: per-column (U, n, rho_w) and mu0."""
    C = MODE_CASES[nquad][0]
    rng = np.random.default_rng(4000 + nquad)
    par = np.stack((np.array([0.0, 1.0, 5.0, 15.0, 2.5, 9.0])[:C], rng.uniform(1.31, 1.36, C), np.array([0.0, 0.02, 0.0, 0.05, 0.01, 0.0])[:C]), axis=1)
    mu0 = np.concatenate(([1.0], rng.uniform(0.2, 0.95, C - 1))) if C > 1 else np.array([0.37])  # (the first column: the sun overhead)
    return par, mu0


def make_mode_case(pool, nquad):
    C, nphi = MODE_CASES[nquad]
    N, nb = nquad // 2, nquad
    nodes, _ = double_gauss(N)
    par, mu0 = mode_columns(nquad)
    mups = [np.concatenate((nodes, [mu0[c]])) for c in range(C)]
    jobs = [(tuple(par[c]), nodes[i], mups[c][j], float(cluster_b(par[c, 0], nodes[i], mups[c][j])), nphi, nb)
            for c in range(C) for i in range(N) for j in range(N + 1)]
    res = np.array(pool.map(_mode_row, jobs, chunksize=4)).reshape(C, N, N + 1, nb).transpose(0, 3, 1, 2)
    q, q0 = res[..., :N].copy(), res[..., N].copy()

    def numpy_rule(n_nodes):
        full = np.stack([rule_numpy(tuple(par[c]), nodes[:, None], mups[c][None, :], n_nodes, nb) for c in range(C)])
        return full[..., :N], full[..., N]

    gq, gq0 = numpy_rule(nphi)
    d = max(float(np.max(np.abs(gq - q) / ((np.where(np.arange(nb) == 0, 1.0, 2.0))[None, :, None, None] * q[:, :1]))),
            float(np.max(np.abs(gq0 - q0) / ((np.where(np.arange(nb) == 0, 1.0, 2.0))[None, :, None] * q0[:, :1]))))
    cq, cq0 = numpy_rule(4096)
    fig = max(float(np.max(np.abs(q - cq) / np.max(np.abs(cq), axis=1, keepdims=True))),
              float(np.max(np.abs(q0 - cq0) / np.max(np.abs(cq0), axis=1, keepdims=True))))
    # adaptive quadrature of the uniform-dphi integral for a few pairs of column 0: (i, j) = grazing, mixed, steep
    from scipy.integrate import quad
    pairs = [(0, 0), (0, N - 1), (N - 1, N - 1), (N // 2, N // 2)]
    adaptive = np.empty((len(pairs), min(nb, 8)))
    for k, (i, j) in enumerate(pairs):
        bw = float(cluster_b(par[0, 0], nodes[i], nodes[j]))
        for m in range(adaptive.shape[1]):
            f = lambda t: float(rho_numpy(tuple(par[0]), nodes[i], nodes[j], np.cos(t), np.sin(t))) * np.cos(m * t)  # noqa: E731
            val = quad(f, 0.0, np.pi, points=[bw, 4 * bw, 16 * bw, min(64 * bw, 3.0)], epsabs=1e-13, epsrel=1e-13, limit=2000)[0]
            adaptive[k, m] = val * (1.0 if m == 0 else 2.0) / np.pi
    return dict(params=np.concatenate((par, np.zeros((C, 1))), axis=1), mu0=mu0, mu=nodes, nphi=np.int32(nphi), q=q, q0=q0, q_conv=cq, q0_conv=cq0,
                np_dist_modes=np.array([d]), conv_fig=np.array([fig]), adaptive_pairs=np.array(pairs), adaptive=adaptive)


def convergence():
    """Worst |q^m(nphi) - q^m(4096)| over each pair's own max_m |q^m|, every mode m < min(64, ...) = NBDRF 64, NumPy float64."""
    out = {}
    for nquad in STREAMS:
        nodes, wts = double_gauss(nquad // 2)
        row = {}
        for U in WINDS:
            par = (U, N_REFR, 0.0)
            ref = rule_numpy(par, nodes[:, None], nodes[None, :], 4096, 64)
            den = np.max(np.abs(ref), axis=0, keepdims=True)
            cell = {str(n): float(np.max(np.abs(rule_numpy(par, nodes[:, None], nodes[None, :], n, 64) - ref) / den)) for n in (256, 512)}
            other = rule_numpy(par, nodes[:, None], nodes[None, :], 2048, 64)
            cell["2048_vs_4096"] = float(np.max(np.abs(other - ref) / den))
            cell["albedo_max"] = float(np.max(np.sum(2 * nodes[None, :] * wts[None, :] * ref[0], axis=1)))
            row[f"U={U:g}"] = cell
            print(nquad, U, cell, flush=True)
        out[str(nquad)] = row
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    prof = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
    if "--convergence" in sys.argv or "--only-convergence" in sys.argv:
        prof["convergence"] = dict(
            what="clustered rule dphi = psi - a sin psi: worst |q^m(nphi) - q^m(4096)| over the pairs of nodes and ALL modes m < 64, of each "
                 "pair's own max_m |q^m|; n = 1.34, shadowing on, NumPy float64 (its rounding floor is ~1e-13 at 64 streams); 2048_vs_4096 "
                 "shows the reference itself converged; albedo_max: the largest hemispherical albedo over the nodes. The front end's "
                 "default nphi = 512 follows this table.",
            streams=convergence())
        json.dump(prof, open(PROFILE, "w"), indent=1)
        if "--only-convergence" in sys.argv:
            return
    with Pool() as pool:
        files = {}
        for nquad in STREAMS:
            for U in WINDS:
                name = f"rho_U{int(U)}_n{nquad}.npz"
                files[name] = make_rho_case(pool, U, nquad)
                print(name, "np_dist", files[name]["np_dist"], "albedo max", files[name]["albedo"].max(), flush=True)
        worst = np.max(np.array([d["np_dist"] for d in files.values()]), axis=0)
        print("np_dist_all", worst)
        for name, d in files.items():
            np.savez_compressed(os.path.join(OUT, name), np_dist_all=worst, **d)
        for nquad in STREAMS:
            d = make_mode_case(pool, nquad)
            print(f"modes_n{nquad}: np_dist_modes {d['np_dist_modes']}, conv_fig {d['conv_fig']}", flush=True)
            k = d["adaptive"].shape[1]
            pr = d["adaptive_pairs"]
            print("  adaptive - q_conv:", np.max(np.abs(d["adaptive"] - d["q_conv"][0, :k, pr[:, 0], pr[:, 1]])), flush=True)
            np.savez_compressed(os.path.join(OUT, f"modes_n{nquad}.npz"), **d)


if __name__ == "__main__":
    main()
