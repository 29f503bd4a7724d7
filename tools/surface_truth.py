#!/usr/bin/env python3
"""Truth of the parametric surface models (csrc/rtd_surface.h) and the fixtures tests/golden/surface/*.npz.

The formulas of include/rtd.h (rtd_surface) are evaluated in 50-digit arithmetic (mpmath) from the float64 inputs -- cosines, parameters
and the azimuth 2 pi p / nphi as an exact rational times pi -- as samples rho(mu, mu', dphi_p) and as the trapezoid modes
    q^m = (2 - delta_m0) / nphi  sum_p rho_p cos(2 pi m p / nphi),
and rounded once to float64.  Cases: two parameter sets each of Hapke, Ross-Li (one of them with rows the clamp at 0 cuts) and RPV;
mu = the double-Gauss nodes of 6, 16 and 34 streams with nphi = 16, 64 and 40; mu' = those nodes, 0.5, one value equal to a node, 1.0.

Next to each truth the file holds the MODEL DISTANCE: the worst distance of a plain NumPy float64 evaluation of the same formulas from
it -- samples relative to the row's max |rho| (`scale`, a row = one pair of cosines over the azimuths), modes relative to
sum_p |rho_p| (2 - delta) / nphi -- measured WITHOUT Ross-Li's clamp, and the worst such distance over all files (`np_dist_all`).
The tests allow the header's routine and the device 16 x np_dist_all[0] of `scale`: device libm and FMA contraction differ from
NumPy's by a few ulp per call, while the mistakes to catch are far larger (the arccos form of the phase angle: 8e-8; a wrong azimuth
convention: O(1)).  The clamp is 1-Lipschitz, so a bound on the unclamped values holds for the clamped ones; `scale` is that of the
unclamped row so that a row the clamp cuts to zero keeps a meaningful tolerance.

--convergence also records max |q^m(nphi) - adaptive integral| for nphi = 256, 1024, 4096 (scipy.integrate.quad_vec, as the
reference's tests integrate; float64) into profiles/surface.json: the stated convergence of the default nphi.  The models' cusp at the
hot spot (tan(xi / 2) and sqrt(D^2) behave like |dphi - pi| on the diagonal mu = mu') makes the trapezoid rule algebraic there: the
recorded errors fall by 16 per factor 4 in nphi, 1 / nphi^2; off the diagonal Hapke and RPV converge spectrally.

Usage: python tools/surface_truth.py [--convergence]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "surface")
PROFILE = os.path.join(ROOT, "profiles", "surface.json")
MODEL_ID = {"lambert": 0, "hapke": 1, "rossli": 2, "rpv": 3}
CASES = {
    "hapke": [(1.0, 0.06, 0.6), (0.4, 0.2, 0.95)],
    "rossli": [(0.3, 0.1, 0.05), (0.2, 0.15, 0.01)],  # the first: rows at the grazing nodes are cut by the clamp
    "rpv": [(0.1, 0.8, -0.1, 0.1), (0.3, 1.2, 0.25, 0.6)],
}
GRIDS = [(6, 16), (16, 64), (34, 40)]  # (streams, nphi)
NMODES = 6


def double_gauss(N):
    x, w = np.polynomial.legendre.leggauss(N)
    return np.sort((x + 1) / 2)


def cs(nphi):
    """cos and sin of 2 pi p / nphi with the argument reduced exactly (what cospi / sinpi do)."""
    x = 2.0 * np.arange(nphi) / nphi
    q = np.floor(2 * x + 0.5).astype(int)
    r = x - 0.5 * q
    cr, sr = np.cos(np.pi * r), np.sin(np.pi * r)
    c = np.choose(q & 3, [cr, -sr, -cr, sr])
    s = np.choose(q & 3, [sr, cr, -sr, -cr])
    return c, s


def rho_numpy(model, par, mu, mup, c, s, clamp=True):
    """The formulas of csrc/rtd_surface.h in NumPy float64 (broadcasting)."""
    par = list(par) + [0.0] * (4 - len(par))
    sm, sp = np.sqrt((1 - mu) * (1 + mu)), np.sqrt((1 - mup) * (1 + mup))
    h = 0.5 * ((sm * c + sp) ** 2 + (sm * s) ** 2 + (mu - mup) ** 2)
    g = 0.5 * ((sm * c - sp) ** 2 + (sm * s) ** 2 + (mu + mup) ** 2)
    cosxi = 1 - h
    if model == "hapke":
        B0, HH, W = par[:3]
        B = B0 * HH / (HH + np.sqrt(h / g))
        gam = np.sqrt(1 - W)
        H0, H = (1 + 2 * mup) / (1 + 2 * mup * gam), (1 + 2 * mu) / (1 + 2 * mu * gam)
        return W / 4 / (mu + mup) * ((1 + B) * (1 + cosxi / 2) + H0 * H - 1)
    ti, tv, sec = sm / mu, sp / mup, 1 / mu + 1 / mup
    D2 = (ti - tv) ** 2 + 2 * ti * tv * (1 + c)
    if model == "rossli":
        xi = 2 * np.arcsin(np.sqrt(0.5 * h))
        Kvol = ((np.pi / 2 - xi) * cosxi + np.sqrt(h * g)) / (mu + mup) - np.pi / 4
        cost = np.minimum(1.0, 2 * np.sqrt(D2 + (ti * tv * s) ** 2) / sec)
        t = np.arccos(cost)
        O = (t - np.sqrt((1 - cost) * (1 + cost)) * cost) * sec / np.pi
        Kgeo = O - sec + g / (2 * mu * mup)
        r = par[0] + par[1] * Kvol + par[2] * Kgeo
        return np.maximum(0.0, r) if clamp else r
    rho0, k, Th, rhoc = par
    den = (1 + Th) ** 2 - 2 * Th * h if Th <= 0 else (1 - Th) ** 2 + 2 * Th * g
    return rho0 * (mu * mup * (mu + mup)) ** (k - 1) * (1 - Th) * (1 + Th) / (den * np.sqrt(den)) * (1 + (1 - rhoc) / (1 + np.sqrt(D2)))


def rho_mp(mp, model, par, mu, mup, p, nphi):
    """One sample in mpmath, from the formulas as include/rtd.h states them; unclamped."""
    mpf = mp.mpf
    par = [mpf(float(v)) for v in par] + [mpf(0)] * (4 - len(par))
    mu, mup = mpf(float(mu)), mpf(float(mup))
    ang = 2 * mp.pi * mpf(p) / mpf(nphi)
    c, s = mp.cos(ang), mp.sin(ang)
    sm, sp = mp.sqrt(1 - mu * mu), mp.sqrt(1 - mup * mup)
    cosxi = mu * mup - sm * sp * c
    h = 1 - cosxi
    if model == "hapke":
        B0, HH, W = par[:3]
        t2 = mp.sqrt(h / (2 - h))
        B = B0 * HH / (HH + t2)
        gam = mp.sqrt(1 - W)
        H0, H = (1 + 2 * mup) / (1 + 2 * mup * gam), (1 + 2 * mu) / (1 + 2 * mu * gam)
        return W / 4 / (mu + mup) * ((1 + B) * (1 + cosxi / 2) + H0 * H - 1)
    ti, tv, sec = sm / mu, sp / mup, 1 / mu + 1 / mup
    D2 = (ti - tv) ** 2 + 2 * ti * tv * (1 + c)
    if D2 < 0:
        D2 = mpf(0)
    if model == "rossli":
        xi = 2 * mp.asin(mp.sqrt(h / 2))
        sinxi = mp.sqrt(h * (2 - h))
        Kvol = ((mp.pi / 2 - xi) * cosxi + sinxi) / (mu + mup) - mp.pi / 4
        cost = 2 * mp.sqrt(D2 + (ti * tv * s) ** 2) / sec
        if cost > 1:
            cost = mpf(1)
        t = mp.acos(cost)
        O = (t - mp.sin(t) * cost) * sec / mp.pi
        Kgeo = O - sec + (1 + cosxi) / (2 * mu * mup)
        return par[0] + par[1] * Kvol + par[2] * Kgeo
    rho0, k, Th, rhoc = par
    return rho0 * (mu * mup * (mu + mup)) ** (k - 1) * (1 - Th * Th) / (1 + Th * Th + 2 * Th * cosxi) ** mpf("1.5") \
        * (1 + (1 - rhoc) / (1 + mp.sqrt(D2)))


def make_case(mp, model, par, nquad, nphi):
    N = nquad // 2
    mu = double_gauss(N)
    mup = np.concatenate((mu, [0.5, mu[N // 2], 1.0]))
    clamp = model == "rossli"
    raw = [[[rho_mp(mp, model, par, a, b, p, nphi) for p in range(nphi)] for b in mup] for a in mu]
    cosm = [[mp.cos(2 * mp.pi * mp.mpf((m * p) % nphi) / nphi) for p in range(nphi)] for m in range(NMODES)]

    def modes(rows):  # [N][N'][nphi] of mpf -> [NMODES][N][N']
        return [[[sum(r * cm for r, cm in zip(row, cosm[m])) * (1 if m == 0 else 2) / nphi for row in rr] for rr in rows] for m in range(NMODES)]

    cut = [[[max(v, mp.mpf(0)) for v in row] for row in rr] for rr in raw] if clamp else raw
    f64 = lambda a: np.array([[[float(v) for v in row] for row in rr] for rr in a])  # noqa: E731
    rho_u, rho = f64(raw), f64(cut)
    q = f64(modes(cut))
    scale = np.max(np.abs(rho_u), axis=2)
    # the model distance: NumPy float64 against the truth, unclamped
    c, s = cs(nphi)
    got = rho_numpy(model, par, mu[:, None, None], mup[None, :, None], c[None, None, :], s[None, None, :], clamp=False)
    # (the difference is formed in mpmath: rho_u is the truth rounded, which would add half an ulp)
    d_s = max(float(abs(mp.mpf(float(got[i, j, p])) - raw[i][j][p])) / scale[i, j] for i in range(N) for j in range(len(mup)) for p in range(nphi))
    ctab = np.array([[float(v) for v in row] for row in cosm])
    q_np = np.einsum("ijp,mp->mij", got, ctab) * np.where(np.arange(NMODES) == 0, 1.0, 2.0)[:, None, None] / nphi
    l1 = np.sum(np.abs(rho_u), axis=2) / nphi
    qm = modes(raw)
    d_m = max(float(abs(mp.mpf(float(q_np[m, i, j])) - qm[m][i][j])) / (l1[i, j] * (1 if m == 0 else 2))
              for m in range(NMODES) for i in range(N) for j in range(len(mup)))
    p4 = np.zeros(4)
    p4[:len(par)] = par
    return dict(model=np.int32(MODEL_ID[model]), params=p4, mu=mu, mup=mup, nphi=np.int32(nphi), rho=rho, scale=scale, q=q, np_dist=np.array([d_s, d_m]), rows_cut=np.int32(np.sum(np.all(rho == 0.0, axis=2))))


def convergence():
    """max |q^m(nphi) - adaptive integral| over m < 8 and the 16-stream nodes, per model (first parameter set; NumPy float64)."""
    from scipy.integrate import quad_vec
    mu = double_gauss(8)
    out = {}
    for model, sets in CASES.items():
        par = sets[0]
        m = np.arange(8)[:, None, None]

        def f(phi):
            return rho_numpy(model, par, mu[None, :, None], mu[None, None, :], np.cos(phi), np.sin(phi)) * np.cos(m * phi)

        ref = quad_vec(f, 0, 2 * np.pi, points=[np.pi], epsabs=1e-13, epsrel=1e-13, limit=2000)[0] / (np.pi * np.where(m == 0, 2.0, 1.0))
        row = {}
        for nphi in (256, 1024, 4096):
            c, s = cs(nphi)
            r = rho_numpy(model, par, mu[:, None, None], mu[None, :, None], c, s)
            ct = np.cos(2 * np.pi * ((np.arange(8)[:, None] * np.arange(nphi)[None, :]) % nphi) / nphi)
            q = np.einsum("ijp,mp->mij", r, ct) * np.where(np.arange(8) == 0, 1.0, 2.0)[:, None, None] / nphi
            err = np.abs(q - ref)
            diag = np.max(err[:, np.arange(8), np.arange(8)])
            off = np.max(err - 10 * np.eye(8)[None])  # (the diagonal excluded)
            row[str(nphi)] = dict(max_abs_err=float(np.max(err)), diagonal=float(diag), off_diagonal=float(off), max_abs_q=float(np.max(np.abs(ref))))
        out[model] = dict(params=list(par), streams=16, modes=8, nphi=row)
    return out


def main():
    import mpmath as mp
    mp.mp.dps = 50
    os.makedirs(OUT, exist_ok=True)
    files = {}
    for model, sets in CASES.items():
        for k, par in enumerate(sets):
            for nquad, nphi in GRIDS:
                name = f"{model}{k}_n{nquad}.npz"
                files[name] = make_case(mp, model, par, nquad, nphi)
                print(name, "np_dist", files[name]["np_dist"], "rows cut", int(files[name]["rows_cut"]), flush=True)
    worst = np.max(np.array([d["np_dist"] for d in files.values()]), axis=0)
    print("np_dist_all", worst)
    for name, d in files.items():
        np.savez_compressed(os.path.join(OUT, name), np_dist_all=worst, **d)
    if "--convergence" in sys.argv:
        prof = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
        prof["convergence"] = dict(
            what="max |q^m(nphi) - adaptive integral| (scipy quad_vec, float64) over the modes m < 8 at the 16-stream nodes; the "
                 "diagonal mu = mu' holds the hot-spot cusp, where the trapezoid rule converges algebraically",
            np_dist_all=dict(samples=float(worst[0]), modes=float(worst[1])), models=convergence())
        json.dump(prof, open(PROFILE, "w"), indent=1)
        print(json.dumps(prof["convergence"], indent=1))


if __name__ == "__main__":
    main()
