#!/usr/bin/env python3
"""Fixtures tests/golden/nt/*.npz: the Nakajima-Tanaka corrections (TMS + IMS; value, tau-antiderivative, tau-derivative) of
tools/nt_truth.py -- a 40-digit closed-form evaluation that shares no code with oracle/ or the package -- at the shapes where
rtd_nt_tables_kernel / rtd_nt_apply_kernel can still go wrong (the table in CASES below says what each one is there for).

Each fixture holds the inputs (keyword arguments of pydisort / pydisort_batch), the points ``tau`` and ``phi``, the three truth
arrays ``truth_<order>`` [NQuad, ntau, nphi] ([C, ...] for the batch), and ``oracle_max_u`` [3]: max|u| of the float64 oracle
without corrections at those points, per order.  A fixture whose max|correction| is below 1e-4 of that max|u| is refused:
a correction lost under u tests nothing.  (The tp_* fixtures take the inputs of a test problem as they are and are exempt; only
the antiderivative of 4a falls below, at 3e-8 of u: the GPU test resolves it only as far as the rounding of u allows.)  Needs numpy and mpmath (and the repository's oracle for max|u|); the reference is not
used -- except that, when PYDISORT_REFERENCE_SRC names the directory that holds the reference's package, q32_L20_thick records
whether the reference's own corrected u is finite there (``reference_nonfinite`` = number of non-finite values, ``reference_size``);
without it those two numbers are carried over from the committed fixture.

Usage:  python tests/golden/make_nt_truth_goldens.py [--check] [names ...]
        --check: recompute and compare with the committed fixtures bit for bit instead of writing.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import nt_truth  # noqa: E402

OUT = os.path.join(HERE, "nt")
ORDERS = nt_truth.ORDERS
ORDER_KW = dict(value={}, antiderivative=dict(is_antiderivative_wrt_tau=True), derivative=dict(is_derivative_wrt_tau=True))
INPUTS = ("tau_arr", "omega_arr", "NQuad", "Leg_coeffs_all", "mu0", "I0", "phi0", "f_arr", "NLeg", "NFourier")
PHI = np.array([0.0, 0.7, 3.0])
MIN_CORRECTION = 1e-4  # of the oracle's max|u|


def points(tau_arr):
    """tau = 0; the first three interfaces, one in the middle, the last interior one; the bottom; three interior points; one
    point 1e-12 (relative) beyond an interface; one point twice; all of it unsorted."""
    t = np.atleast_1d(np.asarray(tau_arr, float))
    L = len(t)
    top = np.concatenate(([0.0], t[:-1]))
    interfaces = sorted({min(k, L - 1) for k in (0, 1, 2, L // 2, L - 2, L - 1) if k >= 0})
    interior = sorted({0, L // 2, L - 1})
    fr = (0.37, 0.5, 0.81)
    pts = [0.0] + [t[k] for k in interfaces] + [top[l] + fr[j % 3] * (t[l] - top[l]) for j, l in enumerate(interior)]
    if L == 1:
        pts += [0.11 * t[0], 0.93 * t[0]]
    else:
        pts.append(t[(L - 1) // 2] * (1 + 1e-12))
    pts.append(pts[len(pts) // 2])
    pts = np.array(pts)
    return pts[np.random.RandomState(len(pts)).permutation(len(pts))]


def hg(g, n):
    return np.asarray(g, float)[..., None] ** np.arange(n)


def column(tau_arr, omega, g, NQuad, nall, mu0, I0=1.0, phi0=0.0, NLeg=None, NFourier=None, f=None):
    tau_arr, omega, g = (np.atleast_1d(np.asarray(v, float)) for v in (tau_arr, omega, g))
    NLeg = NQuad if NLeg is None else NLeg
    leg = hg(np.broadcast_to(g, tau_arr.shape), nall)
    return dict(tau_arr=tau_arr, omega_arr=np.broadcast_to(omega, tau_arr.shape).copy(), NQuad=NQuad, Leg_coeffs_all=leg,
                mu0=float(mu0), I0=float(I0), phi0=float(phi0), f_arr=leg[:, NLeg].copy() if f is None else np.asarray(f, float),
                NLeg=NLeg, NFourier=NQuad if NFourier is None else NFourier)


def q6_L1():
    return column([0.8], 0.9, 0.75, 6, 7, 1.0, I0=2.0, phi0=0.4)


def q10_L2_low_sun():
    return column([0.02, 0.05], [0.95, 0.8], [0.8, 0.7], 10, 40, 0.01, I0=1.5, phi0=2.0)


def q16_L7_mixed():
    kw = column(np.cumsum([0.2, 0.5, 0.1, 0.7, 0.3, 0.4, 0.6]), [0.9, 0.0, 0.8, 0.95, 0.6, 0.99, 0.7],
                [0.8, 0.75, 0.85, 0.7, 0.82, 0.78, 0.8], 16, 40, 0.7, I0=3.0, phi0=1.0, NLeg=12, NFourier=5)
    kw["f_arr"][[2, 5]] = 0.0
    return kw


def q16_L50():
    k = np.arange(50)
    return column(np.cumsum(0.45 + 0.3 * np.cos(0.9 * k) ** 2), 0.55 + 0.44 * np.sin(0.37 * k) ** 2, 0.7 + 0.15 * np.cos(0.53 * k) ** 2,
                  16, 60, 0.8, I0=2.0, phi0=0.3)


def q18_L3():
    return column([0.4, 1.1, 2.0], [0.9, 0.7, 0.97], [0.85, 0.8, 0.87], 18, 80, 0.55, I0=1.0, phi0=0.9)


def q34_L3():
    return column([0.3, 1.0, 1.8], [0.92, 0.75, 0.98], [0.9, 0.88, 0.91], 34, 140, 0.45, I0=2.5, phi0=5.0)


def q66_L2():
    return column([0.5, 1.4], [0.95, 0.85], [0.94, 0.945], 66, 240, 0.65, I0=1.0, phi0=1.7, NFourier=20)


def q32_L20_cloud():
    k = np.arange(20)
    kw = column(np.cumsum(0.1 + 0.25 * np.sin(0.7 * k) ** 2), 0.7 + 0.29 * np.cos(0.41 * k) ** 2, 0.9 + 0.045 * np.sin(0.3 * k) ** 2,
                32, 300, 0.6, I0=3.0, phi0=0.5)
    return kw


def q32_L20_thick():
    k = np.arange(20)
    return column(np.cumsum(13.4 * (1 + 0.5 * np.cos(1.3 * k))) * (268.0 / np.sum(13.4 * (1 + 0.5 * np.cos(1.3 * k)))),
                  0.6 + 0.39 * np.sin(0.61 * k) ** 2, 0.9 + 0.03 * np.cos(0.47 * k), 32, 150, 0.5, I0=1.0, phi0=0.0)


def q64_L5():
    return column(np.cumsum([0.2, 0.6, 0.3, 0.8, 0.5]), [0.9, 0.99, 0.7, 0.95, 0.8], [0.935, 0.94, 0.938, 0.945, 0.936], 64, 240,
                  0.35, I0=2.0, phi0=2.2)


def q128_L2():
    return column([0.6, 1.5], [0.97, 0.9], [0.97, 0.968], 128, 420, 0.75, I0=1.0, phi0=0.2, NFourier=16)


def _near_node_base():
    return dict(tau_arr=np.cumsum([0.3, 0.7, 0.4, 1.1]), omega=[0.9, 0.8, 0.97, 0.6], g=[0.8, 0.82, 0.78, 0.85])


def q16_L4_mu0_near_node():
    b = _near_node_base()
    node = nt_truth.quadrature_nodes(8)[5]
    return column(b["tau_arr"], b["omega"], b["g"], 16, 50, node * (1 + 1e-6), I0=2.0, phi0=1.2)


def q16_L4_smu0_near_node():
    """mu0 such that the IMS-scaled mu0 / (1 - omega_avg f_avg) is a quadrature node times (1 + 1e-5)."""
    b = _near_node_base()
    kw = column(b["tau_arr"], b["omega"], b["g"], 16, 50, 0.5, I0=2.0, phi0=1.2)
    w = kw["omega_arr"] * kw["tau_arr"]
    of = w.sum() / kw["tau_arr"].sum() * ((kw["f_arr"] * w).sum() / w.sum())
    kw["mu0"] = float(nt_truth.quadrature_nodes(8)[5] * (1 + 1e-5) * (1 - of))
    return kw


def _tp(name):
    def make():
        import goldens
        call = goldens.load(name)[0]
        kw = {k: call["kwargs"][k] for k in INPUTS if call["kwargs"].get(k) is not None}
        kw["tau_arr"] = np.atleast_1d(np.asarray(kw["tau_arr"], float))
        L = len(kw["tau_arr"])
        kw["omega_arr"] = np.broadcast_to(np.asarray(kw["omega_arr"], float), (L,)).copy()
        kw["f_arr"] = np.broadcast_to(np.asarray(kw["f_arr"], float), (L,)).copy()
        kw["Leg_coeffs_all"] = np.atleast_2d(np.asarray(kw["Leg_coeffs_all"], float))
        kw.setdefault("NLeg", kw["NQuad"])
        kw.setdefault("NFourier", kw["NQuad"])
        ev = next(e for e in call["evals"] if e["name"] == "u" and not e["kwargs"] and len(e["args"]) == 2)
        return kw, np.atleast_1d(ev["args"][0]).astype(float), np.atleast_1d(ev["args"][1]).astype(float)
    return make


def batch7_q16_L6():
    """Seven columns, every input different per column."""
    rs = np.random.RandomState(7)
    C, L, NQuad, nall = 7, 6, 16, 48
    cols = [column(np.cumsum(rs.uniform(0.1, 0.9, L)), rs.uniform(0.3, 0.99, L), rs.uniform(0.7, 0.88, L), NQuad, nall,
                   rs.uniform(0.15, 0.95), I0=rs.uniform(0.5, 4.0), phi0=rs.uniform(0, 6.0)) for _ in range(C)]
    return cols


# name -> (builder, azimuths, what it is there for)
CASES = {
    "q6_L1": (q6_L1, PHI, "no tables (L > 1 guard), dd >= 0 for every stream, the minimal nleg_all - NLeg; N = 3 in NP = 4"),
    "q10_L2_low_sun": (q10_L2_low_sun, PHI, "dd < 0 for every stream, smallest table; N = 5 in NP = 8"),
    "q16_L7_mixed": (q16_L7_mixed, PHI, "per-layer 1 - f, omega = 0 layer, f = 0 layers among f > 0, NLeg < NQuad, NFourier < NLeg"),
    "q16_L50": (q16_L50, PHI, "the O(L^2) loops at the deepest workload depth, total tau ~ 30"),
    "q18_L3": (q18_L3, PHI, "first stream count of the 16-row padding class (N = 9): d.NP stride against d.N rows"),
    "q34_L3": (q34_L3, PHI, "first stream count of the 32-row padding class (N = 17)"),
    "q66_L2": (q66_L2, PHI, "first stream count of the 64-row padding class (N = 33)"),
    "q32_L20_cloud": (q32_L20_cloud, np.array([0.0, 0.7, 3.0, 4.4, 6.0]),
                      "300 moments: long forward Legendre recurrence; Q nphi = 160 > the 128 threads of the apply kernel"),
    "q32_L20_thick": (q32_L20_thick, PHI, "total tau 268: the reference's cumulative sums divide by an underflowed product"),
    "q64_L5": (q64_L5, PHI, "end of the tuned range"),
    "q128_L2": (q128_L2, PHI, "end of the wide range"),
    "q16_L4_mu0_near_node": (q16_L4_mu0_near_node, PHI, "mu0 = node (1 + 1e-6): TMS cancellation att - e against mu0 / (mu0 - mu)"),
    "q16_L4_smu0_near_node": (q16_L4_smu0_near_node, PHI, "mu0 / (1 - omega_avg f_avg) = node (1 + 1e-5): IMS chi cancellation (1 / x^2)"),
    "tp_4a": (_tp("4a"), None, "test problem 4a at its golden's points: three-way with the reference's captured output"),
    "tp_4b": (_tp("4b"), None, "test problem 4b"),
    "tp_5a": (_tp("5a"), None, "test problem 5a"),
    "tp_5b": (_tp("5b"), None, "test problem 5b"),
    "batch7_q16_L6": (batch7_q16_L6, PHI, "per-column offsets of R, wfull, ims_par; window_nt with work_columns = 3"),
}


def _oracle_max_u(kw, tau, phi):
    from oracle import disort_oracle as O
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        u = O.pydisort(**dict(kw, NT_cor=False))[4]
        return np.array([np.max(np.abs(u(tau, phi, **ORDER_KW[o]))) for o in ORDERS])


def _reference_nonfinite(kw, tau, phi):
    src = os.environ.get("PYDISORT_REFERENCE_SRC")
    if not src:
        return None
    sys.path.insert(0, src)
    import PythonicDISORT
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        u = PythonicDISORT.pydisort(**dict(kw, NT_cor=True))[4](tau, phi)
    return np.array(int(np.sum(~np.isfinite(u)))), np.array(int(np.size(u)))


def build(name):
    """-> dict of arrays, exactly what the fixture file holds."""
    make, phi, _ = CASES[name]
    made = make()
    if isinstance(made, tuple):
        made, tau, phi = made
    else:
        tau = None
    cols = made if isinstance(made, list) else [made]
    taus = [points(kw["tau_arr"]) if tau is None else tau for kw in cols]
    truths = [nt_truth.correction(kw, t, phi) for kw, t in zip(cols, taus)]
    maxu = [_oracle_max_u(kw, t, phi) for kw, t in zip(cols, taus)]
    for kw, tr, mu_ in zip(cols, truths, maxu):
        for j, o in enumerate(ORDERS):
            ratio = np.max(np.abs(tr[o])) / mu_[j]
            if not ratio >= MIN_CORRECTION and not name.startswith("tp_"):  # (a test problem's inputs are not ours to choose)
                raise SystemExit(f"{name}: max|correction| of the {o} is {ratio:.2e} of max|u|: too small to test anything")
    stack = (lambda v: np.stack(v)) if isinstance(made, list) else (lambda v: v[0])
    res = {k: stack([np.asarray(kw[k]) for kw in cols]) for k in INPUTS}
    for k in ("NQuad", "NLeg", "NFourier"):
        res[k] = np.array(int(cols[0][k]))
    res.update(tau=stack(taus), phi=np.asarray(phi, float), oracle_max_u=stack(maxu), batch=np.array(int(isinstance(made, list))))
    for o in ORDERS:
        res["truth_" + o] = stack([tr[o] for tr in truths])
    if name == "q32_L20_thick":
        r = _reference_nonfinite(cols[0], taus[0], phi)
        if r is None:
            z = np.load(os.path.join(OUT, name + ".npz"))
            r = z["reference_nonfinite"], z["reference_size"]
        res["reference_nonfinite"], res["reference_size"] = r
    return res


def main(argv):
    check = "--check" in argv
    names = [a for a in argv if not a.startswith("--")] or list(CASES)
    os.makedirs(OUT, exist_ok=True)
    bad = 0
    for name in names:
        res = build(name)
        path = os.path.join(OUT, name + ".npz")
        if check:
            z = np.load(path)
            same = sorted(z.files) == sorted(res) and all(
                z[k].shape == np.shape(res[k]) and z[k].tobytes() == np.asarray(res[k]).astype(z[k].dtype).tobytes() for k in res)
            print(f"{name}: {'identical' if same else 'DIFFERENT'}", flush=True)
            bad += not same
        else:
            np.savez_compressed(path, **res)
            big = max(np.max(np.abs(res["truth_" + o])) / np.max(np.atleast_2d(res["oracle_max_u"])[:, j]) for j, o in enumerate(ORDERS))
            print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB, max|correction| up to {big:.2e} of max|u|", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
