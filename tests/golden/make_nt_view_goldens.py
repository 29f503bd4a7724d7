#!/usr/bin/env python3
"""Fixtures tests/golden/nt_view/*.npz: the Nakajima-Tanaka corrections (TMS + IMS; value, tau-antiderivative, tau-derivative) at
VIEWING ANGLES, from the 40-digit closed form of tools/nt_view_truth.py (divided-difference form), at the smallest shapes that reach
every branch of rtd_nt_view_tables_kernel / rtd_nt_view_apply_kernel and of csrc/rtd_nt_view.h.

Inputs are those of tests/golden/nt where a fixture of that shape exists (CASES says which and why); ``batch6_q16_L3`` is new: six
columns that differ in every input, 16 streams x 3 layers, 12 moments with NLeg = 8.

Angles of every column (ANGLES below; those beyond +-1 are dropped, which happens for mu0 = 1 only):
    two per hemisphere in general position; one exact node per hemisphere; +-1; +-mu0 exactly; -mu0 (1 +- 1e-9);
    -s and -s (1 + 1e-9), s = the IMS scaled mu0 of the truth rounded to float64 (the device's own ims_par[0] differs from it in the
    last bits: the GPU test adds that one at run time); -1e-3.
Points: tau = 0, the first interface (it belongs to the top layer), an interior point of the middle layer, the bottom; for one layer
0, two interior points and the bottom.  Azimuths: phi0 of the (first) column and 2.1.

Each file holds the inputs (keyword arguments of pydisort / pydisort_batch), ``mu`` [nmu] ([C, nmu] for the batch), ``tau``, ``phi``,
``batch`` and ``truth_<order>`` [nmu, ntau, nphi] ([C, ...] for the batch).  Needs numpy and mpmath only.

Usage:  python tests/golden/make_nt_view_goldens.py [--check] [names ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import mpmath as mp  # noqa: E402
import nt_truth  # noqa: E402
import nt_view_truth  # noqa: E402

OUT = os.path.join(HERE, "nt_view")
NT = os.path.join(HERE, "nt")
ORDERS = nt_view_truth.ORDERS
INPUTS = ("tau_arr", "omega_arr", "NQuad", "Leg_coeffs_all", "mu0", "I0", "phi0", "f_arr", "NLeg", "NFourier")


def from_nt(name):
    def make():
        z = np.load(os.path.join(NT, name + ".npz"))
        assert not bool(z["batch"])
        return {k: (int(z[k]) if k in ("NQuad", "NLeg", "NFourier") else float(z[k]) if z[k].ndim == 0 else np.array(z[k])) for k in INPUTS}
    return make


def batch6_q16_L3():
    rs = np.random.RandomState(63)
    C, L, NQuad, NLeg, nall = 6, 3, 16, 8, 12
    cols = []
    for _ in range(C):
        g = rs.uniform(0.7, 0.86, L)
        leg = g[:, None] ** np.arange(nall)
        cols.append(dict(tau_arr=np.cumsum(rs.uniform(0.15, 0.9, L)), omega_arr=rs.uniform(0.4, 0.99, L), NQuad=NQuad, Leg_coeffs_all=leg,
                         mu0=float(rs.uniform(0.2, 0.8)), I0=float(rs.uniform(0.5, 4.0)), phi0=float(rs.uniform(0, 6.0)),
                         f_arr=leg[:, NLeg].copy(), NLeg=NLeg, NFourier=NLeg))
    return cols


# name -> (builder, what it is there for)
CASES = {
    "q6_L1": (from_nt("q6_L1"), "6 streams x 1 layer: no other-layer term; mu0 = 1, so -mu0 = -1 meets sqrt(1 - mu^2) = 0 and the phi1 limit at once"),
    "batch6_q16_L3": (batch6_q16_L3, "six columns, per-column angles, window offsets; points in the top, middle and bottom layer; 12 moments"),
    "q34_L3": (from_nt("q34_L3"), "34 streams: N = 17 in the 32-row padding class (the basis and the node rows against d.NP)"),
    "q16_L4_mu0_near_node": (from_nt("q16_L4_mu0_near_node"), "mu0 = node (1 + 1e-6): the exact node is then a near-coincidence of the TMS factor too"),
    "q16_L4_smu0_near_node": (from_nt("q16_L4_smu0_near_node"), "scaled mu0 = node (1 + 1e-5): the exact node is a near-coincidence of chi"),
    "q32_L20_cloud": (from_nt("q32_L20_cloud"), "300 moments, 20 layers: the long recurrence with three series side by side, deep prefix / suffix sums"),
}


def scaled_mu0(kw):
    """The IMS scaled mu0 (pydisort.py:601-611) in 40 digits, rounded to float64."""
    with mp.workdps(nt_view_truth.DPS):
        F = lambda v: mp.mpf(float(v))  # noqa: E731
        ta = [F(x) for x in np.atleast_1d(kw["tau_arr"])]
        om = [F(x) for x in np.broadcast_to(kw["omega_arr"], (len(ta),))]
        f = [F(x) for x in np.broadcast_to(kw["f_arr"], (len(ta),))]
        s1 = sum(o * t for o, t in zip(om, ta))
        s2 = sum(x * o * t for x, o, t in zip(f, om, ta))
        return float(F(kw["mu0"]) / (1 - (s1 / sum(ta)) * (s2 / s1)))


def angles(kw):
    nodes = nt_truth.quadrature_nodes(kw["NQuad"] // 2)
    mu0, s = kw["mu0"], scaled_mu0(kw)
    mu = [0.23, 0.71, -0.37, -0.83, nodes[1], -nodes[len(nodes) // 2], 1.0, -1.0, mu0, -mu0, -mu0 * (1 + 1e-9), -mu0 * (1 - 1e-9),
          -s, -s * (1 + 1e-9), -1e-3]
    return np.array([m for m in mu if abs(m) <= 1.0])


def points(tau_arr):
    t = np.atleast_1d(np.asarray(tau_arr, float))
    if len(t) == 1:
        return np.array([0.0, 0.37 * t[0], 0.8 * t[0], t[0]])
    mid = len(t) // 2
    return np.array([0.0, t[0], t[mid - 1] + 0.41 * (t[mid] - t[mid - 1]), t[-1]])


def build(name):
    """-> dict of arrays, exactly what the fixture file holds."""
    made = CASES[name][0]()
    cols = made if isinstance(made, list) else [made]
    phi = np.array([cols[0]["phi0"], 2.1])
    mus = [angles(kw) for kw in cols]
    assert len({len(m) for m in mus}) == 1
    taus = [points(kw["tau_arr"]) for kw in cols]
    truths = [nt_view_truth.correction(kw, m, t, phi) for kw, m, t in zip(cols, mus, taus)]
    stack = (lambda v: np.stack(v)) if isinstance(made, list) else (lambda v: v[0])
    res = {k: stack([np.asarray(kw[k]) for kw in cols]) for k in INPUTS}
    for k in ("NQuad", "NLeg", "NFourier"):
        res[k] = np.array(int(cols[0][k]))
    res.update(mu=stack(mus), tau=stack(taus), phi=phi, batch=np.array(int(isinstance(made, list))))
    for o in ORDERS:
        res["truth_" + o] = stack([tr[o] for tr in truths])
        assert np.all(np.isfinite(res["truth_" + o]))
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
            print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB, nmu {res['mu'].shape[-1]}", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
