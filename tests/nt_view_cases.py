"""The 40-digit fixtures of the Nakajima-Tanaka corrections at viewing angles (tests/golden/nt_view, made by
tests/golden/make_nt_view_goldens.py; arbiter: tools/nt_view_truth.py): loader, the tolerance rule and what the CPU and the GPU test
of rtd_nt_view.hip share.

Tolerance.  There is no derived bound (the forward Legendre recurrence over 300 moments gives no useful one).  The yardstick is what
the EXISTING node kernels show against the 40-digit truth, per padding class and order (tests/test_gpu_nt_truth.py: MEASURED, figures
of the parent commit on an MI355X, 1.5e-15 ... 7.6e-13 of the largest correction); the kernels at the angles are held at ten times
that class's figure, under that test's ceiling of 1e-9 -- the coincidence angles (|mu| = mu0, |mu| = the scaled mu0 and their
neighbours at 1e-9) included: they get the SAME bound, not the near-node allowance of the node kernels."""
import os
import types

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nt_view")
ORDERS = ("value", "antiderivative", "derivative")
ORDER_INT = dict(value=0, antiderivative=-1, derivative=1)
INPUTS = ("tau_arr", "omega_arr", "NQuad", "Leg_coeffs_all", "mu0", "I0", "phi0", "f_arr", "NLeg", "NFourier")
NAMES = ("q6_L1", "batch6_q16_L3", "q34_L3", "q16_L4_mu0_near_node", "q16_L4_smu0_near_node", "q32_L20_cloud")
BATCH = "batch6_q16_L3"
CEILING = 1e-9
EPS = np.finfo(float).eps
# tests/test_gpu_nt_truth.py: MEASURED -- NP: (value, antiderivative, derivative), the node kernels on the parent commit
NODE_KERNEL_MEASURED = {
    4: (1.5e-15, 1.8e-15, 1.7e-15),
    8: (4.5e-14, 3.8e-14, 3.8e-14),
    16: (7.0e-13, 7.6e-13, 4.2e-13),
    32: (1.7e-13, 3.3e-13, 1.8e-13),
    64: (1.9e-13, 1.6e-13, 2.0e-13),
}


def padding_class(NQuad):
    NP = 4
    while NP < NQuad // 2:
        NP *= 2
    return NP


def tolerance(NQuad, order):
    tol = 10 * NODE_KERNEL_MEASURED[padding_class(NQuad)][ORDERS.index(order)]
    assert tol <= CEILING
    return tol


def load(name):
    """-> namespace: kw (keyword arguments of pydisort_batch, leading column axis), C, mu [C, nmu], tau [C, ntau], phi,
    truth {order: [C, nmu, ntau, nphi]} -- the single-column fixtures get their column axis here."""
    z = np.load(os.path.join(DIR, name + ".npz"))
    batch = bool(z["batch"])
    lift = (lambda a: np.array(a)) if batch else (lambda a: np.array(a)[None])
    kw = {k: (int(z[k]) if k in ("NQuad", "NLeg", "NFourier") else lift(z[k])) for k in INPUTS}
    return types.SimpleNamespace(name=name, kw=kw, C=kw["tau_arr"].shape[0], mu=lift(z["mu"]), tau=lift(z["tau"]), phi=np.array(z["phi"]),
                                 truth={o: lift(z["truth_" + o]) for o in ORDERS})


def coincidence(case):
    """Boolean [C, nmu]: the angles within 1e-8 (relative) of -mu0 or of minus the scaled mu0 -- where the node formulas are
    infinity times zero.  (The scaled mu0 is recomputed in float64 here only to CLASSIFY the angles.)"""
    kw = case.kw
    w = kw["omega_arr"] * kw["tau_arr"]
    of = w.sum(1) / kw["tau_arr"].sum(1) * ((kw["f_arr"] * w).sum(1) / w.sum(1))
    s = kw["mu0"] / (1 - of)
    near = lambda x: np.abs(case.mu + x[:, None]) <= 1e-8 * x[:, None]  # noqa: E731
    return near(kw["mu0"]) | near(s)


def worst(got, truth, extra=None):
    """max over the columns of max|got - truth| / max|truth| per column (every column has its own scale); extra: pointwise allowance
    in absolute units, subtracted from the error first."""
    out = 0.0
    for c in range(truth.shape[0]):
        err = np.abs(got[c] - truth[c])
        if extra is not None:
            err = np.maximum(err - extra[c], 0.0)
        out = max(out, float(np.max(err) / np.max(np.abs(truth[c]))))
    return out
