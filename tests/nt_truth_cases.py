"""The 40-digit Nakajima-Tanaka fixtures of tests/golden/nt (tests/golden/make_nt_truth_goldens.py; arbiter: tools/nt_truth.py):
loader and the oracle's side, shared by tests/test_nt_truth_cpu.py and tests/test_gpu_nt_truth.py."""
import os
import types
import warnings

import numpy as np

NT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nt")
ORDERS = ("value", "antiderivative", "derivative")
ORACLE_KW = dict(value={}, antiderivative=dict(is_antiderivative_wrt_tau=True), derivative=dict(is_derivative_wrt_tau=True))
INPUTS = ("tau_arr", "omega_arr", "NQuad", "Leg_coeffs_all", "mu0", "I0", "phi0", "f_arr", "NLeg", "NFourier")
NEAR_NODE = ("q16_L4_mu0_near_node", "q16_L4_smu0_near_node")
TEST_PROBLEMS = ("tp_4a", "tp_4b", "tp_5a", "tp_5b")
BATCH = "batch7_q16_L6"
WELL_CONDITIONED = ("q6_L1", "q10_L2_low_sun", "q16_L7_mixed", "q16_L50", "q18_L3", "q34_L3", "q66_L2", "q32_L20_cloud",
                    "q32_L20_thick", "q64_L5", "q128_L2") + TEST_PROBLEMS + (BATCH,)
SINGLE = tuple(n for n in WELL_CONDITIONED + NEAR_NODE if n != BATCH)


def load(name):
    """-> namespace: z (the file), tau, phi, truth {order: array}, columns (list of pydisort keyword dicts, one per column),
    batch (bool: the arrays carry a leading column axis)."""
    z = np.load(os.path.join(NT_DIR, name + ".npz"))
    batch = bool(z["batch"])

    def col(c):
        kw = {}
        for k in INPUTS:
            v = z[k] if not batch or z[k].ndim == 0 else z[k][c]
            kw[k] = int(v) if k in ("NQuad", "NLeg", "NFourier") else float(v) if v.ndim == 0 else np.array(v)
        return kw
    columns = [col(c) for c in range(z["tau"].shape[0] if batch else 1)]
    return types.SimpleNamespace(name=name, z=z, batch=batch, tau=z["tau"], phi=z["phi"], columns=columns,
                                 truth={o: z["truth_" + o] for o in ORDERS})


def batch_kwargs(case):
    """Keyword arguments of pydisort_batch for the whole fixture (one column for the single-column ones)."""
    cols = case.columns
    kw = {k: np.stack([np.asarray(c[k]) for c in cols]) for k in INPUTS if k not in ("NQuad", "NLeg", "NFourier")}
    kw.update({k: cols[0][k] for k in ("NQuad", "NLeg", "NFourier")})
    return kw


def oracle_terms(kw, tau, phi, order):
    """The oracle's tms + ims [NQuad, ntau, nphi] in the caller's units, without solving anything (the corrections are closed
    forms of the prepared inputs)."""
    from oracle import disort_oracle as O, nt_oracle
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = O.prepare(**dict(kw, NT_cor=True))
    sol = types.SimpleNamespace(p=p, mu_arr=np.concatenate((p["mu"], -p["mu"])))
    tau_a, l, ts = O.Solution._locate(sol, tau)
    ad, dv = order == "antiderivative", order == "derivative"
    corr = nt_oracle.tms(sol, tau_a, l, ts, phi, ad, dv)
    corr[p["N"]:] += nt_oracle.ims(sol, tau_a, phi, ad, dv)
    return p["rescale"] * corr


def distance(got, truth):
    """max|got - truth| / max|truth|."""
    return float(np.max(np.abs(np.asarray(got) - truth)) / np.max(np.abs(truth)))
