"""Cases and fixture format of tests/test_gpu_eigen_stage_bits.py: tiny batches whose eigen-stage tensors and evaluated fields are
pinned BIT FOR BIT (tests/golden/eigen_bits/<case>.npz, written by tests/golden/make_eigen_bits_goldens.py on an MI355X from the
commit before the eigen kernel's select-free reductions and Cholesky steps).

Shapes: the smallest that reach every path of the 16-stream-group eigen kernel -- 32 streams with 4 Fourier modes at 1, 5 and 20
layers (four problems per wavefront: the last wavefront of a column is partial at 1 and 5), beam only, beam plus a thermal
polynomial (mode 0 takes the thermal branch), no beam, one column whose 1/mu0 lies 5e-4 above an eigenvalue; 18 and 30 streams
(padding streams inside the group of 16); one 16-stream and one 64-stream case for the neighbouring instances.  Two cases pin the
remaining instances of the fused eigen kernel (fixtures from the commit before that kernel was cut into stage functions): 66
streams, the smallest count that takes the one-problem-per-wavefront instance, and the 32-stream beam + thermal case with the
assembly on the matrix cores (RTD_EIG_MFMA=1, a switch the launcher reads once per process: computed in a fresh child process).

What is pinned per case: ``Plan.tensors`` of every column (G from Y, A and k; K; B; the thermal vector G_inv_mu_inv; GC, which
adds the boundary-condition solve) and u, u0 and the three fluxes at the interfaces and the layers' mid-points (E = exp(-k dtau)
and the thermal vectors dq, vb reach these).  An array over FULL_BYTES is stored as its two diagonal corner blocks along the leading axes
(first Fourier mode of the first layer, last mode of the last layer) and every array, stored whole or not, with the SHA-256 of all its bytes.
"""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

FULL_BYTES = 40 << 10
PHI = np.array([0.0, 1.0, np.pi])
TENSORS = ("G", "K", "B", "G_inv_mu_inv", "GC")

# name -> (NQuad, L, columns, kind)
CASES = {
    "q32_L1_beam": (32, 1, 2, "beam"),
    "q32_L5_beam": (32, 5, 2, "beam"),
    "q32_L20_beam": (32, 20, 1, "beam"),
    "q32_L5_beam_thermal": (32, 5, 2, "beam_thermal"),
    "q32_L5_no_beam": (32, 5, 2, "no_beam"),
    "q32_L1_resonant": (32, 1, 2, "resonant"),
    "q18_L3_padded": (18, 3, 2, "beam_thermal"),
    "q30_L3_padded": (30, 3, 2, "beam_thermal"),
    "q16_L3_neighbour": (16, 3, 2, "beam_thermal"),
    "q64_L3_neighbour": (64, 3, 1, "beam_thermal"),
    "q66_L2_wide": (66, 2, 1, "beam_thermal"),
    "q32_L5_beam_thermal_mfma": (32, 5, 2, "beam_thermal"),  # the inputs of q32_L5_beam_thermal
}
# cases computed under a run-time switch of the library that is read once per process: name -> environment of the child
CHILD_ENV = {"q32_L5_beam_thermal_mfma": {"RTD_EIG_MFMA": "1"}}
NFOURIER = 4
RESONANCE_OFFSET = 5e-4  # 1/mu0 - k of the resonant column (column 1 of its case)


def inputs(name, resonant_mu0=None):
    """Keyword arguments of ``pydisort_batch`` for a case.  The resonant case needs mu0 of its column 1, which depends on an
    eigenvalue the solver computed: the fixture carries it (``resonant_mu0``)."""
    from pydisort_amd import synthetic
    nquad, L, C, kind = CASES[name]
    cfg = synthetic.cfg4_columns(C, first=300, L=L, NQuad=nquad)
    cfg["NFourier"] = NFOURIER
    if kind in ("beam_thermal", "no_beam"):
        rng = np.random.default_rng([11, nquad, L])
        cfg["s_poly_coeffs"] = rng.uniform(0.05, 0.4, (C, L, 1)) * np.array([1.0, 0.1])
        cfg["b_neg"] = 0.05
        cfg["b_pos"] = 0.1
    if kind == "no_beam":
        cfg["I0"] = np.zeros(C)
    if kind == "resonant" and resonant_mu0 is not None:
        cfg["mu0"] = cfg["mu0"].copy()
        cfg["mu0"][1] = resonant_mu0
    return cfg


def eval_tau(cfg):
    """0, every interface and the mid-point of every layer, per column."""
    edges = np.concatenate((np.zeros((cfg["tau_arr"].shape[0], 1)), cfg["tau_arr"]), axis=1)
    return np.sort(np.concatenate((edges, 0.5 * (edges[:, 1:] + edges[:, :-1])), axis=1), axis=1)


def compute(amd, cfg):
    """name -> array: the tensors of every column (``c<i>.<tensor>``) and the evaluated fields of the batch."""
    _, sol = amd.pydisort_batch(**cfg)
    out = {}
    try:
        for c in range(cfg["tau_arr"].shape[0]):
            t = sol.plan.tensors(c)
            for k in TENSORS:
                out[f"c{c}.{k}"] = t[k]
        tau = eval_tau(cfg)
        out["u"] = sol.u(tau, PHI)
        out["u0"] = sol.u0(tau)
        out["flux_up"] = sol.flux_up(tau)
        out["flux_down_diffuse"], out["flux_down_direct"] = sol.flux_down(tau)
    finally:
        sol.plan.close()
    return out


def compute_in_child(name):
    """``compute`` of a CHILD_ENV case in a fresh process that starts with the case's switches set."""
    with tempfile.TemporaryDirectory(prefix="eigen_bits_") as tmp:
        out = os.path.join(tmp, name + ".npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name, out], env=dict(os.environ, **CHILD_ENV[name]),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        with np.load(out) as z:
            return {k: z[k] for k in z.files}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def stored_part(a):
    """What a fixture keeps of an array: all of it up to FULL_BYTES, else its two diagonal corner blocks [0, 0] and [-1, -1]."""
    if a.nbytes <= FULL_BYTES or a.ndim < 3:
        return a
    return a[[0, a.shape[0] - 1], [0, a.shape[1] - 1]]


if __name__ == "__main__":  # the child of compute_in_child: CASE OUTPUT.npz
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), os.path.join(os.path.dirname(here), "pythonic-disort_amd")]
    import pydisort_amd
    assert all(os.environ.get(k) == v for k, v in CHILD_ENV[sys.argv[1]].items())
    np.savez(sys.argv[2], **compute(pydisort_amd, inputs(sys.argv[1])))
