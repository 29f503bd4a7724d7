"""Cases and fixture format of tests/test_gpu_bc32_bits.py: tiny batches whose boundary-condition solve by rtd_bc_mfma_kernel (18 ...
32 streams) is pinned BIT FOR BIT (tests/golden/bc32_bits/<case>.npz, written by tests/golden/make_bc32_bits_goldens.py on an MI355X
from the commit before the kernel's global accesses went to a scalar base plus a 32-bit lane offset).

Shapes: the smallest at which the kernel's addressing and its backward sweep can go wrong -- 2 columns x 2 Fourier modes (mode 0 and
one mode above it), 32 streams unless the name says otherwise:
  L = 1 (no interface: the early return), 2, 3, 4, 7 (the backward loop rotates two operand sets: both remainders, the first full
  rotation and a few more), 23 (> RTD_BCF_WIN = 20: the window is refilled inside both sweeps);
  at L = 4: beam only, no beam, beam + thermal polynomial, and a bidirectionally reflecting surface (NBDRF = 2);
  18 and 30 streams (padding lanes);
  beam + thermal at L = 4 under RTD_BC_FORCE_PIVOT=1 (every elimination redone in LDS) and =2 (pivoted in registers throughout).

What is pinned per case, on both paths of the kernel: without the fused interface evaluation (``pydisort_batch``: coefficients only;
u, u0 and the fluxes at the interfaces then come from the evaluation kernel) and with it (``set_eval_points`` at the interfaces +
``run``: u^m leaves the backward sweep itself).  The coefficients C-/C+ of every layer are read through ``Plan.tensors``: GC is G
with column j scaled by C_j, and G is the eigen stage's (pinned by tests/test_gpu_eigen_stage_bits.py), so a changed bit of a
coefficient changes GC.  Arrays over FULL_BYTES are stored as in tests/eigen_bits_cases.py: two corner blocks and the SHA-256 of
all bytes.
"""
import numpy as np

from eigen_bits_cases import digest, stored_part  # noqa: F401  (the fixture format is the eigen-bits files')

PHI = np.array([0.0, 1.0, np.pi])
NFOURIER = 2
COLUMNS = 2

# name -> (NQuad, L, kind, RTD_BC_FORCE_PIVOT or None)
CASES = {
    "q32_L1_beam": (32, 1, "beam", None),
    "q32_L2_beam": (32, 2, "beam", None),
    "q32_L3_beam": (32, 3, "beam", None),
    "q32_L7_beam": (32, 7, "beam", None),
    "q32_L23_beam_thermal": (32, 23, "beam_thermal", None),
    "q32_L4_beam": (32, 4, "beam", None),
    "q32_L4_no_beam": (32, 4, "no_beam", None),
    "q32_L4_beam_thermal": (32, 4, "beam_thermal", None),
    "q32_L4_bdrf": (32, 4, "bdrf", None),
    "q18_L4_padded": (18, 4, "beam_thermal", None),
    "q30_L4_padded": (30, 4, "beam_thermal", None),
    "q32_L4_beam_thermal_redo": (32, 4, "beam_thermal", "1"),
    "q32_L4_beam_thermal_pivoted": (32, 4, "beam_thermal", "2"),
}


def inputs(name):
    """Keyword arguments of ``pydisort_batch`` for a case."""
    from pydisort_amd import synthetic
    nquad, L, kind, _ = CASES[name]
    C = COLUMNS
    cfg = synthetic.cfg4_columns(C, first=500, L=L, NQuad=nquad)
    cfg["NFourier"] = NFOURIER
    if kind in ("beam_thermal", "no_beam", "bdrf"):
        rng = np.random.default_rng([13, nquad, L])
        cfg["s_poly_coeffs"] = rng.uniform(0.05, 0.4, (C, L, 1)) * np.array([1.0, 0.1])
        cfg["b_neg"] = 0.05
        cfg["b_pos"] = 0.1
    if kind == "no_beam":
        cfg["I0"] = np.zeros(C)
    if kind == "bdrf":  # the surface of synthetic.cfg5_columns: two Fourier modes tabulated on the quadrature grid
        N = nquad // 2
        x, _ = np.polynomial.legendre.leggauss(N)
        mu, mu0 = 0.5 * (x + 1), cfg["mu0"]
        rho = np.array([0.15, 0.35])[:C]
        s, s0 = np.sqrt(1 - mu**2), np.sqrt(1 - mu0**2)
        q0 = rho[:, None, None] * (1 + 0.5 * mu[None, :, None] * mu[None, None, :])
        q1 = rho[:, None, None] * 0.3 * (s[None, :, None] * s[None, None, :])
        q00 = rho[:, None] * (1 + 0.5 * mu[None, :] * mu0[:, None])
        q10 = rho[:, None] * 0.3 * s[None, :] * s0[:, None]
        cfg.update(bdrf_q=np.stack((q0, q1), axis=1), bdrf_q0=np.stack((q00, q10), axis=1), b_pos=0.1 * (1 - rho))
    return cfg


def interfaces(cfg):
    """0 and the bottom of every layer, per column."""
    return np.concatenate((np.zeros((cfg["tau_arr"].shape[0], 1)), cfg["tau_arr"]), axis=1)


def compute(amd, name):
    """name -> array.  ``coef.c<i>.GC``, ``coef.u`` ...: the solve without the fused evaluation and the evaluation kernel's fields at
    the interfaces; ``run.c<i>.GC``, ``run.u`` ...: the same plan after ``set_eval_points`` at the interfaces and ``run``.  The
    caller sets RTD_BC_FORCE_PIVOT (read when the plan is built) for the forced cases."""
    cfg = inputs(name)
    tau = interfaces(cfg)
    _, sol = amd.pydisort_batch(**cfg)
    plan = sol.plan
    out = {}
    try:
        assert not np.any(plan.column_status()), (name, plan.column_status())
        for c in range(COLUMNS):
            out[f"coef.c{c}.GC"] = plan.tensors(c)["GC"]
        out["coef.u"] = sol.u(tau, PHI)
        out["coef.u0"] = sol.u0(tau)
        out["coef.flux_up"] = sol.flux_up(tau)
        out["coef.flux_down_diffuse"], out["coef.flux_down_direct"] = sol.flux_down(tau)
        plan.set_eval_points(tau, PHI)
        plan.run()
        for k, v in plan.fetch().items():
            out["run." + k] = v
        assert not np.any(plan.column_status()), (name, plan.column_status())
        for c in range(COLUMNS):
            out[f"run.c{c}.GC"] = plan.tensors(c)["GC"]
    finally:
        plan.close()
    return out
