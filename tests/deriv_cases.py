"""The cases of the tau-derivative fixtures (tests/golden/deriv/*.npz), shared by their maker
(tests/golden/make_derivative_goldens.py) and by the tests that read them: name -> keyword arguments of ``pydisort``.

Catalogue cases are the first captured call of tests/golden/ref/<id>.npz; the synthetic ones are single columns of
pydisort_amd.synthetic.  The omega = 1 - 1e-6 problems (ILL_CONDITIONED in tests/test_gpu_parity.py) and 8ARTS_* stay out: there
the reference's float64 is itself the side that is off.
"""
import os

import numpy as np

import goldens

DERIV_DIR = os.path.join(goldens.HERE, "golden", "deriv")
CATALOGUE = ("1a", "2a", "4b", "4c", "6d", "6h", "7a", "7d", "8a", "8c", "9a", "9c", "9corrections", "11a")
SYNTHETIC = ("cfg2_q32", "cfg4_0", "cfg4_2", "cfg5_0")
CASES = CATALOGUE + SYNTHETIC
ONE_SIDED = ("9c", "cfg4_0")
QUANTITIES = ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct")
PHI = np.array([0.0, 1.0, 2.5])
CAP, CAP_ONE_SIDED = 5e-9, 1e-6  # admission: fd_uncertainty of a stored quantity
CFG5_NFOURIER = 4


def batch_config(name):
    """-> (pydisort_batch keyword arguments, column of `name` in that batch): the synthetic multi-layer cases embedded in a
    larger batch, with other columns behind them."""
    from pydisort_amd import synthetic
    if name in ("cfg4_0", "cfg4_2"):
        return synthetic.cfg4_columns(5), int(name[-1])
    if name == "cfg5_0":
        return dict(synthetic.cfg5_columns(2), NFourier=CFG5_NFOURIER), 0
    raise KeyError(name)


def case_kwargs(name):
    """Keyword arguments of the one-column ``pydisort`` (the reference's and this project's alike)."""
    from pydisort_amd import synthetic
    if name in CATALOGUE:
        return goldens.load(name)[0]["kwargs"]
    if name == "cfg2_q32":
        return dict(synthetic.literal_cases()[name][0])
    cfg, i = batch_config(name)
    kw = synthetic.column_kwargs(cfg, i)
    if "NFourier" in cfg:
        kw["NFourier"] = cfg["NFourier"]
    if "bdrf_q" in cfg:  # tabulated on the quadrature grid: replayed as callables f(mu, -mu')
        kw["BDRF_Fourier_modes"] = [goldens.TabulatedBDRF(cfg["bdrf_q"][i, m], cfg["bdrf_q0"][i, m])
                                    for m in range(cfg["bdrf_q"].shape[1])]
    return kw


def load(name, one_sided=False):
    return np.load(os.path.join(DERIV_DIR, ("onesided_" if one_sided else "") + name + ".npz"), allow_pickle=False)


def evaluate(res, tau, phi, **kw):
    """The five quantities from the tuple ``pydisort`` returned (mu_arr, flux_up, flux_down, u0[, u]) -> dict, with the tau
    axis kept whatever the number of points (the closures squeeze a single point away): u [NQuad, ntau, nphi],
    u0 [NQuad, ntau], fluxes [ntau]."""
    nt = np.size(tau)
    fd = res[2](tau, **kw)
    out = {"flux_up": np.asarray(res[1](tau, **kw), float).reshape(nt),
           "u0": np.asarray(res[3](tau, **kw), float).reshape(-1, nt),
           "flux_down_diffuse": np.asarray(fd[0], float).reshape(nt),
           "flux_down_direct": np.broadcast_to(np.asarray(fd[1], float), (nt,)).copy()}  # (no beam: the scalar 0)
    if len(res) > 4:
        out["u"] = np.asarray(res[4](tau, phi, **kw), float).reshape(-1, nt, len(phi))
    return out
