"""The cases of the tau-derivative fixtures (tests/golden/deriv/*.npz), shared by their maker
(tests/golden/make_derivative_goldens.py) and by the tests that read them: name -> keyword arguments of ``pydisort``.

Catalogue cases are the first captured call of tests/golden/ref/<id>.npz; the synthetic ones are single columns of
pydisort_amd.synthetic; random<family>_<seed> are seeds of the generators of tests/test_gpu_random_parity.py, picked for what the
others leave out: Nakajima-Tanaka corrections in several layers (nt_L6_q16, random_3, random_29), thermal polynomials of degree 2
(random_24, _31, _49, random128_1, _4), more than 64 streams (random128_1: 66, 40 modes; _4: 112; _6: 70, one layer, no beam,
40 modes), 6 streams, vector b_pos, only_flux.  The omega = 1 - 1e-6 problems (ILL_CONDITIONED in tests/test_gpu_parity.py) and 8ARTS_* stay out: there
the reference's float64 is itself the side that is off.
"""
import os

import numpy as np

import goldens

DERIV_DIR = os.path.join(goldens.HERE, "golden", "deriv")
CATALOGUE = ("1a", "2a", "4b", "4c", "6d", "6h", "7a", "7d", "8a", "8c", "9a", "9c", "9corrections", "11a")
SYNTHETIC = ("cfg2_q32", "cfg4_0", "cfg4_2", "cfg5_0")
NT_MULTILAYER = ("nt_L6_q16",)
RANDOM = ("random_3", "random_29", "random_24", "random_31", "random_49", "random128_1", "random128_4", "random128_6")
CASES = CATALOGUE + SYNTHETIC + NT_MULTILAYER + RANDOM
ONE_SIDED = ("9c", "cfg4_0", "nt_L6_q16", "random_24")
QUANTITIES = ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct")
FLUXES = QUANTITIES[2:]
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


def random_case(family, seed):
    """Keyword arguments of seed `seed` of a random family of tests/test_gpu_random_parity.py ("random", "random32", ...)."""
    import test_gpu_random_parity as R
    return {"random": R.make_case, "random32": R.make_case_many_streams, "random64": R.make_case_64_streams,
            "random128": R.make_case_128_streams}[family](seed)


SWEEP_FAMILIES = (("random", 60), ("random32", 40), ("random64", 12), ("random128", 10))  # every seed of the value sweeps


def sweep_case(family, seed):
    """-> (keyword arguments, is_twin) of a seed as the sweeps of both tau-orders run it (tests/test_gpu_random_orders.py).  With
    a layer at omega > 1 - 1e-5 the oracle's float64 is itself off (the value sweeps judge such a seed against its 40-digit
    fixture, which holds values only): the sweeps run its twin, the same atmosphere with omega_arr = minimum(omega_arr, 0.999)."""
    kw = random_case(family, seed)
    twin = bool(np.any(kw["omega_arr"] > 1 - 1e-5))
    if twin:
        kw = dict(kw, omega_arr=np.minimum(kw["omega_arr"], 0.999))
    return kw, twin


def case_kwargs(name):
    """Keyword arguments of the one-column ``pydisort`` (the reference's and this project's alike)."""
    from pydisort_amd import synthetic
    if name in CATALOGUE:
        return goldens.load(name)[0]["kwargs"]
    if name in RANDOM:
        family, seed = name.split("_")
        return random_case(family, int(seed))
    if name == "nt_L6_q16":  # (17 moments given, 16 used: the corrections are active in all six layers)
        return dict(synthetic.column_kwargs(synthetic.cfg4_columns(3, L=6, NQuad=16), 1), NLeg=16, NT_cor=True)
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


def tolerance(fd_uncertainty, tol_floor, ceiling, factor=10.0):
    """The rule every fixture quantity is held by, whoever is held (the kernels, the oracle's analytic derivative):
    min(ceiling, max(tol_floor, factor x fd_uncertainty)); ceiling None: no ceiling (the one-sided fixtures)."""
    tol = max(tol_floor, factor * fd_uncertainty)
    return tol if ceiling is None else min(ceiling, tol)


def hold(label, got, z, tol_floor, ceiling, factor=10.0, record=None):
    """Asserts every quantity of `got` (dict as ``evaluate`` returns) against the fixture z under ``tolerance``: the largest
    difference over the largest reference magnitude, per quantity; a quantity that is identically zero in the fixture is held
    absolutely, on the scale of the case's fluxes.  record(label, quantity, err, pointwise, tol, fd_uncertainty), if given, is
    called before the assertion.  -> the worst error over tolerance."""
    flux_scale = max(float(np.max(np.abs(z[q]))) for q in FLUXES if q in z.files)
    worst = 0.0
    for q in QUANTITIES:
        if q not in got:
            continue
        want, unc = z[q], float(z[q + ".unc"])
        tol = tolerance(unc, tol_floor, ceiling, factor)
        assert got[q].shape == want.shape, (label, q, got[q].shape, want.shape)
        assert np.all(np.isfinite(got[q])), (label, q)
        if int(z[q + ".abs"]):
            err, pw = float(np.max(np.abs(got[q]))) / flux_scale, 0.0
        else:
            err, pw = goldens.max_rel_err(got[q], want)
        print(f"tau-derivative {label:28s} {q:18s} scale-rel {err:.3e} pointwise {pw:.3e} fd_uncertainty {unc:.1e} tol {tol:.1e}")
        if record is not None:
            record(label, q, err, pw, tol, unc)
        assert err < tol, (label, q, err, tol)
        worst = max(worst, err / tol)
    return worst
