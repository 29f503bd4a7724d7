"""The ocean surface model on the device: ``surface=dict(model="ocean", ...)`` of the batch, streamed and band entry points,
``surface_reflectance("ocean")``, ``Plan.get_bdrf`` (csrc/rtd_surface.h, csrc/rtd_surface_ocean.hip).

Truth is tools/surface_ocean_truth.py (tests/golden/surface_ocean), whose docstring states every bound used here:

* the device's samples against rho in 50 digits at 16 x np_dist_all[0] of the row's max |rho|, the bound of
  tests/test_surface_ocean_cpu.py (the uniform grid of ``surface_reflectance`` at nphi = 4 hits the fixture's exact azimuths 0, pi/2,
  pi);
* ``get_bdrf()`` against the 50-digit modes OF THE SAME QUADRATURE RULE within
      tol_m = [16 np_dist_modes + (52 m + 104 + nphi / 2 + 8) 2^-53] (2 - delta_m0) q^0(pair)
  (the second part is derived in csrc/rtd_surface_ocean.hip from the kernel's loop, the first is the conditioning of a sample in
  dphi, measured by the tool on a NumPy float64 evaluation of the rule);
* ``get_bdrf()`` against the CONVERGED integrals (the rule at 4096 nodes) within MARGIN x FIG[streams] of each pair's own
  max_m |q^m|, FIG the convergence table of profiles/surface_ocean.json for the test's nphi (worst over U = 0, 1, 5, 15, all modes
  < 64) and MARGIN = 4 -- the table is for the nodes alone and U on a grid, the test's columns have a mu0 column and other winds --
  plus twice the rounding bound above (the device's and that of the float64 reference);
* everything else is BIT identity, each its own assertion: the request against its own tables uploaded, shared against repeated
  parameters, one window against windows of 4, the band entry against the batch entry, Kirchhoff's law on the device-formed mode;
* rho_w alone moves q^0 by rho_w and no other mode, to rounding (bound in the test).

Shapes: 6 columns x 3 layers at 6 / 16 / 34 streams with NBDRF = NFourier = NQuad, per-column (U, n, rho_w) and mu0 (column 0: the
sun overhead, mu0 = 1), nphi = 256 / 256 / 512; one column's tables alone at 64 streams, nphi = 512 (one pass of 64 modes).  Without
the model every test here fails at the front end (unknown model -> ValueError)."""
import functools
import glob
import os

import numpy as np
import pytest

import test_gpu_surface as ts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "surface_ocean")
RHO_FILES = sorted(glob.glob(os.path.join(GOLDEN, "rho_U*.npz")))
C, L, PHI = ts.C, ts.L, ts.PHI
U53 = 2.0 ** -53
FIG = {6: 5.6e-15, 16: 3.3e-12, 34: 1.4e-14, 64: 1.7e-9}  # profiles/surface_ocean.json: nphi = 256, 256, 512, 512; worst over U
MARGIN = 4.0


@functools.lru_cache(maxsize=None)
def case(NQuad):
    """The fixture of `NQuad` streams and the batch it belongs to (built once, left unchanged)."""
    d = dict(np.load(os.path.join(GOLDEN, f"modes_n{NQuad}.npz")))
    n = len(d["mu0"])
    kw = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in ts.columns(NQuad).items()}
    kw["mu0"] = d["mu0"]
    sf = dict(model="ocean", params=d["params"][:, :3], nphi=int(d["nphi"]))
    for v in list(d.values()) + [sf["params"]]:
        v.setflags(write=False)
    return d, kw, sf


def mode_tol(d, nb):
    m = np.arange(nb)
    return 16.0 * float(d["np_dist_modes"][0]) + (52.0 * m + 104.0 + int(d["nphi"]) / 2 + 8.0) * U53


@pytest.mark.parametrize("path", RHO_FILES, ids=[os.path.basename(f)[:-4] for f in RHO_FILES])
def test_device_samples_against_truth(path):
    import pydisort_amd
    d = np.load(path)
    tol = 16.0 * float(d["np_dist_all"][0])
    assert 1e-16 < tol < 2e-12
    got = pydisort_amd.surface_reflectance("ocean", d["params"][:3], d["mu"][:, None], d["mup"][None, :], 4)
    assert got.shape == d["rho"].shape[:2] + (4,) and np.all(np.isfinite(got))
    err = np.abs(got[..., :3] - d["rho"][..., :3]) / d["scale"][:, :, None]
    print(f"{os.path.basename(path)}: tolerance {tol:.3e} of the row's max |rho|; worst on the device {err.max():.3e}")
    assert err.max() <= tol
    assert np.array_equal(got[..., 3], got[..., 1])  # even in dphi


@pytest.mark.parametrize("NQuad", [6, 16, 34, 64])
def test_tables_against_the_modes_of_the_rule_and_the_converged_integrals(NQuad):
    import pydisort_amd
    d, kw, sf = case(NQuad)
    N = NQuad // 2
    _, sol = pydisort_amd.pydisort_batch(**kw, surface=sf, _defer_solve=True)
    q, q0 = sol.plan.get_bdrf()
    assert q.shape == d["q"].shape == (len(d["mu0"]), NQuad, N, N) and q0.shape == d["q0"].shape and np.all(np.isfinite(q)) and np.all(np.isfinite(q0))
    tol = mode_tol(d, NQuad) * np.where(np.arange(NQuad) == 0, 1.0, 2.0)
    assert 1e-15 < tol.min() and tol.max() < 1e-11
    e = np.abs(q - d["q"]) / d["q"][:, :1] / tol[None, :, None, None]
    e0 = np.abs(q0 - d["q0"]) / d["q0"][:, :1] / tol[None, :, None]
    print(f"{NQuad} streams, nphi {int(d['nphi'])}: same rule, worst error / bound {e.max():.3f} (q), {e0.max():.3f} (q0); bound {tol.min():.2e} ... {tol.max():.2e}")
    assert e.max() <= 1.0
    assert e0.max() <= 1.0
    allowed = MARGIN * FIG[NQuad] + 2.0 * tol.max()
    c = np.abs(q - d["q_conv"]) / np.max(np.abs(d["q_conv"]), axis=1, keepdims=True)
    c0 = np.abs(q0 - d["q0_conv"]) / np.max(np.abs(d["q0_conv"]), axis=1, keepdims=True)
    print(f"  converged integrals: worst {c.max():.3e} (q), {c0.max():.3e} (q0) of the pair's largest mode; allowed {allowed:.3e}")
    assert c.max() <= allowed
    assert c0.max() <= allowed
    # the adaptive quadrature of the uniform-dphi integral agrees with what "converged" means here (column 0, a few pairs)
    pr, k = d["adaptive_pairs"], d["adaptive"].shape[1]
    a = np.abs(q[0, :k, pr[:, 0], pr[:, 1]] - d["adaptive"]) / np.max(np.abs(d["adaptive"]), axis=1, keepdims=True)
    assert a.max() <= allowed + 1e-11  # (scipy's quad: epsabs = epsrel = 1e-13 requested, 1.6e-12 measured against the rule at 64 streams)


@pytest.mark.parametrize("NQuad", [6, 16, 34])
def test_request_gives_the_bits_of_its_tables_uploaded(NQuad):
    import pydisort_amd
    d, kw, sf = case(NQuad)
    _, sol = pydisort_amd.pydisort_batch(**kw, surface=sf)
    q, q0 = sol.plan.get_bdrf()
    _, ref = pydisort_amd.pydisort_batch(**kw, device_prepare=True, bdrf_q=q, bdrf_q0=q0)
    ts.same_tables(sol.plan, ref.plan, "request against tables")
    ts.same_bits(ts.fields(sol, ts.levels(kw)), ts.fields(ref, ts.levels(kw)), "request against tables")


@pytest.mark.parametrize("NQuad", [6, 16, 34])
def test_shared_parameters_give_the_bits_of_repeated_ones(NQuad):
    import pydisort_amd
    d, kw, sf = case(NQuad)
    row = sf["params"][2]
    _, shared = pydisort_amd.pydisort_batch(**kw, surface=dict(sf, params=row))
    _, repeated = pydisort_amd.pydisort_batch(**kw, surface=dict(sf, params=np.tile(row, (C, 1))))
    qa, _ = ts.same_tables(shared.plan, repeated.plan, "shared against repeated")
    ts.same_bits(ts.fields(shared, ts.levels(kw)), ts.fields(repeated, ts.levels(kw)), "shared against repeated")
    # column 2 of the shared plan IS column 2 of the fixture (the nodes' table does not depend on mu0); column 0 is not column 0
    tol = mode_tol(d, NQuad) * np.where(np.arange(NQuad) == 0, 1.0, 2.0)
    assert np.all(np.abs(qa[2] - d["q"][2]) <= tol[:, None, None] * d["q"][2, :1])
    assert not np.all(np.abs(qa[0] - d["q"][0]) <= tol[:, None, None] * d["q"][0, :1])


@pytest.mark.parametrize("NQuad", [6, 16, 34])
def test_streamed_windows_give_the_bits_of_one_window(NQuad):
    import pydisort_amd
    d, kw, sf = case(NQuad)
    _, sol = pydisort_amd.pydisort_batch(**kw, surface=sf, _defer_solve=True)
    assert sol.plan.windows()[1] == 1
    sol.plan.set_eval_points(ts.levels(kw), PHI)
    want = sol.plan.run_fetch()
    got = pydisort_amd.solve_columns_streamed(dict(kw, surface=sf), ts.levels(kw), PHI, chunk_columns=4)
    ts.same_bits({k: got[k] for k in want}, want, "windows of 4")


@pytest.mark.parametrize("NQuad", [8, 16, 32])
def test_band_entry_gives_the_bits_of_the_batch_entry(NQuad):
    import pydisort_amd
    import test_gpu_band as tb
    kw = tb.band(NQuad)
    P, G = tb.P, tb.G
    rng = np.random.default_rng(11)
    par = np.stack((rng.uniform(0.0, 12.0, (P, G)), np.linspace(1.33, 1.36, P * G).reshape(P, G), rng.uniform(0.0, 0.05, (P, G))), axis=2)  # n follows the wavelength
    nphi = 4 * NQuad
    tau, om, f, leg = pydisort_amd.band_mix(kw["dtau_abs"], kw["dtau_spec"], kw["omega_spec"], kw["Leg_spec"], NQuad, delta_M=True)
    rep = lambda a: np.repeat(a, G, axis=0)  # noqa: E731
    _, sol = pydisort_amd.pydisort_batch(tau, om, NQuad, leg, rep(kw["mu0"]), kw["I0"].reshape(-1), rep(kw["phi0"]), f_arr=f,
                                         b_pos=rep(kw["b_pos"]), b_neg=kw["b_neg"], surface=dict(model="ocean", params=par.reshape(P * G, 3), nphi=nphi))
    lev = np.concatenate((np.zeros((P * G, 1)), tau), axis=1)
    _, bsol = pydisort_amd.pydisort_band(**kw, weights=tb.WEIGHTS, surface=dict(model="ocean", params=par, nphi=nphi))
    ts.same_tables(bsol.plan, sol.plan, "band against batch")
    ts.same_bits(ts.fields(bsol.columns, lev), ts.fields(sol, lev), "band against batch")
    q, q0 = sol.plan.get_bdrf()  # the streamed band form: the request against the same tables uploaded per column
    got = pydisort_amd.solve_band_streamed(**kw, weights=tb.WEIGHTS, phi=PHI, chunk_columns=4, surface=dict(model="ocean", params=par, nphi=nphi))
    ref = pydisort_amd.solve_band_streamed(**kw, weights=tb.WEIGHTS, phi=PHI, chunk_columns=4, bdrf_q=q, bdrf_q0=q0)
    keys = ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct")
    ts.same_bits({k: got[k] for k in keys}, {k: ref[k] for k in keys}, "streamed band")


def test_kirchhoff_emissivity_uses_the_device_formed_mode():
    import pydisort_amd
    d, kw, sf = case(16)
    rng = np.random.default_rng(5)
    th = dict(TEMPER=np.sort(rng.uniform(200.0, 300.0, (C, L + 1)), axis=1), WVNMLO=500.0, WVNMHI=900.0, BTEMP=rng.uniform(280.0, 310.0, C),
              TTEMP=60.0, TEMIS=0.8)
    _, sol = pydisort_amd.pydisort_batch(**kw, surface=sf, thermal=th)
    q, q0 = sol.plan.get_bdrf()
    _, ref = pydisort_amd.pydisort_batch(**kw, device_prepare=True, bdrf_q=q, bdrf_q0=q0, thermal=th)
    ts.same_tables(sol.plan, ref.plan, "kirchhoff")
    ts.same_bits(ts.fields(sol, ts.levels(kw)), ts.fields(ref, ts.levels(kw)), "kirchhoff")
    _, black = pydisort_amd.pydisort_batch(**kw, thermal=th)  # the emissivity did come from the mode: a black surface emits more
    assert np.all(black.flux_up(ts.levels(kw))[:, -1] != sol.flux_up(ts.levels(kw))[:, -1])


def test_rho_w_alone_moves_the_zeroth_mode_by_rho_w():
    """q^m(rho + rho_w) - q^m(rho) = rho_w x (the rule applied to cos(m dphi)) = rho_w delta_m0: the integrand
    cos(m (psi - a sin psi)) (1 - a cos psi) has the Fourier coefficients J_k(m a) in psi, gone long before k = nphi - m = 192.  In
    float64 both runs use the SAME nodes, weights and factors T_m; a sample differs by fl(rho + rho_w) - rho = rho_w (1 + e), |e| <= u
    of rho + rho_w, and each run's sum is rounded: with S = q^0 + q^0' (the two sums of |terms|)
        |difference - rho_w delta_m0| <= (2 - delta_m0) [(nphi / 2 + 10) u S + (52 m + 104) u rho_w]
    -- (nphi / 2 + 8) u S for the two summations, 2 u S for the addition and the weight, and the factors' error (derived in
    csrc/rtd_surface_ocean.hip) on the difference of the samples only, rho_w."""
    import pydisort_amd
    d, kw, sf = case(16)
    rw, nphi, NB = 0.05, int(d["nphi"]), 16
    par = np.array(sf["params"])
    par[:, 2] = 0.0
    _, a = pydisort_amd.pydisort_batch(**kw, surface=dict(sf, params=par), _defer_solve=True)
    par2 = par.copy()
    par2[:, 2] = rw
    _, b = pydisort_amd.pydisort_batch(**kw, surface=dict(sf, params=par2), _defer_solve=True)
    m = np.arange(NB)
    sc = np.where(m == 0, 1.0, 2.0)
    for ta, tb_ in zip(a.plan.get_bdrf(), b.plan.get_bdrf()):
        shp = (1, NB) + (1,) * (ta.ndim - 2)
        S = ta[:, :1] + tb_[:, :1]
        tol = sc.reshape(shp) * ((nphi / 2 + 10) * U53 * S + ((52.0 * m + 104.0) * U53 * rw).reshape(shp))
        want = np.where(m == 0, rw, 0.0).reshape(shp)
        err = np.abs(tb_ - ta - want)
        print(f"rho_w shift: worst error / bound {np.max(err / tol):.3f}")
        assert np.all(ta[:, 0] > 0) and np.all(err <= tol)
