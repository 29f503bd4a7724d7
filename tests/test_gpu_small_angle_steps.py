"""The small-angle form of the eigen kernel's Jacobi step (PairStep in csrc/rtd_eig.hip) -- run with
``-m gpu`` on an MI355X.

A step takes that form when EVERY pair of the wavefront has |t| < 2^-27.  The columns here have four layers, so that one
wavefront holds the whole (column, mode) at 32 and 30 streams and its four layers share every such decision:

* straddle:  omega = 1e-12, 1e-7, 1e-6, 1e-5 -- a layer that does not scatter (t = 0 exactly) beside layers whose
  off-diagonals lie on both sides of 2^-27;
* mixed:     one layer with omega = 0.99 beside three with 1e-9 -- the wavefront keeps the general form for as long as one
  of its problems still rotates;
* ordinary0, ordinary1: two columns of the benchmark's distribution (`cfg4_columns`), whose sweep counts must stay what the
  parent build gave;
* padded:    30 streams (15 per hemisphere in 16 lanes);
* eight:     16 streams (the NP = 8 instance, eight layers' worth of lanes per wavefront).

Every column is held to the CPU oracle at the bounds tests/test_gpu_parity.py applies to well-conditioned problems: TOL of the
field scale for u and the fluxes, PW_TOL pointwise where |I| > 1e-8 of the largest, over all Fourier modes with the beam on, at
the five interfaces and three azimuths.  All of omega <= 0.99: inside, or better conditioned than, the cfg4 envelope.  The
oracle's own error on these inputs was measured on the CPU by solving every column once more with each layer cut into two
equal halves (the same atmosphere, twice the eigen-decompositions and another boundary system): the two solves agree to
1.5e-13 of the field scale and 2.1e-11 pointwise on the straddle column (whose field is 4e-6 of the beam) and to <= 1.8e-14 /
1.4e-12 on the other five, far inside the bounds.  Reordering the layers themselves gives another atmosphere, so it was
checked in the same way: the straddle and mixed columns with their layers in the orders 3210 and 1302 agree with their
re-layered selves to <= 1.6e-13 / 1.3e-10 (fluxes: <= 6.3e-11 of the flux scale)."""
import numpy as np
import pytest

import goldens

pytestmark = pytest.mark.gpu

TOL, PW_TOL = 1e-9, 1e-6  # tests/test_gpu_parity.py: scale-relative; pointwise over |I| > 1e-8 of the largest
PHI = np.array([0.0, 1.0, np.pi])

# rtd_plan_max_sweeps of the two ordinary columns, recorded once from the build of the parent commit (the kernel without the
# small-angle form, on an MI355X): the step must not change how many sweeps a wavefront takes
PARENT_MAX_SWEEPS = {"ordinary0": 6, "ordinary1": 6}


def _hg_column(omega, g=0.85, NQuad=32):
    """Four Henyey-Greenstein layers like cfg4's (NQuad + 1 moments, delta-M on), with the given albedos."""
    from pydisort_amd import synthetic
    cfg = synthetic.cfg4_columns(1, L=4, NQuad=NQuad)
    cfg["omega_arr"] = np.array([omega], float)
    gs = np.full((1, 4), g)
    cfg["Leg_coeffs_all"] = gs[:, :, None] ** np.arange(NQuad + 1)[None, None, :]
    cfg["f_arr"] = gs ** NQuad
    return cfg


def columns():
    from pydisort_amd import synthetic
    return {
        "straddle": _hg_column([1e-12, 1e-7, 1e-6, 1e-5]),
        "mixed": _hg_column([0.99, 1e-9, 1e-9, 1e-9]),
        "ordinary0": synthetic.cfg4_columns(1, first=0, L=4),
        "ordinary1": synthetic.cfg4_columns(1, first=1, L=4),
        "padded": synthetic.cfg4_columns(1, first=2, L=4, NQuad=30),
        "eight": synthetic.cfg4_columns(1, first=3, L=4, NQuad=16),
    }


NAMES = ("straddle", "mixed", "ordinary0", "ordinary1", "padded", "eight")


@pytest.fixture(scope="module")
def solved():
    """name -> (device results, oracle results, max sweeps): every column solved once on each side."""
    import pydisort_amd
    from pydisort_amd import _engine, synthetic
    from oracle import disort_oracle as O
    assert _engine.device_count() >= 1, "no HIP device visible"
    out = {}
    for name, cfg in columns().items():
        tau = np.concatenate(([0.0], cfg["tau_arr"][0]))
        _, sol = pydisort_amd.pydisort_batch(**cfg)
        fd, fdir = sol.flux_down(tau[None])
        got = dict(u=sol.u(tau[None], PHI)[0], flux_up=sol.flux_up(tau[None])[0], flux_down=fd[0], flux_direct=fdir[0])
        sweeps = sol.plan.max_sweeps()
        sol.plan.close()
        ref = O.pydisort(**synthetic.column_kwargs(cfg, 0))
        rfd, rfdir = ref[2](tau)
        want = dict(u=ref[4](tau, PHI), flux_up=ref[1](tau), flux_down=rfd, flux_direct=rfdir)
        out[name] = (got, want, sweeps)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_column_against_oracle(solved, name):
    got, want, sweeps = solved[name]
    assert got["u"].shape == want["u"].shape == (columns()[name]["NQuad"], 5, 3)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    a, b = goldens.max_rel_err(got["u"], want["u"])
    fs = max(np.max(np.abs(want["flux_up"])), np.max(np.abs(want["flux_down"])))
    fu = np.max(np.abs(got["flux_up"] - want["flux_up"])) / fs
    fd = np.max(np.abs(got["flux_down"] - want["flux_down"])) / fs
    print(f"{name}: u {a:.2e} of the scale, {b:.2e} pointwise; flux up {fu:.2e}, down {fd:.2e} of the scale; {sweeps} sweeps")
    assert a < TOL and b < PW_TOL, (name, a, b)
    assert fu < TOL and fd < TOL, (name, fu, fd)
    assert np.allclose(got["flux_direct"], want["flux_direct"], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("name", sorted(PARENT_MAX_SWEEPS))
def test_sweep_count_is_the_parents(solved, name):
    assert solved[name][2] == PARENT_MAX_SWEEPS[name]
