"""Radiances at user polar angles, before anything touches the device: the entry points of include/rtd.h (rtd_plan_set_view_mu,
rtd_plan_fetch_view, rtd_plan_fetch_band_view) are declared, bound and exported and the header stays C99; bad angles are refused
with the reference's text before a plan exists; the streamed form checks the caller's arrays and lets `u` stay on the device only
when `mu` is given."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, L, NQ, NMU = 3, 3, 8, 4
MU = np.array([1.0, 0.37, 0.0, -0.62])


@pytest.fixture()
def no_plan(monkeypatch):
    """Any attempt to create a plan fails the test: the refusals come first."""
    from pydisort_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a plan was created before the inputs were refused")
    monkeypatch.setattr(_engine.Plan, "__init__", boom)


class Reached(Exception):
    pass


@pytest.fixture()
def fake_plan(monkeypatch):
    """A plan that records what reaches it and stops at run_fetch: everything before that is host code."""
    from pydisort_amd import _engine, batch
    seen = {}

    class FakePlan:
        _ACT = _engine.Plan._ACT
        numeric_errors = "raise"

        def __init__(self, prep, **k):
            self.prep, self.C, self.Q = prep, prep["C"], 2 * prep["N"]

        def set_eval_points(self, tau, phi):
            pass

        def set_eval_order(self, order):
            pass

        def set_view(self, mu):
            seen["mu"] = mu

        def run_fetch(self, out):
            seen["out"] = out
            raise Reached

        def close(self):
            seen["closed"] = True

    monkeypatch.setattr(batch, "Plan", FakePlan)
    return seen


def batch_cfg():
    rng = np.random.default_rng(12)
    leg = rng.uniform(0.3, 0.8, (C, L, 1)) ** np.arange(NQ + 3)[None, None, :]
    return dict(tau_arr=np.cumsum(rng.uniform(0.1, 1.0, (C, L)), axis=1), omega_arr=rng.uniform(0.2, 0.9, (C, L)), NQuad=NQ,
                Leg_coeffs_all=leg, mu0=np.full(C, 0.6), I0=np.ones(C), phi0=np.zeros(C), f_arr=leg[:, :, NQ])


def band_kw(**over):
    rng = np.random.default_rng(11)
    P, G, S = 2, 3, 2
    kw = dict(dtau_abs=rng.uniform(0.01, 0.5, (P, G, L)), dtau_spec=rng.uniform(0.05, 0.4, (P, L, S)),
              omega_spec=rng.uniform(0.1, 0.95, (P, L, S)), Leg_spec=np.array([0.7, 0.3])[:, None] ** np.arange(NQ + 3)[None, :],
              NQuad=NQ, mu0=0.6, I0=1.0, phi0=0.0, weights=np.full(G, 0.2))
    kw.update(over)
    return kw


TAU = np.zeros((C, 2))
PHI = np.array([0.0, 1.0])


def full_out(**over):
    out = dict(u=np.empty((C, NQ, 2, 2)), u0=np.empty((C, NQ, 2)), flux_up=np.empty((C, 2)), flux_down_diffuse=np.empty((C, 2)),
               flux_down_direct=np.empty((C, 2)))
    out.update(over)
    return {k: v for k, v in out.items() if v is not None}


BAD_MU = [
    (np.array([0.5, 1.0000001]), "mu values must be between -1 and 1."),
    (np.array([-1.5]), "mu values must be between -1 and 1."),
    (np.array([0.5, np.nan]), "mu values must be between -1 and 1."),
    (np.zeros((C + 1, 2)), "mu must have the shape"),
    (np.zeros((C, 2, 2)), "mu must have the shape"),
    (np.zeros(0), "mu must have the shape"),
]


@pytest.mark.parametrize("mu,msg", BAD_MU)
def test_bad_angles_are_refused_before_a_plan(no_plan, mu, msg):
    import pydisort_amd
    with pytest.raises(ValueError, match=re.escape(msg)):
        pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, PHI, mu=mu)
    if mu.ndim != 2:  # (per profile the leading axis is P = 2)
        with pytest.raises(ValueError, match=re.escape(msg)):
            pydisort_amd.solve_band_streamed(**band_kw(), mu=mu)
    with pytest.raises(ValueError, match=re.escape("mu must have the shape [nmu] or [P = 2, nmu]")):
        pydisort_amd.solve_band_streamed(**band_kw(), mu=np.zeros((3, 2)))


def test_u_may_stay_on_the_device_only_when_mu_is_given(fake_plan):
    import pydisort_amd
    with pytest.raises(ValueError, match=re.escape("out['u'] must be a C-contiguous float64 array")):
        pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, PHI, out=full_out(u=None))
    assert fake_plan.pop("closed")
    with pytest.raises(ValueError, match=re.escape("out['u'] must be")):
        pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, PHI, out=full_out(u=None), actinic=True)
    mine = full_out(u=None)
    with pytest.raises(Reached):
        pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, PHI, out=mine, mu=MU)
    assert fake_plan["out"] is mine and "u" not in mine and np.array_equal(fake_plan["mu"], MU) and fake_plan["closed"]
    with pytest.raises(Reached):  # per column
        pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, PHI, out=full_out(), mu=np.tile(MU, (C, 1)))
    assert fake_plan["mu"].shape == (C, NMU) and fake_plan["mu"].flags.c_contiguous


@pytest.mark.parametrize("key,bad", [
    ("u_mu", np.empty((C, NMU, 2, 3))),
    ("u_mu", np.empty((C, NMU, 2, 2), np.float32)),
    ("u_mu", np.empty((2, 2, NMU, C)).T),
    ("u0_mu", np.empty((C, NMU + 1, 2))),
    ("u0_mu", np.empty((2, NMU, C)).T),
    ("u", np.empty((C, NQ, 2, 3))),
])
def test_the_streamed_form_checks_the_callers_arrays(fake_plan, key, bad):
    import pydisort_amd
    with pytest.raises(ValueError, match=re.escape(f"out[{key!r}] must be a C-contiguous float64 array of shape")):
        pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, PHI, out=full_out(**{key: bad}), mu=MU)
    good = full_out(u_mu=np.empty((C, NMU, 2, 2)), u0_mu=np.empty((C, NMU, 2)))
    with pytest.raises(Reached):
        pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, PHI, out=good, mu=MU)


def test_only_flux_with_mu_asks_for_u0_mu_alone(fake_plan):
    import pydisort_amd
    out = full_out(u=None, u_mu=np.empty(1))  # (u_mu is not a result of this call: it is not looked at)
    with pytest.raises(Reached):
        pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, None, only_flux=True, out=out, mu=MU)
    with pytest.raises(ValueError, match=re.escape("out['u0_mu']")):
        pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, None, only_flux=True, out=full_out(u=None, u0_mu=np.empty((C, NMU, 3))), mu=MU)


def test_signatures_symbols_and_version():
    import pydisort_amd
    from pydisort_amd import _lib
    lib = _lib.load()
    for sym in ("rtd_plan_set_view_mu", "rtd_plan_fetch_view", "rtd_plan_fetch_band_view"):
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
    assert lib.rtd_version() >= 216
    assert len(_lib.SIGNATURES["rtd_plan_set_view_mu"][1]) == 4 and len(_lib.SIGNATURES["rtd_plan_fetch_view"][1]) == 3
    assert len(_lib.SIGNATURES["rtd_plan_fetch_band_view"][1]) == 3
    mu = np.array([0.5])
    assert lib.rtd_plan_set_view_mu(None, 1, _lib.dptr(mu), 0) == 1  # RTD_ERR_ARG
    assert lib.rtd_plan_fetch_view(None, None, None) == 1 and lib.rtd_plan_fetch_band_view(None, None, None) == 1
    for m in ("set_view", "fetch_view", "fetch_band_view"):
        assert hasattr(pydisort_amd._Plan, m)
    for cls, names in ((pydisort_amd.BatchSolution, ("mu", "tau", "phi")), (pydisort_amd.BandSolution, ("mu", "levels", "phi"))):
        assert list(inspect.signature(cls.u_at).parameters)[1:4] == list(names)
        assert list(inspect.signature(cls.u0_at).parameters)[1:3] == list(names[:2])
    batch_u_at = inspect.signature(pydisort_amd.BatchSolution.u_at).parameters
    assert batch_u_at["is_antiderivative_wrt_tau"].default is False
    assert batch_u_at["is_derivative_wrt_tau"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (pydisort_amd.solve_columns_streamed, pydisort_amd.solve_band_streamed):
        par = inspect.signature(fn).parameters["mu"]
        assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY
    assert pydisort_amd._Plan._view_want(("u0", "view")) == ("u", "u0") and pydisort_amd._Plan._view_want(("view_u0",)) == ("u0",)
    assert pydisort_amd._Plan._view_want(("u", "act")) == ()


def test_the_header_with_the_new_entry_points_is_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "use_view.c"
    src.write_text('#include "rtd.h"\n'
                   "int use(rtd_plan* p, const double* mu, double* u_mu, double* u0_mu) {\n"
                   "  int rc = rtd_plan_set_view_mu(p, 3, mu, 0);\n"
                   "  if (!rc) rc = rtd_plan_fetch_view(p, u_mu, u0_mu);\n"
                   "  if (!rc) rc = rtd_plan_fetch_band_view(p, u_mu, u0_mu);\n"
                   "  return rc;\n"
                   "}\n")
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    str(src)], check=True)
