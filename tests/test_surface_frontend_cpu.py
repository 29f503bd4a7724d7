"""Parametric surface models, before anything touches the device: the entry points of include/rtd.h (rtd_plan_request_surface,
rtd_surface_samples, rtd_plan_get_bdrf) are declared, bound and exported and the header stays C99; everything a user can get wrong
in ``surface=`` -- of ``pydisort_batch``, ``solve_columns_streamed``, ``pydisort_band`` and ``solve_band_streamed`` -- and in
``surface_reflectance`` is refused with a ValueError before a plan exists; what is accepted reaches the plan as the request
``Plan.request_surface`` takes, with no table and no sample array on the host."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, L, NQ = 3, 3, 8


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
    """A plan that records the prepared batch and stops: everything before it is host code."""
    from pydisort_amd import batch, band
    seen = {}

    class FakePlan:
        def __init__(self, prep, **k):
            seen["prep"] = prep
            raise Reached

    monkeypatch.setattr(batch, "Plan", FakePlan)
    monkeypatch.setattr(band, "Plan", FakePlan)
    return seen


def batch_cfg(**over):
    rng = np.random.default_rng(12)
    leg = rng.uniform(0.3, 0.8, (C, L, 1)) ** np.arange(NQ + 3)[None, None, :]
    cfg = dict(tau_arr=np.cumsum(rng.uniform(0.1, 1.0, (C, L)), axis=1), omega_arr=rng.uniform(0.2, 0.9, (C, L)), NQuad=NQ,
               Leg_coeffs_all=leg, mu0=np.full(C, 0.6), I0=np.ones(C), phi0=np.zeros(C), f_arr=leg[:, :, NQ])
    cfg.update(over)
    return cfg


def band_kw(**over):
    rng = np.random.default_rng(11)
    P, G, S = 2, 3, 2
    kw = dict(dtau_abs=rng.uniform(0.01, 0.5, (P, G, L)), dtau_spec=rng.uniform(0.05, 0.4, (P, L, S)),
              omega_spec=rng.uniform(0.1, 0.95, (P, L, S)), Leg_spec=np.array([0.7, 0.3])[:, None] ** np.arange(NQ + 3)[None, :],
              NQuad=NQ, mu0=0.6, I0=1.0, phi0=0.0, weights=np.full(G, 0.2))
    kw.update(over)
    return kw


ROSSLI = dict(model="rossli", params=(0.3, 0.1, 0.05))
BAD_SURFACE = [
    ("rossli", "must be a dict"),
    (dict(model="rossli"), "params is required"),
    (dict(model="oren-nayar", params=(0.3,)), "unknown model"),
    (dict(model=2, params=(0.3, 0.1, 0.05)), "unknown model"),
    (dict(ROSSLI, azimuths=64), "unknown entries ['azimuths']"),
    (dict(model="rossli", params=(0.3, 0.1)), "must have the shape"),
    (dict(model="rpv", params=(0.1, 0.8, -0.1)), "must have the shape"),
    (dict(model="rossli", params=np.full((C + 1, 3), 0.1)), "must have the shape"),
    (dict(model="rossli", params=(0.3, -0.1, 0.05)), "row 0"),
    (dict(model="rossli", params=np.array([[0.3, 0.1, 0.05], [0.3, 0.1, np.nan], [0.3, 0.1, 0.05]])), "row 1"),
    (dict(model="lambert", params=1.5), "0 <= albedo <= 1"),
    (dict(model="hapke", params=(1.0, 0.0, 0.6)), "HH > 0"),
    (dict(model="hapke", params=(1.0, 0.06, 1.2)), "0 < W <= 1"),
    (dict(model="rpv", params=(0.1, 0.8, 1.0, 0.1)), "|Theta| < 1"),
    (dict(model="rpv", params=(0.1, 0.0, 0.1, 0.1)), "k > 0"),
    (dict(ROSSLI, nphi=14), "nphi must be an integer"),       # 2 (NBDRF - 1) = 14 with NBDRF = NFourier = 8
    (dict(ROSSLI, nphi=16385), "nphi must be an integer"),
    (dict(ROSSLI, nphi=64.0), "nphi must be an integer"),
]


@pytest.mark.parametrize("surface,msg", BAD_SURFACE, ids=[m for _, m in BAD_SURFACE])
def test_bad_surfaces_are_refused_before_a_plan(no_plan, surface, msg):
    import pydisort_amd
    with pytest.raises(ValueError, match=re.escape(msg)):
        pydisort_amd.pydisort_batch(**batch_cfg(), surface=surface)
    with pytest.raises(ValueError, match=re.escape(msg)):
        pydisort_amd.solve_columns_streamed(batch_cfg(surface=surface), np.zeros((C, 2)), np.array([0.0]))
    if not (isinstance(surface, dict) and np.ndim(surface.get("params")) == 2):  # (per profile the leading axis is P = 2)
        with pytest.raises(ValueError, match=re.escape(msg)):
            pydisort_amd.pydisort_band(**band_kw(), surface=surface)
        with pytest.raises(ValueError, match=re.escape(msg)):
            pydisort_amd.solve_band_streamed(**band_kw(), surface=surface)


def test_exclusions_are_refused_before_a_plan(no_plan):
    import pydisort_amd
    N = NQ // 2
    q, q0 = np.zeros((C, 1, N, N)), np.zeros((C, 1, N))
    with pytest.raises(ValueError, match="either surface or bdrf_q"):
        pydisort_amd.pydisort_batch(**batch_cfg(), surface=ROSSLI, bdrf_q=q, bdrf_q0=q0)
    with pytest.raises(ValueError, match="either surface or bdrf_q"):
        pydisort_amd.pydisort_batch(**batch_cfg(), surface=ROSSLI, bdrf_samples=(np.zeros((C, N, N, 16)), None))
    with pytest.raises(ValueError, match="surface cannot be combined with mode_shard"):
        pydisort_amd.pydisort_batch(**batch_cfg(), surface=ROSSLI, mode_shard=(0, 2))
    with pytest.raises(ValueError, match="0 < NBDRF <= NFourier"):
        pydisort_amd.pydisort_batch(**batch_cfg(), surface=ROSSLI, NBDRF=NQ + 1)
    with pytest.raises(ValueError, match="0 < NBDRF <= NFourier"):
        pydisort_amd.pydisort_batch(**batch_cfg(), surface=ROSSLI, NBDRF=0)
    with pytest.raises(ValueError, match="either surface or bdrf_q"):
        pydisort_amd.pydisort_band(**band_kw(), surface=ROSSLI, bdrf_q=np.zeros((2, 1, N, N)), bdrf_q0=np.zeros((2, 1, N)))
    with pytest.raises(ValueError, match=re.escape("must have the shape")):
        pydisort_amd.pydisort_band(**band_kw(), surface=dict(model="rossli", params=np.full((6, 3), 0.1)))  # [P G, npar] is not a shape of a band
    # the older path keeps its refusal of Kirchhoff emissivity
    with pytest.raises(ValueError, match="give `emissivity` with bdrf_samples"):
        pydisort_amd.pydisort_batch(**batch_cfg(), bdrf_samples=(np.zeros((C, N, N, 16)), None),
                                    thermal=dict(TEMPER=np.full(L + 1, 250.0), WVNMLO=300.0, WVNMHI=800.0, BTEMP=290.0))


def test_what_is_accepted_reaches_the_plan_as_a_request(fake_plan):
    import pydisort_amd
    per_col = np.array([[0.3, 0.1, 0.05], [0.2, 0.15, 0.01], [0.1, 0.0, 0.0]])
    with pytest.raises(Reached):
        pydisort_amd.pydisort_batch(**batch_cfg(), surface=dict(model="RossLi", params=per_col, nphi=64), NBDRF=4)
    prep = fake_plan["prep"]
    sf = prep["surface"]
    assert prep["NBDRF"] == 4 and prep["raw"]["bdrf_q"] is None and prep["raw"]["bdrf_q0"] is None  # no table on the host
    assert sf["model"] == 2 and sf["nphi"] == 64 and sf["params"].shape == (C, 4) and sf["params"].flags.c_contiguous
    assert np.array_equal(sf["params"][:, :3], per_col) and np.all(sf["params"][:, 3] == 0)
    # thermal without emissivity is accepted: Kirchhoff's law reads the device-formed zeroth mode
    with pytest.raises(Reached):
        pydisort_amd.pydisort_batch(**batch_cfg(), surface=dict(model="lambert", params=0.3),
                                    thermal=dict(TEMPER=np.full(L + 1, 250.0), WVNMLO=300.0, WVNMHI=800.0, BTEMP=290.0))
    prep = fake_plan["prep"]
    assert prep["surface"]["model"] == 0 and prep["surface"]["params"].tolist() == [[0.3, 0, 0, 0]] and prep["surface"]["nphi"] == 256
    assert prep["NBDRF"] == NQ and prep["thermal"]["emissivity"] is None and prep["Ns"] == 2
    with pytest.raises(Reached):  # one albedo per column
        pydisort_amd.pydisort_batch(**batch_cfg(), surface=dict(model="lambert", params=np.array([0.1, 0.2, 0.3])), only_flux=True)
    assert fake_plan["prep"]["surface"]["params"][:, 0].tolist() == [0.1, 0.2, 0.3] and fake_plan["prep"]["NBDRF"] == 1
    with pytest.raises(Reached):
        pydisort_amd.solve_columns_streamed(batch_cfg(surface=dict(model="rpv", params=(0.1, 0.8, -0.1, 0.1)), NBDRF=2), np.zeros((C, 2)), np.array([0.0]))
    assert fake_plan["prep"]["surface"]["model"] == 3 and fake_plan["prep"]["NBDRF"] == 2
    # a band: shared, per profile [P, npar] (P rows: the device shares a row among the profile's G columns), per column [P, G, npar]
    for params, rows in (((1.0, 0.06, 0.6), 1), (np.tile((1.0, 0.06, 0.6), (2, 1)), 2), (np.tile((1.0, 0.06, 0.6), (2, 3, 1)), 6)):
        with pytest.raises(Reached):
            pydisort_amd.pydisort_band(**band_kw(), surface=dict(model="hapke", params=params, nphi=32), NBDRF=3)
        prep = fake_plan["prep"]
        assert prep["surface"]["params"].shape == (rows, 4) and prep["NBDRF"] == 3 and prep["cols"]["bdrf_q"] is None
    with pytest.raises(Reached):
        pydisort_amd.solve_band_streamed(**band_kw(), surface=dict(model="hapke", params=(1.0, 0.06, 0.6)))
    assert fake_plan["prep"]["surface"]["nphi"] == 256 and fake_plan["prep"]["NBDRF"] == NQ


BAD_REFLECTANCE = [
    (("oren", (0.3,), 0.5, 0.5, 16), "unknown model"),
    (("rossli", (0.3, 0.1), 0.5, 0.5, 16), "must have the shape"),
    (("rossli", (0.3, 0.1, -0.05), 0.5, 0.5, 16), "row 0"),
    (("rossli", (0.3, 0.1, 0.05), 0.0, 0.5, 16), "must lie in (0, 1]"),
    (("rossli", (0.3, 0.1, 0.05), 0.5, 1.5, 16), "must lie in (0, 1]"),
    (("rossli", (0.3, 0.1, 0.05), 0.5, 0.5, 0), "nphi must be an integer"),
    (("rossli", (0.3, 0.1, 0.05), 0.5, 0.5, 16385), "nphi must be an integer"),
    (("rossli", np.full((2, 3), 0.1), np.full(3, 0.5), 0.5, 16), "do not broadcast"),
]


@pytest.mark.parametrize("args,msg", BAD_REFLECTANCE, ids=[m + str(i) for i, (_, m) in enumerate(BAD_REFLECTANCE)])
def test_surface_reflectance_refuses_on_the_host(monkeypatch, args, msg):
    import pydisort_amd
    from pydisort_amd import _lib

    def boom():
        raise AssertionError("the library was reached before the inputs were refused")
    monkeypatch.setattr(_lib, "load", boom)
    with pytest.raises(ValueError, match=re.escape(msg)):
        pydisort_amd.surface_reflectance(*args)


def test_signatures_symbols_and_version():
    import ctypes
    import pydisort_amd
    from pydisort_amd import _lib, _surface
    lib = _lib.load()
    for sym in ("rtd_plan_request_surface", "rtd_surface_samples", "rtd_plan_get_bdrf"):
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
    assert lib.rtd_version() >= 217
    assert len(_lib.SIGNATURES["rtd_plan_request_surface"][1]) == 2 and len(_lib.SIGNATURES["rtd_surface_samples"][1]) == 8
    assert len(_lib.SIGNATURES["rtd_plan_get_bdrf"][1]) == 3
    assert [n for n, _ in _lib.rtd_surface._fields_] == ["model", "nphi", "rows", "params"]
    assert ctypes.sizeof(_lib.rtd_surface) == 24
    assert lib.rtd_plan_request_surface(None, None) == 1 and lib.rtd_plan_get_bdrf(None, None, None) == 1  # RTD_ERR_ARG
    assert lib.rtd_surface_samples(0, 7, 1, None, None, None, 4, None) == 1
    assert lib.rtd_surface_samples(0, 0, 0, None, None, None, 4, None) == 0  # (n = 0 touches no device)
    hdr = open(os.path.join(ROOT, "include", "rtd.h")).read()
    for name, (mid, _) in _surface.MODELS.items():
        assert re.search(rf"RTD_SURFACE_{name.upper()} = {mid}\b", hdr)
    assert " *   RTD_SURFACE_BYTES " in hdr
    for m in ("request_surface", "get_bdrf"):
        assert hasattr(pydisort_amd._Plan, m)
    assert "surface_reflectance" in pydisort_amd.__all__
    assert list(inspect.signature(pydisort_amd.surface_reflectance).parameters)[:5] == ["model", "params", "mu", "mu_p", "nphi"]
    for fn in (pydisort_amd.pydisort_batch, pydisort_amd.pydisort_band, pydisort_amd.solve_band_streamed):
        assert inspect.signature(fn).parameters["surface"].default is None
    for fn in (pydisort_amd.pydisort_band, pydisort_amd.solve_band_streamed):
        assert inspect.signature(fn).parameters["NBDRF"].default is None


def test_the_header_with_the_new_entry_points_is_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "use_surface.c"
    src.write_text('#include "rtd.h"\n'
                   "int use(rtd_plan* p, const double* par, const double* mu, double* rho, double* q, double* q0) {\n"
                   "  rtd_surface sf;\n"
                   "  int rc;\n"
                   "  sf.model = RTD_SURFACE_ROSSLI; sf.nphi = 256; sf.rows = 1; sf.params = par;\n"
                   "  rc = rtd_plan_request_surface(p, &sf);\n"
                   "  if (!rc) rc = rtd_surface_samples(0, RTD_SURFACE_RPV, 4, par, mu, mu, 16, rho);\n"
                   "  if (!rc) rc = rtd_plan_get_bdrf(p, q, q0);\n"
                   "  if (!rc) rc = rtd_plan_request_surface(p, 0);\n"
                   "  return rc + RTD_SURFACE_LAMBERT + RTD_SURFACE_HAPKE;\n"
                   "}\n")
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    str(src)], check=True)
