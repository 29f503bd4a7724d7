"""Nakajima-Tanaka corrections on the device-prepared entries -- pydisort_batch(device_prepare=True, NT_cor=True),
solve_columns_streamed, pydisort_band / solve_band_streamed(NT_cor=True) -- before anything touches the device: every refusal is a
ValueError raised before a plan exists, the new entry points (include/rtd.h: rtd_plan_request_nt, rtd_plan_get_nt) are declared,
bound and exported, and the header stays C99."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, G, S, L, NQ = 2, 3, 2, 3, 8


@pytest.fixture()
def no_plan(monkeypatch):
    """Any attempt to create a plan fails the test: the refusals come first."""
    from pydisort_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a plan was created before the inputs were refused")
    monkeypatch.setattr(_engine.Plan, "__init__", boom)


def _node(NQuad):
    from pydisort_amd._prepare import double_gauss
    return float(double_gauss(NQuad // 2)[0][1])


def band_kw(**over):
    rng = np.random.default_rng(11)
    kw = dict(dtau_abs=rng.uniform(0.01, 0.5, (P, G, L)), dtau_spec=rng.uniform(0.05, 0.4, (P, L, S)),
              omega_spec=rng.uniform(0.1, 0.95, (P, L, S)), Leg_spec=np.array([0.7, 0.3])[:, None] ** np.arange(NQ + 3)[None, :],
              NQuad=NQ, mu0=0.6, I0=1.0, phi0=0.0, weights=np.full(G, 0.2), NT_cor=True)
    kw.update(over)
    return kw


def batch_kw(**over):
    rng = np.random.default_rng(12)
    C = 3
    leg = rng.uniform(0.3, 0.8, (C, L, 1)) ** np.arange(NQ + 3)[None, None, :]
    kw = dict(tau_arr=np.cumsum(rng.uniform(0.1, 1.0, (C, L)), axis=1), omega_arr=rng.uniform(0.2, 0.9, (C, L)), NQuad=NQ,
              Leg_coeffs_all=leg, mu0=np.full(C, 0.6), I0=np.ones(C), phi0=np.zeros(C), f_arr=leg[:, :, NQ], NT_cor=True,
              device_prepare=True)
    kw.update(over)
    return kw


BAND_BAD = [
    (dict(delta_M=False), "NT_cor needs delta_M"),
    (dict(delta_M=False, Leg_spec=np.array([0.7, 0.3])[:, None] ** np.arange(NQ)[None, :]), "NT_cor needs"),
    (dict(Leg_spec=np.array([0.7, 0.3])[:, None] ** np.arange(NQ)[None, :]), "more Legendre coefficients"),
    (dict(I0=np.array([1.0, 0.0, 1.0])), "NT_cor needs a beam source in every column"),
    (dict(mu0=_node), "Some quadrature angles come too close to `mu0`"),
    (dict(thermal=dict(TEMPER=np.full(L + 1, 250.0), WVNMLO=500.0, WVNMHI=900.0)), "NT_cor is not combined with thermal"),
]


@pytest.mark.parametrize("streamed", [False, True])
@pytest.mark.parametrize("override,msg", BAND_BAD)
def test_band_refusals_come_before_a_plan(no_plan, override, msg, streamed):
    import pydisort_amd
    over = {k: (v(NQ) if callable(v) else v) for k, v in override.items()}
    fn = pydisort_amd.solve_band_streamed if streamed else pydisort_amd.pydisort_band
    with pytest.raises(ValueError, match=re.escape(msg)):
        fn(**band_kw(**over))


BATCH_BAD = [
    (dict(I0=np.array([1.0, 0.0, 1.0])), "NT_cor needs a beam source in every column"),
    (dict(NLeg=NQ, Leg_coeffs_all="truncate"), "NLeg < number of Legendre coefficients"),
    (dict(mu0="node"), "Some quadrature angles come too close to `mu0`"),
    (dict(mode_shard=(0, 2)), "device_prepare cannot be combined"),
    (dict(thermal=dict(TEMPER=np.full(L + 1, 250.0), WVNMLO=500.0, WVNMHI=900.0)), "device_prepare cannot be combined"),
]


@pytest.mark.parametrize("override,msg", BATCH_BAD)
def test_batch_refusals_come_before_a_plan(no_plan, override, msg):
    import pydisort_amd
    kw = batch_kw()
    for k, v in override.items():
        if isinstance(v, str) and v == "truncate":
            kw[k] = kw[k][:, :, :NQ]
        elif isinstance(v, str) and v == "node":
            kw[k] = np.array([0.6, _node(NQ), 0.6])
        else:
            kw[k] = v
    with pytest.raises(ValueError, match=re.escape(msg)):
        pydisort_amd.pydisort_batch(**kw)
    if "mode_shard" not in override:  # the streamed form takes the same dict
        cfg = {k: v for k, v in kw.items() if k != "device_prepare"}
        with pytest.raises(ValueError, match=re.escape(msg)):
            pydisort_amd.solve_columns_streamed(cfg, np.zeros((3, 1)), [0.0])


def test_only_flux_ignores_nt_cor_in_the_checks(monkeypatch):
    """With only_flux there is no u to correct: the inputs that NT_cor alone would refuse reach the plan."""
    import pydisort_amd
    from pydisort_amd import _engine

    class Reached(Exception):
        pass

    def reached(self, prep, **k):
        assert not prep.get("nt")
        raise Reached
    monkeypatch.setattr(_engine.Plan, "__init__", reached)
    with pytest.raises(Reached):
        pydisort_amd.pydisort_band(**band_kw(delta_M=False, only_flux=True))
    with pytest.raises(Reached):
        pydisort_amd.pydisort_batch(**batch_kw(I0=np.array([1.0, 0.0, 1.0]), only_flux=True))


def test_the_request_reaches_the_plan(monkeypatch):
    import pydisort_amd
    from pydisort_amd import _engine
    seen = []

    class Reached(Exception):
        pass

    def reached(self, prep, **k):
        seen.append(prep.get("nt"))
        raise Reached
    monkeypatch.setattr(_engine.Plan, "__init__", reached)
    for call in (lambda: pydisort_amd.pydisort_band(**band_kw()), lambda: pydisort_amd.pydisort_batch(**batch_kw()),
                 lambda: pydisort_amd.pydisort_batch(**batch_kw(NT_cor=False))):
        with pytest.raises(Reached):
            call()
    assert seen[0] == NQ + 3 and seen[1] == NQ + 3 and not seen[2]


def test_signatures_symbols_and_version():
    import pydisort_amd
    from pydisort_amd import _lib
    band = list(inspect.signature(pydisort_amd.pydisort_band).parameters)
    streamed = inspect.signature(pydisort_amd.solve_band_streamed).parameters
    assert band[-1] == "NT_cor" and inspect.signature(pydisort_amd.pydisort_band).parameters["NT_cor"].default is False
    assert list(streamed)[-1] == "NT_cor" and streamed["NT_cor"].default is False
    lib = _lib.load()
    for sym in ("rtd_plan_request_nt", "rtd_plan_get_nt"):
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
    assert lib.rtd_version() >= 215
    for m in ("request_nt", "get_nt"):
        assert hasattr(pydisort_amd._Plan, m)
    assert lib.rtd_plan_request_nt(None, 12) == 1 and lib.rtd_plan_get_nt(None, None, None, None, None, None) == 1  # RTD_ERR_ARG


def test_the_header_with_the_new_entry_points_is_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "use_nt.c"
    src.write_text('#include "rtd.h"\n'
                   "int use(rtd_plan* p, double* w, double* f, double* c, double* q) {\n"
                   "  int32_t rows = 0;\n"
                   "  int rc = rtd_plan_request_nt(p, 12);\n"
                   "  if (!rc) rc = rtd_plan_get_nt(p, w, f, c, q, &rows);\n"
                   "  return rc ? rc : (int)rows;\n"
                   "}\n")
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    str(src)], check=True)
