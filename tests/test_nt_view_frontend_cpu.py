"""The `corrections=` keyword of the views (``Plan.set_view``, ``BatchSolution.u_at``, ``BandSolution.u_at``, `view_corrections=` of the two
streamed forms) and rtd_plan_set_view_nt behind it, before anything touches a device: the symbol is declared, bound and exported and the
header stays C99; the keyword is keyword-only with defaults that keep the interpolating mode; an unknown spelling and mu = 0 with
"at_angles" are refused before a plan exists; and, over the real host code of csrc/rtd_api.hip on the stand-in runtime
(tests/cpu/nt_view_frontend_driver.py), a request made after the evaluation leaves u_mu unavailable until the next one while u0_mu is
served."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import host_program
from test_view_frontend_cpu import PHI, TAU, band_kw, batch_cfg, no_plan  # noqa: F401  (no_plan: a fixture)

ROOT = host_program.ROOT


def test_symbol_signatures_and_version():
    import pydisort_amd
    from pydisort_amd import _engine, _lib
    lib = _lib.load()
    assert "rtd_plan_set_view_nt" in _lib.SIGNATURES and hasattr(lib, "rtd_plan_set_view_nt") and lib.rtd_version() >= 218
    assert lib.rtd_plan_set_view_nt(None, 1) == 1  # RTD_ERR_ARG
    for fn, name in ((pydisort_amd._Plan.set_view, "corrections"), (pydisort_amd.BatchSolution.u_at, "corrections"),
                     (pydisort_amd.BandSolution.u_at, "corrections"), (pydisort_amd.solve_columns_streamed, "view_corrections"),
                     (pydisort_amd.solve_band_streamed, "view_corrections")):
        par = inspect.signature(fn).parameters[name]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default == "interpolated", fn
    for cls in (pydisort_amd.BatchSolution, pydisort_amd.BandSolution):
        assert "corrections" not in inspect.signature(cls.u0_at).parameters  # (the corrections never touched u0)
    assert _engine.view_corrections("interpolated") == 0 and _engine.view_corrections("at_angles") == 1
    assert _engine.view_corrections("interpolated", np.array([0.0, 0.5])) == 0
    # the one-column drop-in and subroutines.interpolate stay as the reference has them
    assert "corrections" not in inspect.signature(pydisort_amd.pydisort).parameters
    assert list(inspect.signature(pydisort_amd.subroutines.interpolate).parameters) == ["u"]


@pytest.mark.parametrize("bad", ["exact", "At_angles", None, 1, ""])
def test_unknown_spellings_are_refused_before_a_plan(no_plan, bad):  # noqa: F811
    import pydisort_amd
    msg = re.escape('corrections must be "interpolated" or "at_angles"')
    with pytest.raises(ValueError, match=msg):
        pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, PHI, mu=np.array([0.5]), view_corrections=bad)
    with pytest.raises(ValueError, match=msg):
        pydisort_amd.solve_band_streamed(**band_kw(), mu=np.array([0.5]), view_corrections=bad)
    with pytest.raises(ValueError, match=msg):  # (checked with or without angles)
        pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, PHI, view_corrections=bad)


@pytest.mark.parametrize("mu", [np.array([0.5, 0.0]), np.array([-0.0]), np.array([[0.3, -0.2], [0.0, 0.1]])])
def test_mu_zero_is_refused_with_at_angles_before_a_plan(no_plan, mu):  # noqa: F811
    import pydisort_amd
    msg = re.escape('mu = 0 is not accepted with corrections="at_angles"')
    if mu.ndim == 1:
        with pytest.raises(ValueError, match=msg):
            pydisort_amd.solve_columns_streamed(batch_cfg(), TAU, PHI, mu=mu, view_corrections="at_angles")
    with pytest.raises(ValueError, match=msg):  # (per profile the leading axis is P = 2)
        pydisort_amd.solve_band_streamed(**band_kw(), mu=mu, view_corrections="at_angles")


def test_the_header_with_the_new_entry_point_is_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "use_view_nt.c"
    src.write_text('#include "rtd.h"\nint use(rtd_plan* p, const double* mu) {\n  int rc = rtd_plan_set_view_mu(p, 3, mu, 0);\n'
                   "  if (!rc) rc = rtd_plan_set_view_nt(p, 1);\n  return rc;\n}\n")
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    str(src)], check=True)


def test_the_keyword_over_the_real_host_code(tmp_path):
    lib = host_program.build_trace_library(tmp_path)
    env = dict(os.environ, RTD_LIB=lib, FAKE_HIP_TOTAL=str(8 << 30))
    for k in ("RTD_POOL_BYTES", "RTD_WORK_BYTES", "RTD_NO_PIPELINE", "RTD_RCCL_STUB", "PYTHONPATH"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(host_program.CPU, "nt_view_frontend_driver.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "NT VIEW FRONTEND DONE" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert "NONFINITE" not in r.stdout
    assert out.count("windows (6, 1)") == 1 and out.count("windows (4, 2)") == 1
    twice = lambda line: out.count(line) == 2  # noqa: E731  (once per plan: one window, windows of 4)
    for order in ("[]", "['is_antiderivative_wrt_tau']", "['is_derivative_wrt_tau']"):
        assert twice(f"u_at at_angles {order} -> (6, 4, 3, 2) finite")
    assert twice("u_at per column -> (6, 4, 3, 2) finite") and twice("u_at interpolated takes mu = 0 -> (6, 2, 3, 2) finite")
    assert twice("u_at unknown raises ValueError: corrections must be \"interpolated\" or \"at_angles\", not 'exact'.")
    assert twice('u_at at_angles mu = 0 raises ValueError: mu = 0 is not accepted with corrections="at_angles": the limit differs by hemisphere.')
    assert sum(line.startswith("u_at positional raises TypeError") for line in out) == 2
    # the request made after the evaluation: RTD_ERR_STATE with a message that says what to do; u0_mu is served; the next evaluation serves u_mu
    late = [i for i, line in enumerate(out) if line.startswith("fetch_view u raises RuntimeError: librtd error 4: fetch_view:")]
    assert len(late) == 2 and all("set after the latest one: evaluate again" in out[i] for i in late)
    for i in late:
        assert out[i - 1] == "set_view at_angles after the evaluation -> NoneType"
        assert out[i + 1] == "fetch_view u0 -> u0_mu(6, 4, 3)" and out[i + 2] == "evaluate view -> u_mu(6, 4, 3, 2)"
    assert any(line.startswith("streamed at_angles -> ") and "u_mu(6, 4, 3, 2)" in line and "u0_mu(6, 4, 3)" in line for line in out)
