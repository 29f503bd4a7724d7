"""pydisort_batch(thermal=...): every error a user can make is a ValueError raised BEFORE a plan is created (so none of this
needs a GPU: without one, reaching the device would be a RuntimeError), and include/rtd.h with the thermal entry points is
still plain C99."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, L, NQ = 3, 2, 8


def call(thermal, **kw):
    import pydisort_amd
    args = dict(tau_arr=np.tile([0.5, 1.5], (C, 1)), omega_arr=0.3, NQuad=NQ, Leg_coeffs_all=np.tile(0.5 ** np.arange(NQ + 1), (L, 1)),
                mu0=0.5, I0=0.0, phi0=0.0, only_flux=True, thermal=thermal)
    args.update(kw)
    return pydisort_amd.pydisort_batch(**args)


GOOD = dict(TEMPER=[250.0, 260.0, 270.0], WVNMLO=300.0, WVNMHI=800.0, BTEMP=280.0, TTEMP=100.0, TEMIS=0.5)


@pytest.mark.parametrize("thermal, kw, match", [
    (GOOD, dict(s_poly_coeffs=np.ones((C, L, 2))), "either s_poly_coeffs or thermal"),
    (GOOD, dict(bdrf_samples=(np.zeros((C, NQ // 2, NQ // 2, 8)), None)), "emissivity"),
    (dict(GOOD, TEMPER=[250.0, 260.0]), {}, "Missing temperature specification at some boundaries / interfaces."),
    (dict(GOOD, TEMPER=np.full((C, L + 2), 250.0)), {}, "Missing temperature specification at some boundaries / interfaces."),
    (dict(GOOD, TEMPER=[250.0, -1.0, 270.0]), {}, "TEMPER must not be negative"),
    (dict(GOOD, BTEMP=-5.0), {}, "BTEMP must not be negative"),
    (dict(GOOD, TTEMP=[100.0, -100.0, 100.0]), {}, "TTEMP must not be negative"),
    (dict(GOOD, WVNMLO=900.0), {}, "0 <= WVNMLO <= WVNMHI"),
    (dict(GOOD, WVNMLO=-1.0), {}, "0 <= WVNMLO <= WVNMHI"),
    (dict(GOOD, WVNMLO=[300.0, 300.0, 801.0]), {}, "0 <= WVNMLO <= WVNMHI"),
    (GOOD, dict(NT_cor=True), "device_prepare cannot be combined"),
    (GOOD, dict(mode_shard=(0, 2), only_flux=False), "device_prepare cannot be combined"),
    (dict(GOOD, emissivity=np.ones((C, 2))), {}, "emissivity must be"),
    (dict(GOOD, BTEMP=[280.0, 280.0]), {}, "BTEMP must be a scalar or"),
    (dict(GOOD, TEMP=1.0), {}, "unknown entries"),
    ({k: v for k, v in GOOD.items() if k != "WVNMHI"}, {}, "WVNMHI is required"),
])
def test_thermal_errors_are_raised_before_any_device_work(thermal, kw, match):
    with pytest.raises(ValueError, match=match):
        call(thermal, **kw)


def test_pydisort_keeps_the_reference_signature():
    import inspect
    import pydisort_amd
    assert "thermal" not in inspect.signature(pydisort_amd.pydisort).parameters
    assert "thermal" in inspect.signature(pydisort_amd.pydisort_batch).parameters
    assert callable(pydisort_amd.planck_band)


def test_header_with_the_thermal_entry_points_is_c99(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include "rtd.h"\n'
                   "int f(rtd_plan* p, const double* a, const rtd_thermal* th) {\n"
                   "  rtd_thermal t = {0, 0, 0, 0, 0, 0, 0};\n"
                   "  double out[1];\n"
                   "  (void)t;\n"
                   "  return rtd_plan_set_columns_thermal(p, a, a, a, 4, a, a, a, a, 0, 0, 0, 0, th) + rtd_planck_band(0, 1, a, a, a, out);\n"
                   "}\n")
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    str(src)], check=True)
