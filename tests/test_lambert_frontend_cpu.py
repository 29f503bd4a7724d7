"""``lambert_sweep=True`` of ``pydisort_batch`` / ``pydisort_band`` and the entry points behind it (rtd_plan_couple_lambert,
rtd_plan_couple_lambert_band, rtd_lambert_kappa), before anything touches a device: the symbols are declared, bound and exported and
the header stays C99; everything the keyword excludes is refused before a plan exists; and, over the real host code of
csrc/rtd_api.hip on the traced stand-in runtime (tests/cpu/lambert_frontend_driver.py), the front end builds the companion it should,
every evaluator of the sweep returns the albedo axis where it belongs, makes the launches it should and no solve on a retained plan,
a batch that never asks launches nothing of it, and bad albedos, emissions and shapes are ValueErrors of the front end."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import host_program
from test_view_frontend_cpu import band_kw, batch_cfg, no_plan  # noqa: F401  (no_plan: a fixture)

ROOT = host_program.ROOT
C, N = 3, 4


def test_symbols_signatures_and_version():
    import pydisort_amd
    from pydisort_amd import _lib
    lib = _lib.load()
    for sym in ("rtd_plan_couple_lambert", "rtd_plan_couple_lambert_band", "rtd_lambert_kappa"):
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
    assert lib.rtd_version() >= 219
    assert len(_lib.SIGNATURES["rtd_plan_couple_lambert"][1]) == 14 and len(_lib.SIGNATURES["rtd_plan_couple_lambert_band"][1]) == 14
    null = [None, None, 1, None, 1] + [None] * 9  # (null plans: RTD_ERR_ARG)
    assert lib.rtd_plan_couple_lambert(*null) == 1 and lib.rtd_plan_couple_lambert_band(*null) == 1
    for fn in (pydisort_amd.pydisort_batch, pydisort_amd.pydisort_band):
        assert inspect.signature(fn).parameters["lambert_sweep"].default is False
    for fn in (pydisort_amd.pydisort, pydisort_amd.solve_columns_streamed, pydisort_amd.solve_band_streamed):
        assert "lambert_sweep" not in inspect.signature(fn).parameters  # out of scope: the one-column drop-in and the streamed forms
    for m in ("couple_lambert", "couple_lambert_band", "evaluate_resident"):
        assert hasattr(pydisort_amd._Plan, m)
    for cls, sweep, point in ((pydisort_amd.BatchSolution, pydisort_amd.LambertSweep, "tau"), (pydisort_amd.BandSolution, pydisort_amd.BandLambertSweep, "levels")):
        assert list(inspect.signature(cls.lambert).parameters)[1:] == ["albedo", "emission", "BTEMP"] and hasattr(cls, "lambert_terms")
        for name in ("u", "u0", "flux_up", "flux_down", "u_at", "u0_at"):
            assert list(inspect.signature(getattr(sweep, name)).parameters) == list(inspect.signature(getattr(cls, name)).parameters), name
        assert point in inspect.signature(sweep.u0).parameters
    for name in ("LambertSweep", "BandLambertSweep", "lambert_kappa"):
        assert name in pydisort_amd.__all__


REFUSED = [
    (dict(bdrf_q=np.zeros((C, 1, N, N)), bdrf_q0=np.zeros((C, 1, N))), "lambert_sweep cannot be combined with bdrf_q"),
    (dict(bdrf_q0=np.zeros((C, 1, N))), "lambert_sweep cannot be combined with bdrf_q0"),
    (dict(bdrf_samples=(np.zeros((C, N, N, 8)), None)), "lambert_sweep cannot be combined with bdrf_samples"),
    (dict(surface=dict(model="lambert", params=0.3)), "lambert_sweep cannot be combined with surface"),
    (dict(mode_shard=(0, 2)), "lambert_sweep cannot be combined with mode_shard"),
    (dict(b_pos=0.5), "lambert_sweep needs b_pos = 0"),
    (dict(b_pos=np.full((C, N), 1e-300)), "lambert_sweep needs b_pos = 0"),
    (dict(thermal=dict(TEMPER=np.full(4, 250.0), WVNMLO=500.0, WVNMHI=600.0, BTEMP=280.0)), "BTEMP and emissivity belong to lambert("),
    (dict(thermal=dict(TEMPER=np.full(4, 250.0), WVNMLO=500.0, WVNMHI=600.0, emissivity=0.9)), "BTEMP and emissivity belong to lambert("),
    (dict(_defer_solve=True), "lambert_sweep is not available in the streamed forms"),
]


@pytest.mark.parametrize("extra,msg", REFUSED)
def test_what_the_keyword_excludes_is_refused_before_a_plan(no_plan, extra, msg):  # noqa: F811
    import pydisort_amd
    with pytest.raises(ValueError, match=re.escape(msg)):
        pydisort_amd.pydisort_batch(**batch_cfg(), **extra, lambert_sweep=True)
    band_extra = {k: v for k, v in extra.items() if k not in ("bdrf_samples", "mode_shard")}
    if "b_pos" in band_extra and np.ndim(band_extra["b_pos"]) == 2:
        band_extra["b_pos"] = np.full((2, N), 1e-300)  # (per profile: P = 2)
    if "bdrf_q" in band_extra or "bdrf_q0" in band_extra:
        band_extra = {k: v[:2] for k, v in band_extra.items()}
    if band_extra:
        with pytest.raises(ValueError, match=re.escape(msg)):
            pydisort_amd.pydisort_band(**band_kw(), **band_extra, lambert_sweep=True)


def test_the_small_arrays_are_checked_on_the_host():
    from pydisort_amd import _engine
    F, s = np.ones(C), np.full(C, 0.2)
    alb, f, sp, E = _engine.lambert_arrays([0.0, 0.5, 1.0], (C,), F, s, 1.7, C)
    assert alb.shape == (3,) and E.shape == (C,) and E.flags.c_contiguous and np.all(E == 1.7)
    assert _engine.lambert_arrays(np.zeros((C, 2)), (C,), F, s, None, C)[3] is None
    for bad, msg in ((np.array([0.2, 1.0000001]), "albedo values must be between 0 and 1."), (np.array([-1e-12]), "albedo values must be"),
                     (np.array([np.nan]), "albedo values must be"), (np.zeros((C + 1, 2)), "albedo must have the shape"), (np.zeros(0), "albedo must have the shape"),
                     (np.zeros((C, 2, 2)), "albedo must have the shape")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            _engine.lambert_arrays(bad, (C,), F, s, None, C)
    for bad in (-1.0, np.inf, np.nan, np.full(C, -0.1)):
        with pytest.raises(ValueError, match=re.escape("emission must be finite and not negative.")):
            _engine.lambert_arrays([0.5], (C,), F, s, bad, C)
    with pytest.raises(ValueError, match=re.escape("emission must be a scalar or [C = 3].")):
        _engine.lambert_arrays([0.5], (C,), F, s, np.zeros(C + 1), C)
    with pytest.raises(ValueError, match=re.escape("fdown_bottom and sph_albedo must have the shape [C = 3].")):
        _engine.lambert_arrays([0.5], (C,), np.ones(C + 1), s, None, C)


def test_the_header_with_the_new_entry_points_is_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "use_lambert.c"
    src.write_text('#include "rtd.h"\n'
                   "int use(rtd_plan* a, rtd_plan* b, const double* alb, const double* F, const double* s, double* out, int32_t* flag) {\n"
                   "  int rc = rtd_plan_couple_lambert(a, b, 4, alb, 1, F, s, 0, out, 0, 0, 0, 0, 0);\n"
                   "  if (!rc) rc = rtd_plan_couple_lambert_band(a, b, 4, alb, 1, F, s, 0, 0, out, 0, 0, 0, 0);\n"
                   "  if (!rc) rc = rtd_lambert_kappa(0, 8, 4, alb, 1, F, s, 0, out, flag);\n"
                   "  return rc;\n"
                   "}\n")
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    str(src)], check=True)


def test_the_keyword_over_the_real_host_code(tmp_path):
    lib = host_program.build_trace_library(tmp_path)
    env = dict(os.environ, RTD_LIB=lib, FAKE_HIP_TOTAL=str(8 << 30))
    for k in ("RTD_POOL_BYTES", "RTD_WORK_BYTES", "RTD_NO_PIPELINE", "RTD_RCCL_STUB", "RTD_LAMBERT_BYTES", "PYTHONPATH"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(host_program.CPU, "lambert_frontend_driver.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "LAMBERT FRONTEND DONE" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    twice = lambda line: out.count(line) == 2  # noqa: E731  (once per plan pair: one window, retained windows of 4)
    starts = lambda prefix: [line for line in out if line.startswith(prefix)]  # noqa: E731
    # a batch that never asks launches nothing of the sweep, and refuses its methods
    assert out.count("plain u -> (6, 8, 3, 2) finite | kappa 0 couple 0 reduce 0 solves 0") == 1
    assert out.count("plain lambert raises ValueError: lambert needs a solution made with lambert_sweep=True.") == 1
    # the companion: one mode, no beam, no source, no BDRF, the first NLeg moments; the same windows and retention as the primary
    assert twice("companion 1 False 0 0 (6, 3, 8)")
    assert out.count("windows (6, 1) (6, 1) retained full full") == 1 and out.count("windows (4, 2) (4, 2) retained full full") == 1
    assert twice("lambert_terms -> flux_down_bottom(6,) spherical_albedo(6,) | kappa 0 couple 0 reduce 0 solves 0") and twice("kappa (6, 4) (6,)")
    # shapes: the albedo axis after the column axis; one kappa launch per call, one couple launch per output, no solve
    shapes = {"u": "(6, 4, 8, 3, 2)", "u0 ['is_antiderivative_wrt_tau']": "(6, 4, 8, 3)", "u0 ['is_derivative_wrt_tau']": "(6, 4, 8, 3)",
              "u_at": "(6, 4, 3, 3, 2)", "u_at at_angles": "(6, 4, 3, 3, 2)", "u0_at per column": "(6, 4, 3, 3)"}
    for label, shape in shapes.items():
        lines = starts(f"{label} -> {shape}")
        assert len(lines) == 2 and all(line.endswith("| kappa 1 couple 1 reduce 0 solves 0") for line in lines), label
    for label in ("flux_up -> (6, 4, 3)", "flux_down -> (6, 4, 3)", "per column flux_up -> (6, 4, 3)"):
        lines = starts(label)
        assert len(lines) == 2 and all(line.endswith("| kappa 1 couple 2 reduce 0 solves 0") for line in lines), label
    assert all(" (6, 4, 3) |" in line for line in starts("flux_down -> "))  # (the direct part: finite, broadcast over the albedos)
    assert len(starts("below u0_at -> (6, 3, 1) finite")) == 2
    assert len(starts("Plan.couple_lambert -> flux_down_diffuse(6, 4, 3)")) == 2 and all("u(6, 4, 8, 3, 2)" in line and "couple 3" in line
                                                                                         for line in starts("Plan.couple_lambert -> "))
    # refusals of the front end, with their texts
    assert twice("u both orders raises ValueError: `is_derivative_wrt_tau` and `is_antiderivative_wrt_tau` cannot both be set.")
    assert twice("tau out of range raises ValueError: tau input outside the tau range specified for the atmosphere (check `tau_arr`).")
    assert twice("lambert bad albedo raises ValueError: albedo values must be between 0 and 1.")
    assert twice("lambert bad rows raises ValueError: albedo must have the shape [A] or [rows, A] with rows in [6] and A >= 1.")
    assert twice("lambert bad emission raises ValueError: emission must be finite and not negative.")
    assert twice("lambert BTEMP without thermal raises ValueError: BTEMP needs the band of thermal= (WVNMLO, WVNMHI).")
    assert twice("Plan.couple_lambert_band without weights raises ValueError: set_band_weights must precede couple_lambert_band.")
    assert len(starts("Plan.couple_lambert itself raises RuntimeError: librtd error 4: couple_lambert: the companion must have one Fourier mode")) == 2
    # thermal: BTEMP through planck_band over the band of thermal=
    assert "emission (6,)" in out and len(starts("thermal flux_up -> (6, 4, 3)")) == 1
    assert "emission and BTEMP raises ValueError: Give either emission or BTEMP, not both." in out
    # the band: [P, K, A, ...]; the coupling precedes the reduction (one reduce per output; the flux evaluator reduces the primary's three too)
    assert "band lambert_terms -> flux_down_bottom(2, 3) spherical_albedo(2, 3) | kappa 0 couple 0 reduce 0 solves 0" in out
    assert out.count("band kappa (2, 3, 4)") == 3
    for label in ("[A]", "[P, A]", "[P, G, A]"):
        assert len(starts(f"band flux_up {label} -> (2, 2, 4, 4)")) == 1 and starts(f"band flux_up {label}")[0].endswith("| kappa 1 couple 2 reduce 5 solves 0")
        assert len(starts(f"band u {label} -> (2, 2, 4, 8, 2, 2)")) == 1 and starts(f"band u {label}")[0].endswith("| kappa 1 couple 1 reduce 1 solves 0")
    assert len(starts("band flux_down -> (2, 2, 4, 3)")) == 1 and len(starts("band u_at -> (2, 2, 4, 3, 2, 2)")) == 1
    assert len(starts("band u0_at per profile -> (2, 2, 4, 3, 4)")) == 1
    assert len(starts("band lambert bad shape raises ValueError: albedo must have the shape [A], [P = 2, A] or [P, G = 3, A].")) == 1
    assert len(starts("band lambert bad spectral shape raises ValueError: albedo must have the shape")) == 1
