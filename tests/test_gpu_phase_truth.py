"""Every kernel class against 40-digit truth on phase functions beyond Henyey-Greenstein with 0 <= g < 1 (tests/phase_cases.py:
isotropic, Rayleigh, backscattering and double Henyey-Greenstein, a short expansion padded with zeros, cloud C1; near-conservative
layers up to 128 streams), one column at a time and the six columns of a stream count stacked into one batch.  The fixtures are
tests/golden/hp/phase_<NQuad>_<column>.npz (tools/hp_truth_case.py phase ...); tests/test_phase_truth_cpu.py checks them on the CPU.

Held, per case: u, u0, flux_up and both parts of flux_down within  min(10 x MEASURED, ceiling)  of the truth, in both metrics of
goldens.max_rel_err (of the scale / pointwise where |truth| > 1e-8 max|truth|).  Ceilings:
1e-9 / 1e-6 up to 32 streams, 2e-9 / 1e-6 at 34 ... 64, 2e-8 / 1e-7 at 66 ... 128.  Per batch: the same, and every column within
1e-12 of the scale of its one-column solve (the bar of tools/fuzz_batch.py).

MEASURED: the worst of the five quantities, of the one-column solve and of the batch column, on one MI355X; beside it the
float64 oracle's (= the reference's algorithm) distance from the same truth for u, as the fixture records it.
The inputs are well posed where the oracle is furthest off: one ulp of every omega and moment moves the truth of 126_c1 by 2.4e-16
and of 126_c0 by 5.1e-16 of the scale (oracle: 4.0e-4, 6.5e-5).
"""
import warnings

import numpy as np
import pytest

import goldens
import phase_cases as P

pytestmark = pytest.mark.gpu

QUANTITIES = ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct")
BATCH_VS_ONE_COLUMN = 1e-12

#   case: (of the scale, pointwise)         oracle's u: of the scale / pointwise
MEASURED = {
    "6_c0": (5.3e-14, 4.1e-13),     # 2.8e-10 / 3.3e-10
    "6_c1": (5.6e-14, 6.4e-14),     # 1.3e-09 / 2.4e-09
    "6_c2": (3.2e-16, 2.8e-15),     # 1.5e-14 / 1.3e-13
    "6_c3": (6.0e-14, 1.7e-13),     # 7.6e-14 / 2.1e-13
    "6_c4": (4.3e-15, 1.4e-13),     # 1.1e-14 / 5.5e-14
    "6_c5": (3.5e-14, 1.2e-13),     # 8.9e-11 / 3.3e-10
    "14_c0": (6.6e-14, 2.2e-13),    # 5.5e-09 / 7.2e-09
    "14_c1": (1.4e-13, 4.8e-13),    # 9.3e-09 / 2.1e-08
    "14_c2": (4.3e-16, 9.3e-15),    # 6.5e-14 / 8.5e-13
    "14_c3": (6.4e-15, 6.7e-14),    # 1.7e-13 / 5.6e-13
    "14_c4": (1.9e-14, 2.6e-13),    # 8.5e-14 / 7.9e-13
    "14_c5": (1.6e-14, 5.0e-14),    # 1.0e-09 / 6.4e-09
    "30_c0": (1.6e-13, 1.3e-12),    # 1.5e-08 / 2.1e-08
    "30_c1": (1.4e-13, 2.3e-13),    # 2.8e-07 / 6.2e-07
    "30_c2": (2.4e-15, 4.7e-14),    # 8.8e-13 / 1.4e-11
    "30_c3": (1.2e-14, 2.6e-13),    # 3.6e-13 / 2.7e-12
    "30_c4": (3.1e-14, 3.3e-13),    # 2.7e-12 / 2.7e-11
    "30_c5": (1.7e-14, 9.5e-14),    # 4.7e-09 / 5.0e-08
    "62_c0": (7.0e-13, 6.0e-12),    # 1.5e-05 / 2.1e-05
    "62_c1": (1.6e-13, 2.4e-13),    # 5.7e-06 / 1.3e-05
    "62_c2": (2.3e-14, 3.7e-13),    # 2.0e-11 / 3.9e-10
    "62_c3": (1.3e-13, 9.7e-12),    # 3.7e-11 / 3.7e-10
    "62_c4": (1.3e-12, 1.1e-11),    # 2.0e-10 / 1.5e-09
    "62_c5": (6.5e-14, 7.8e-13),    # 6.1e-08 / 1.4e-06
    "126_c0": (4.0e-13, 3.4e-12),   # 6.5e-05 / 1.4e-04
    "126_c1": (9.9e-13, 9.9e-13),   # 4.0e-04 / 9.8e-04
    "126_c2": (2.5e-15, 5.2e-14),   # 1.0e-09 / 2.1e-08
    "126_c3": (5.4e-14, 1.3e-11),   # 6.5e-11 / 3.2e-09
    "126_c4": (8.2e-12, 1.5e-10),   # 4.5e-09 / 4.8e-08
    "126_c5": (1.2e-12, 1.1e-9),    # 3.9e-06 / 2.8e-04
    "8_c5": (4.5e-14, 1.1e-13),     # 1.9e-10 / 1.0e-09
    "16_c5": (2.7e-14, 2.0e-13),    # 9.1e-10 / 6.0e-09
    "32_c5": (1.8e-13, 1.3e-12),    # 2.9e-09 / 2.7e-08
    "64_c5": (4.2e-14, 4.4e-13),    # 6.5e-08 / 1.4e-06
    "128_c5": (9.4e-14, 2.9e-10),   # 9.9e-07 / 6.4e-05
}
# The negative-truncation case (P.NEGATIVE) on the MI355X: solved -- Pm and Qm stayed positive definite, no status bit, nothing
# raised -- at these distances from the truth (the oracle: 7.7e-11 / 2.5e-10).
NEGATIVE_MEASURED = dict(flagged=[], status=0, scale=3.0e-14, pointwise=7.8e-14)


def ceiling(NQuad):
    return (1e-9, 1e-6) if NQuad <= 32 else (2e-9, 1e-6) if NQuad <= 64 else (2e-8, 1e-7)


def tolerance(key):
    assert key in MEASURED, f"no measured distance recorded for {key}"
    c = ceiling(int(key.split("_")[0]))
    return min(10 * MEASURED[key][0], c[0]), min(10 * MEASURED[key][1], c[1])


@pytest.fixture(scope="module")
def amd():
    import pydisort_amd
    from pydisort_amd import _engine
    assert _engine.device_count() >= 1, "no HIP device visible"
    return pydisort_amd


_ONE = {}


def one_column(amd, key):
    """The five quantities of the one-column solve at the case's points; solved once and shared with the batch test."""
    if key not in _ONE:
        kw = P.case(key)
        tau, phi = P.points(kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = amd.pydisort(**kw)
            fd = got[2](tau)
            _ONE[key] = dict(u=got[4](tau, phi), u0=got[3](tau), flux_up=got[1](tau), flux_down_diffuse=fd[0], flux_down_direct=fd[1])
    return _ONE[key]


def distances(fields, z):
    """(worst of the scale, worst pointwise) over the five quantities, each printed."""
    worst = [0.0, 0.0]
    for k in QUANTITIES:
        assert np.all(np.isfinite(fields[k])), k
        a, b = goldens.max_rel_err(fields[k], z[k])
        print(f"    {k}: {a:.3e} of the scale, {b:.3e} pointwise")
        worst = [max(worst[0], a), max(worst[1], b)]
    return worst


def held(label, key, fields):
    from conftest import record_parity
    z = np.load(P.fixture_path(key))
    tau, phi = P.points(P.case(key))
    assert np.array_equal(z["tau"], tau) and np.array_equal(z["phi"], phi)
    print(f"phase-truth {label}:")
    a, b = distances(fields, z)
    print(f"phase-truth {label}: worst {a:.3e} of the scale, {b:.3e} pointwise; oracle u {float(z['oracle_u_scale_rel']):.3e} / "
          f"{float(z['oracle_u_pointwise_rel']):.3e}")
    tol = tolerance(key)
    record_parity(f"phase/{label}", a, b, tol[0], tol[1], against="40-digit truth",
                  oracle_vs_truth_scale_rel=float(z["oracle_u_scale_rel"]), oracle_vs_truth_pointwise_rel=float(z["oracle_u_pointwise_rel"]))


@pytest.mark.parametrize("key", P.keys())
def test_one_column_against_truth(amd, key):
    held(key, key, one_column(amd, key))


def batch_columns(amd, NQuad):
    cfg, tau = P.batch_kwargs(NQuad)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, sol = amd.pydisort_batch(**cfg)
        fd = sol.flux_down(tau)
        out = dict(u=sol.u(tau, P.PHI), u0=sol.u0(tau), flux_up=sol.flux_up(tau), flux_down_diffuse=fd[0], flux_down_direct=fd[1])
    assert not np.any(sol.plan.column_status())
    sol.plan.close()
    return out


@pytest.mark.parametrize("NQuad", P.FULL)
def test_six_columns_in_one_batch_against_truth(amd, NQuad):
    """Columns of different structure side by side in a wavefront (64 lanes of rtd_eigen_lane_kernel, 8 or 16 chains of
    rtd_bc_small_kernel, 4 layers of rtd_eigen_kernel<16,2>, 2 problems of <32,2>), and the near-conservative columns on the thermal
    branch with a zero source."""
    got = batch_columns(amd, NQuad)
    failures = []
    for c, col in enumerate(P.COLUMNS):
        key = f"{NQuad}_{col}"
        fields = {k: got[k][c] for k in QUANTITIES}
        one = one_column(amd, key)
        for k in QUANTITIES:
            scale = np.max(np.abs(one[k]))
            d = float(np.max(np.abs(fields[k] - one[k])) / scale) if scale > 0 else float(np.max(np.abs(fields[k])))
            print(f"phase-truth batch {key} {k}: {d:.3e} of the scale from the one-column solve")
            if not d <= BATCH_VS_ONE_COLUMN:
                failures.append((key, k, "batch vs one column", d))
        try:
            held(f"batch {key}", key, fields)
        except AssertionError as e:  # every column is measured before the test fails
            failures.append((key, str(e)))
    assert not failures, failures


def test_negative_truncation_case(amd):
    """8 streams, Rayleigh / 0.8 0.8^l + 0.2 (-0.5)^l / isotropic: the 8-moment truncation of the middle layer dips to -0.25, so the
    input is outside what the library promises to solve -- but the reference's algorithm and the 40-digit solve agree on it to
    1e-10.  The device either meets the truth like every other case, or reports the column (column_status and LinAlgError); never
    unflagged numbers that miss the truth."""
    from conftest import record_parity
    kw = P.case(P.NEGATIVE)
    tau, phi = P.points(kw)
    z = np.load(P.fixture_path(P.NEGATIVE))
    assert P.truncation_minimum(kw).min() < -0.2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = amd.pydisort(**kw)
    plan = got[1].__self__.plan
    calls = dict(u=lambda: got[4](tau, phi), u0=lambda: got[3](tau), flux_up=lambda: got[1](tau),
                 flux_down_diffuse=lambda: got[2](tau)[0], flux_down_direct=lambda: got[2](tau)[1])
    flagged, worst = [], [0.0, 0.0]
    for k in QUANTITIES:
        try:
            v = calls[k]()
        except np.linalg.LinAlgError:
            flagged.append(k)
            continue
        a, b = goldens.max_rel_err(v, z[k])
        print(f"phase-truth {P.NEGATIVE} {k}: {a:.3e} of the scale, {b:.3e} pointwise")
        worst = [max(worst[0], a), max(worst[1], b)]
    status = int(plan.column_status()[0])
    print(f"phase-truth {P.NEGATIVE}: flagged {flagged}, column_status {status:#x}, worst of the returned {worst[0]:.3e} / {worst[1]:.3e}")
    assert bool(flagged) == (status != 0)
    assert NEGATIVE_MEASURED is not None, "no measured outcome recorded for the negative-truncation case"
    assert (flagged, status) == (NEGATIVE_MEASURED["flagged"], NEGATIVE_MEASURED["status"])
    # whatever was returned unflagged meets the truth
    tol = (min(10 * NEGATIVE_MEASURED["scale"], 1e-9), min(10 * NEGATIVE_MEASURED["pointwise"], 1e-6))
    record_parity(f"phase/{P.NEGATIVE}", worst[0], worst[1], tol[0], tol[1], against="40-digit truth",
                  oracle_vs_truth_scale_rel=float(z["oracle_u_scale_rel"]), oracle_vs_truth_pointwise_rel=float(z["oracle_u_pointwise_rel"]))
