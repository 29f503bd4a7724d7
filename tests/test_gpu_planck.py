"""pydisort_amd.planck_band (include/rtd.h: rtd_planck_band) on the device against the 40-digit truth of
tests/golden/planck/rows.json, and a call whose length is no multiple of any block size.

The device runs the routine the host test measures (csrc/rtd_planck.h; tests/test_planck_truth_cpu.py: 8.7e-16) with the device's
exp and expm1; it is held at ten times the CPU figure under the same ceiling of 1e-12.  Measured on the MI355X: 8.6e-16 at
worst over the rows, 8.5e-16 over the 100 003-element call.
"""
import json
import os
from decimal import Decimal, getcontext

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = json.load(open(os.path.join(ROOT, "tests", "golden", "planck", "rows.json")))["rows"]
CPU_MEASURED = 8.7e-16
TOL = min(10 * CPU_MEASURED, 1e-12)
getcontext().prec = 60
T, LO, HI = (np.array([r[k] for r in ROWS]) for k in ("T", "lo", "hi"))
HELD = np.array([Decimal(r["truth"]) >= Decimal("1e-280") for r in ROWS])


def rel_errs(values):
    out = np.zeros(len(ROWS))
    for i, (r, v) in enumerate(zip(ROWS, values)):
        t = Decimal(r["truth"])
        if HELD[i]:
            out[i] = float(abs(Decimal(float(v)) - t) / t)
    return out


@pytest.fixture(scope="module")
def device_rows():
    import pydisort_amd
    return pydisort_amd.planck_band(T, LO, HI)


def test_fixture_rows_against_truth(device_rows):
    errs = rel_errs(device_rows)
    for r, v, e in zip(ROWS, device_rows, errs):
        print(f"T={r['T']} band={r['lo']}..{r['hi']}: {v!r} rel err {e:.2e}")
    print(f"worst relative error {errs.max():.3e} (held at {TOL:.1e})")
    assert errs.max() <= TOL
    for r, v in zip(ROWS, device_rows):
        if r["T"] == 0.0 or r["lo"] == r["hi"]:
            assert v == 0.0
        elif Decimal(r["truth"]) < Decimal("1e-280"):
            assert np.isfinite(v) and 0.0 <= v <= 1e-270


def test_odd_length_call_matches_the_rows_tiled(device_rows):
    """100 003 elements = 390 blocks of 256 and a tail of 163: every element must be the integral of ITS (T, band)."""
    import pydisort_amd
    n = 100003
    idx = np.arange(n) % len(ROWS)
    got = pydisort_amd.planck_band(T[idx], LO[idx], HI[idx])
    assert got.shape == (n,)
    want = np.array([float(Decimal(r["truth"])) for r in ROWS])[idx]
    held = HELD[idx]
    err = np.max(np.abs(got[held] - want[held]) / want[held])
    print(f"worst relative error over {n} elements {err:.3e}")
    assert err <= TOL + 2.3e-16  # (the truth itself rounded to double)
    assert np.array_equal(got, np.asarray(device_rows)[idx])  # the same thread-independent routine: the same bits


def test_broadcasting_and_shapes():
    import pydisort_amd
    temps = np.array([[200.0, 250.0, 300.0], [0.0, 320.0, 100.0]])
    got = pydisort_amd.planck_band(temps, 300.0, np.array([800.0, 900.0, 1000.0]))
    assert got.shape == (2, 3) and got[1, 0] == 0.0
    one = pydisort_amd.planck_band(300.0, 300.0, 800.0)
    assert np.ndim(one) == 0 and one == pydisort_amd.planck_band(np.array([300.0]), 300.0, 800.0)[0]
    assert got[0, 2] > got[0, 0] > 0.0
    assert pydisort_amd.planck_band(np.zeros(0), 1.0, 2.0).shape == (0,)
