"""The band-integrated Planck function of csrc/rtd_planck.h, as the host compiles it, against 40-digit truth.

tests/cpu/planck_host.cpp (a stand-alone program over the header) is built with g++ and the address / undefined-behaviour
sanitizers (their runtimes linked in: the program needs no preload) and run directly; its results for the rows of
tests/golden/planck/rows.json are compared with the truth stored there (tools/planck_truth.py: the polylogarithm closed form in mpmath, independent of the routine's quadrature and of SciPy's).

Measured (this routine, g++ 64-bit libm): worst relative error 8.7e-16 over the rows with truth >= 1e-280 (the narrow band
2702.99 ... 2703.01 at 200 K and the x ~ 575 Wien-tail row; most rows 1e-17 ... 3e-16).  The reference's helper with
epsrel=1e-13 is 5e-17 ... 1.0e-14 from the same truth (1.3e-13 on the Wien-tail row).  Held at ten times the measured figure,
under the ceiling of 1e-12.
"""
import json
import os
import shutil
import subprocess
from decimal import Decimal, getcontext

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = json.load(open(os.path.join(ROOT, "tests", "golden", "planck", "rows.json")))["rows"]
MEASURED = 8.7e-16
TOL = min(10 * MEASURED, 1e-12)
getcontext().prec = 60


def rel_err(value, truth):
    """|value - truth| / truth, exactly (a double is a finite decimal), truth a decimal string."""
    t = Decimal(truth)
    return float(abs(Decimal(value) - t) / t)


@pytest.fixture(scope="module")
def host_values(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("planck") / "planck_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "cpu", "planck_host.cpp"), "-o", exe], check=True)
    text = "".join(f"{float(r['T']).hex()} {float(r['lo']).hex()} {float(r['hi']).hex()}\n" for r in ROWS)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(ROWS)
    return [float.fromhex(v) for v in out]


def test_fixture_covers_the_regimes():
    have = {(r["T"], r["lo"], r["hi"]) for r in ROWS}
    for need in [(200.0, 300.0, 800.0), (300.0, 300.0, 800.0), (200.0, 2702.99, 2703.01), (300.0, 2702.99, 2703.01),
                 (100.0, 0.0, 80000.0), (200.0, 0.0, 80000.0), (300.0, 0.0, 80000.0), (320.0, 0.0, 80000.0),
                 (550.0, 999.0, 1000.0), (700.0, 999.0, 1000.0), (6000.0, 1.0, 2.0), (150.0, 3000.0, 3001.0),
                 (100.0, 50000.0, 80000.0)]:
        assert need in have, need
    assert any(lo == 0.0 and hi == 50000.0 for _, lo, hi in have)
    assert any(T == 0.0 for T, _, _ in have) and any(lo == hi for _, lo, hi in have)


def test_host_routine_against_truth(host_values):
    worst = 0.0
    for r, v in zip(ROWS, host_values):
        if Decimal(r["truth"]) >= Decimal("1e-280"):
            e = rel_err(v, r["truth"])
            print(f"T={r['T']} band={r['lo']}..{r['hi']}: {v!r} rel err {e:.2e}")
            worst = max(worst, e)
    print(f"worst relative error {worst:.3e} (held at {TOL:.1e})")
    assert worst <= TOL


def test_degenerate_and_underflowing_rows(host_values):
    seen = 0
    for r, v in zip(ROWS, host_values):
        if r["T"] == 0.0 or r["lo"] == r["hi"]:
            assert v == 0.0 and Decimal(r["truth"]) == 0
            seen += 1
        elif Decimal(r["truth"]) < Decimal("1e-280"):
            assert v == v and 0.0 <= v <= 1e-270, v  # finite, not negative, small
            seen += 1
    assert seen >= 3


def test_truth_agrees_with_the_reference_helper():
    """Pins the closed form (constants, units, the factor 2e8 h c^2) to the reference's Planck integral."""
    n = 0
    for r in ROWS:
        if r["reference"] is not None:
            assert rel_err(float.fromhex(r["reference"]), r["truth"]) <= 1e-12, r
            n += 1
        else:
            assert Decimal(r["truth"]) < Decimal("1e-280")
    assert n >= 16
