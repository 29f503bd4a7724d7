#!/usr/bin/env python3
"""40-digit truth for the band-integrated Planck function (csrc/rtd_planck.h, include/rtd.h: rtd_planck_band).

    E(T, lo, hi) = 2e8 h c^2 (T / c2)^4 [F(xlo) - F(xhi)],   c2 = 100 h c / k,   x = c2 nu / T,
    F(x) = Int_x^inf t^3 / (e^t - 1) dt = 6 Li4(e^-x) + 6 x Li3(e^-x) + 3 x^2 Li2(e^-x) - x^3 ln(1 - e^-x)

from the polylogarithm closed form in mpmath, with the exact SI values of h, c, k.  It shares nothing with the routine under test
(Gauss-Legendre panels in float64) nor with the reference's SciPy quadrature.  The working precision is 40 digits PLUS the
digits the difference F(xlo) - F(xhi) cancels on a narrow band, so that the result has 40.

    python tools/planck_truth.py T LO HI            one value
    python tools/planck_truth.py --write-fixture    tests/golden/planck/rows.json; with the reference package importable
                                                    (PYTHONPATH) the rows also carry blackbody_contrib_to_BCs(..., epsrel=1e-13)
"""
import json
import os
import sys

import mpmath as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "planck", "rows.json")
DIGITS = 40
H, C, K = "6.62607015e-34", "299792458", "1.380649e-23"  # exact by definition of the SI (scipy.constants.h, .c, .k)

# (T, lo, hi): the reference's own test bands at their temperatures (pydisotest/7_test.py, 9_test.py), then the regimes in which a
# float64 evaluation can lose digits
ROWS = [
    (200.0, 300.0, 800.0), (300.0, 300.0, 800.0),
    (200.0, 2702.99, 2703.01), (300.0, 2702.99, 2703.01),
    (100.0, 0.0, 80000.0), (200.0, 0.0, 80000.0), (300.0, 0.0, 80000.0), (320.0, 0.0, 80000.0),
    (550.0, 999.0, 1000.0), (600.0, 999.0, 1000.0), (650.0, 999.0, 1000.0), (700.0, 999.0, 1000.0),
    (200.0, 0.0, 50000.0), (300.0, 0.0, 50000.0),
    (6000.0, 1.0, 2.0),            # Rayleigh-Jeans: x ~ 2.4e-4 ... 4.8e-4
    (150.0, 3000.0, 3001.0),       # Wien: x ~ 28.8
    (0.0, 300.0, 800.0),           # T = 0
    (250.0, 1234.5, 1234.5),       # lo = hi
    (100.0, 50000.0, 80000.0),     # the result underflows: 1.6e-307
    (100.0, 40000.0, 41000.0),     # deep Wien tail, x ~ 575, result ~ 1e-240: still a normal number
    (250.0, 10.0, 12000.0),        # a wide band from inside the Rayleigh-Jeans end across the peak into the tail
    (1.0, 0.0, 5.0),               # a cold body: everything within 7 units of x, T^4 = 1
]


def planck_band(T, lo, hi, digits=DIGITS):
    """E(T, lo, hi) in W / m^2 as an mpf with `digits` significant digits; T, lo, hi are taken as the doubles they are."""
    T, lo, hi = mp.mpf(T), mp.mpf(lo), mp.mpf(hi)
    if T == 0 or lo == hi:
        return mp.mpf(0)
    extra = 0 if lo == 0 else int(mp.ceil(mp.log10(max(lo, hi) / abs(hi - lo)))) + 2
    with mp.workdps(digits + 10 + extra):
        h, c, k = mp.mpf(H), mp.mpf(C), mp.mpf(K)
        c2 = 100 * h * c / k

        def F(x):
            if x == 0:
                return mp.pi ** 4 / 15
            e = mp.exp(-x)
            return 6 * mp.polylog(4, e) + 6 * x * mp.polylog(3, e) + 3 * x ** 2 * mp.polylog(2, e) - x ** 3 * mp.log1p(-e)

        return +(2e8 * h * c ** 2 * (T / c2) ** 4 * (F(c2 * lo / T) - F(c2 * hi / T)))


def planck_band_float(T, lo, hi):
    """The truth rounded to the nearest double."""
    return float(planck_band(T, lo, hi))


def _reference_values():
    try:
        from PythonicDISORT.subroutines import blackbody_contrib_to_BCs
    except ImportError:
        return None
    return [float(blackbody_contrib_to_BCs(T, lo, hi, epsrel=1e-13)) for T, lo, hi in ROWS]


def write_fixture():
    ref = _reference_values()
    if ref is None:
        sys.exit("the reference package (PythonicDISORT) is not importable: put its src/ on PYTHONPATH")
    rows = []
    for (T, lo, hi), r in zip(ROWS, ref):
        t = planck_band(T, lo, hi)
        rows.append(dict(T=T, lo=lo, hi=hi, truth=mp.nstr(t, DIGITS, min_fixed=0, max_fixed=0),
                         reference=float(r).hex() if t >= mp.mpf("1e-280") else None))
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        json.dump(dict(units="T [K], lo / hi [cm^-1], truth [W m^-2] to 40 digits (tools/planck_truth.py), reference = "
                             "blackbody_contrib_to_BCs(T, lo, hi, epsrel=1e-13) of the reference as a hex double",
                       rows=rows), f, indent=1)
        f.write("\n")
    print(FIXTURE, len(rows), "rows")


if __name__ == "__main__":
    if sys.argv[1:] == ["--write-fixture"]:
        write_fixture()
    elif len(sys.argv) == 4:
        print(mp.nstr(planck_band(*[float(a) for a in sys.argv[1:]]), DIGITS))
    else:
        sys.exit(__doc__)
