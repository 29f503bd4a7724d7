"""csrc/rtd_lambert.h on the host: the two routines rtd_lambert_kappa_kernel and rtd_lambert_couple_kernel run, compiled into the
stand-alone program tests/cpu/lambert_arith_main.cpp with g++ -fsanitize=address,undefined and run directly -- no Python under a
sanitizer, nothing preloaded.

Every kappa and every coupled element is held to the exact fractions.Fraction value of the float64 inputs within the bounds the
header DERIVES from its operations as written (each one correctly rounded operation: a division by the float64 pi, three fma, a
division; then one fma per element): 6 u (A |F| / pi + (1 - A) E) / (1 - A s) for kappa and 8 u (|a| + |kappa b|) for an element,
u = 2^-53 (tests/lambert_cases.py: kappa_ratio, couple_ratio).  Nothing is measured into a bound.  The same inputs go through the
NumPy / Fraction model of lambert_cases, which must agree bit for bit: the model is what tests/test_lambert_cpu.py applies.

Cases: A = 0 (kappa = E exactly; with E = 0 the element is a itself, a negative zero included), A = 1 (the emission drops out
exactly), s up to 0.999 with A = 1 (1 - A s = 0.001), E = 0, E = 1e6 F, an albedo of 1e-300, random values between; 1 - A s <= 0 and non-finite factors
raise the flag.

Seen with g++ on x86-64: kappa worst 0.41 of its bound, elements worst 0.32 of theirs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lambert_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("lambert_arith") / "lambert_arith")
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-static-libubsan", os.path.join(ROOT, "tests", "cpu", "lambert_arith_main.cpp"), "-o", out], check=True)
    return out


def run(exe, rows, tmp_path):
    path = tmp_path / "in.txt"
    path.write_text("".join(" ".join(float(v).hex() for v in row) + "\n" for row in rows))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(path)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    out = [line.split() for line in r.stdout.strip().splitlines()]
    assert len(out) == len(rows)
    return [(float.fromhex(k), int(bad), float.fromhex(o)) for k, bad, o in out]


def _rows():
    """(A, F, s, E, a, b): the named edge cases, then random ones."""
    rng = np.random.default_rng(20261)
    rows = []
    for A in (0.0, 1.0, 0.3, 0.95, np.nextafter(1.0, 0.0), 1e-300):
        for s in (0.0, 1e-9, 0.1397, 0.869, 0.999):
            for F, E in ((1.349, 0.0), (1.349, 1.7), (1e-3, 1e3), (0.0, 1.7), (2.5, 0.0), (0.0, 0.0)):
                rows.append((A, F, s, E, rng.normal(), rng.normal()))
    for _ in range(300):
        rows.append((rng.uniform(), 10.0 ** rng.uniform(-6, 3), rng.uniform(0, 0.999), rng.choice([0.0, 10.0 ** rng.uniform(-6, 3)]),
                     rng.normal() * 10.0 ** rng.uniform(-8, 2), rng.normal() * 10.0 ** rng.uniform(-8, 2)))
    rows.append((0.0, 1.0, 0.5, 0.0, -0.0, 3.0))  # kappa = 0: a itself, the sign of a zero included
    rows.append((0.7, 1.0, 0.5, 0.0, 1.0, -0.0))
    return rows


def test_kappa_and_coupled_elements_against_exact_values(exe, tmp_path):
    rows = _rows()
    out = run(exe, rows, tmp_path)
    worst_k = worst_c = 0.0
    for (A, F, s, E, a, b), (kappa, bad, got) in zip(rows, out):
        assert bad == 0
        assert (kappa, got) == (LC.kappa_model(A, F, s, E)[0], float(LC.couple_model(a, b, kappa)))  # the model, bit for bit
        rk = LC.kappa_ratio(kappa, A, F, s, E)
        rc = LC.couple_ratio(got, a, b, A, F, s, E)
        assert rk <= 1.0 and rc <= 1.0, (A, F, s, E, a, b, rk, rc)
        worst_k, worst_c = max(worst_k, rk), max(worst_c, rc)
        if A == 0.0:
            assert kappa == E  # exactly: g does not enter, (1 - 0) E = E
            if E == 0.0:
                assert got == a and np.signbit(got) == np.signbit(a)
        if A == 1.0:
            assert kappa == LC.kappa_model(1.0, F, s, 0.0)[0]  # the emission drops out exactly
    assert any(s == 0.999 and A == 1.0 for A, _, s, *_ in rows) and any(E >= 1e5 * F > 0 for _, F, _, E, *_ in rows)
    print(f"LAMBERT arith: kappa worst {worst_k:.2f} of its bound, elements worst {worst_c:.2f} of theirs")


def test_the_flag_is_raised_where_the_formula_has_no_meaning(exe, tmp_path):
    rows = [(1.0, 1.0, 1.0, 0.0, 1.0, 1.0),             # 1 - A s = 0
            (1.0, 1.0, 1.25, 0.0, 1.0, 1.0),            # 1 - A s < 0
            (0.5, float("inf"), 0.5, 0.0, 1.0, 1.0),    # a non-finite numerator
            (0.5, float("nan"), 0.5, 0.0, 1.0, 1.0),
            (0.5, 1.0, float("nan"), 0.0, 1.0, 1.0),    # a non-finite denominator
            (0.5, 1.0, 0.5, 0.0, 1.0, 1.0)]             # (and a sound one)
    out = run(exe, rows, tmp_path)
    assert [bad for _, bad, _ in out] == [1, 1, 1, 1, 1, 0]
    assert [LC.kappa_model(*row[:4])[1] for row in rows] == [1, 1, 1, 1, 1, 0]
