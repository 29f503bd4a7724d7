"""csrc/rtd_nt_prep.h on the host: the routines rtd_api.hip's preparation kernels of the corrections run (the IMS constants of a column lane by lane,
the weighted full moments, a band's mixed moments), compiled into the stand-alone program tests/cpu/nt_prep_host_main.cpp with
g++ -fsanitize=address,undefined and run directly -- no Python under a sanitizer, nothing preloaded.

Cases: L = 1, 3 and 7 layers x 12 moments with NLeg = 8; high moments of both signs; one column whose f is 0 in every layer (no IMS
term: coef 0, amplitude 0, scaled mu0 = mu0, exactly); a mix of S = 1, 2, 3 species with a layer that has no scatterer.  Every output
is held to the exact fractions.Fraction value of the float64 inputs within the bounds DERIVED in tests/nt_prep_cases.py from the
loops as written: gamma_{2L+4} sum|resid w| / sum f w for r_k, that propagated through (2k + 1)(2 r - r^2), gamma_{2L+6} / (1 - omega f)
for the scaled mu0 and twice that for the amplitude, gamma_{2S+3} sum|t leg| / sca for a mixed moment; the weighted moments bit for
bit.  Nothing is measured into a bound.

Seen with g++ on x86-64 (no contraction): IMS worst 0.130 of the bound (L = 1), 0.130 (L = 3), 0.088 (L = 7); mix worst 0.349
(S = 1), 0.287 (S = 2), 0.374 (S = 3)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nt_prep_cases as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLEG, NALL = NP.NLEG, NP.NALL


def hexes(a):
    return " ".join(float(v).hex() for v in np.asarray(a, float).ravel())


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("nt_prep") / "nt_prep_host")
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-static-libubsan", os.path.join(ROOT, "tests", "cpu", "nt_prep_host_main.cpp"), "-o", out], check=True)
    return out


def run(exe, text, tmp_path):
    path = tmp_path / "in.txt"
    path.write_text(text)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(path)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return [[float.fromhex(v) for v in line.split()] for line in r.stdout.strip().splitlines()]


@pytest.mark.parametrize("L", [1, 3, 7])
def test_ims_constants_and_weighted_moments_against_exact_values(exe, tmp_path, L):
    c = NP.columns(L, 0)
    C = len(c["mu0"])
    text = f"ims {C} {L} {NLEG} {NALL}\n"
    for i in range(C):
        text += " ".join(hexes(c[k][i]) for k in ("tau", "omega", "f", "leg")) + f" {hexes(c['mu0'][i])} {hexes(c['I0'][i])}\n"
    out = run(exe, text, tmp_path)
    assert len(out) == C and all(len(row) == L * NALL + NALL + 2 for row in out)
    worst = 0.0
    for i, row in enumerate(out):
        wfull, coef, par = np.array(row[:L * NALL]).reshape(L, NALL), row[L * NALL:L * NALL + NALL], row[-2:]
        NP.hold_wfull(wfull, c["leg"][i])
        worst = max(worst, NP.hold_ims(coef, par, c["tau"][i], c["omega"][i], c["f"][i], c["leg"][i], NLEG, c["mu0"][i], c["I0"][i]))
    assert out[-1][L * NALL:] == [0.0] * NALL + [float(c["mu0"][-1]), 0.0]  # the column without truncation: exact
    assert np.any(c["leg"][:, :, NLEG:] < 0) and np.any(c["leg"][:, :, NLEG:] > 0)
    print(f"NT-PREP host L {L}: worst {worst:.3f} of the derived bound")


@pytest.mark.parametrize("S", [1, 2, 3])
def test_mixed_moments_against_exact_values(exe, tmp_path, S):
    rng = np.random.default_rng([78, S])
    R, L = 3, 3
    ds, om = rng.uniform(0.01, 0.6, (R, L, S)), rng.uniform(0.0, 1.0, (R, L, S))
    om[1, 1, :] = 0.0  # nothing scatters
    ds[1, 1, 0] = 0.0
    ls = rng.uniform(0.3, 0.9, (S, 1)) ** np.arange(NALL)[None, :] * np.where(np.arange(NALL) % 3 == 2, -1.0, 1.0)[None, :]
    ls[:, 0] = 1.0
    out = run(exe, f"mix {R} {L} {S} {NALL}\n{hexes(ds)}\n{hexes(om)}\n{hexes(ls)}\n", tmp_path)
    assert len(out) == R * L and all(len(row) == NALL for row in out)
    worst = 0.0
    for rl, row in enumerate(out):
        r, l = divmod(rl, L)
        for k in range(NALL):
            want, bound = NP.exact_mix(ds[r, l], om[r, l], ls, k)
            err = abs(NP.F(row[k]) - want)
            assert err <= bound, (r, l, k, row[k], float(want))
            if bound > 0:
                worst = max(worst, float(err / bound))
    assert out[1 * L + 1] == [1.0] + [0.0] * (NALL - 1)
    print(f"NT-PREP host mix S {S}: worst {worst:.3f} of the derived bound")
