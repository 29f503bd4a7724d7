"""The surface models of csrc/rtd_surface.h, as the host compiles them, against 50-digit truth.

tests/cpu/surface_rho_main.cpp (a stand-alone program over the header) is built with g++ and the address / undefined-behaviour
sanitizers (their runtimes linked in: the program needs no preload) and run directly.  Its samples for every pair of cosines of
tests/golden/surface/*.npz (tools/surface_truth.py: the formulas of include/rtd.h in mpmath, from the float64 inputs) are held to

    |rho - truth| <= 16 x np_dist_all[0] x scale,

np_dist_all[0] the worst distance of a plain NumPy float64 evaluation from the same truth over all files (2.8e-15 of the row's max
|rho| as generated; the value is read from the fixture and printed) and scale the max |rho| of the row (one pair of cosines over the
azimuths), taken before Ross-Li's clamp so that a row the clamp cuts to zero keeps a tolerance; the clamp is 1-Lipschitz, so the
bound carries over.  16: the host's libm and FMA contraction differ from NumPy's by a few ulp per call.  What the bound must catch
is far larger: the arccos form of the phase angle is 8e-8 off at the hot spot, a wrong azimuth convention O(1).

Reciprocity rho(a, b, dphi) = rho(b, a, dphi) is held to the same bound (both orders are within it of one truth, so to twice it of
each other), and Ross-Li is held non-negative and finite on a grid that reaches grazing cosines of 1e-3."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "surface", "*.npz")))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("surface") / "surface_rho")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "cpu", "surface_rho_main.cpp"), "-o", exe], check=True)

    def run(rows):
        """rows of (model, par[4], mu, mup, nphi) -> list of arrays [nphi] (None where the program answered "bad")"""
        text = "".join(f"{int(m)} {' '.join(float(v).hex() for v in par)} {float(a).hex()} {float(b).hex()} {int(n)}\n" for m, par, a, b, n in rows)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(rows)
        return [None if ln == "bad" else np.array([float.fromhex(v) for v in ln.split()]) for ln in lines]

    return run


def test_fixtures_cover_the_cases():
    names = {os.path.basename(f) for f in FILES}
    assert names == {f"{m}{k}_n{n}.npz" for m in ("hapke", "rossli", "rpv") for k in (0, 1) for n in (6, 16, 34)}
    cut = 0
    for f in FILES:
        d = np.load(f)
        N = len(d["mu"])
        assert d["rho"].shape == (N, N + 3, int(d["nphi"])) and d["scale"].shape == (N, N + 3)
        assert 0.5 in d["mup"] and 1.0 in d["mup"] and np.sum(d["mup"] == d["mu"][N // 2]) >= 2  # (17 nodes: the middle one is 0.5 itself)
        assert np.all(d["rho"] >= 0) or int(d["model"]) != 2
        if int(d["model"]) == 2:
            cut += int(d["rows_cut"])
    assert cut > 0  # some Ross-Li rows are cut to zero by the clamp
    assert {int(np.load(f)["nphi"]) for f in FILES} == {16, 64, 40}


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_header_routine_against_truth_and_reciprocity(program, path):
    d = np.load(path)
    mu, mup, nphi, model, par = d["mu"], d["mup"], int(d["nphi"]), int(d["model"]), d["params"]
    tol = 16.0 * float(d["np_dist_all"][0])
    assert 1e-16 < tol < 1e-12  # a fixture that lost its distance would otherwise pass anything
    rows = [(model, par, a, b, nphi) for a in mu for b in mup] + [(model, par, b, a, nphi) for a in mu for b in mup]
    got = np.array(program(rows)).reshape(2, len(mu), len(mup), nphi)
    err = np.abs(got[0] - d["rho"]) / d["scale"][:, :, None]
    rec = np.abs(got[1] - d["rho"]) / d["scale"][:, :, None]  # the swapped call against the same truth
    print(f"{os.path.basename(path)}: tolerance {tol:.3e} of the row's max |rho|; worst {err.max():.3e}, swapped {rec.max():.3e}")
    assert err.max() <= tol
    assert rec.max() <= tol
    if model == 2:
        assert np.all(got >= 0.0)


def test_rossli_is_never_negative_and_bad_parameters_are_named(program):
    mus = [1e-3, 0.0199, 0.1, 0.5, 0.97, 1.0]
    rows = [(2, par + (0.0,), a, b, 32) for par in ((0.3, 0.1, 0.05), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (0.02, 0.3, 0.2))
            for a in mus for b in mus]
    out = np.array(program(rows))
    assert np.all(np.isfinite(out)) and np.all(out >= 0.0)
    assert np.any(out == 0.0) and np.any(out > 0.0)
    bad = [(0, (1.5, 0, 0, 0)), (0, (-0.1, 0, 0, 0)), (1, (-1.0, 0.06, 0.6, 0)), (1, (1.0, 0.0, 0.6, 0)), (1, (1.0, 0.06, 0.0, 0)),
           (1, (1.0, 0.06, 1.5, 0)), (2, (-0.1, 0.1, 0.1, 0)), (2, (0.1, 0.1, -0.1, 0)), (3, (-0.1, 0.8, 0.0, 0.1)), (3, (0.1, 0.0, 0.0, 0.1)),
           (3, (0.1, 0.8, 1.0, 0.1)), (3, (0.1, 0.8, -1.0, 0.1)), (2, (float("nan"), 0.1, 0.1, 0)), (3, (0.1, 0.8, 0.0, float("inf"))),
           (4, (0.1, 0.1, 0.1, 0.1)), (-1, (0.1, 0.1, 0.1, 0.1))]
    assert program([(m, par, 0.5, 0.5, 4) for m, par in bad]) == [None] * len(bad)
    good = [(0, (0.0, 0, 0, 0)), (0, (1.0, 0, 0, 0)), (1, (0.0, 0.06, 1.0, 0)), (2, (0.0, 0.0, 0.0, 0)), (3, (0.0, 0.8, -0.99, -3.0))]
    assert all(v is not None for v in program([(m, par, 0.5, 0.5, 4) for m, par in good]))


def test_exact_azimuths_and_the_hot_spot(program):
    """dphi = 0, pi/2, pi, 3 pi/2 carry exact cosines; at the hot spot (mu = mu', dphi = pi) Hapke's surge is B0 exactly:
    rho = W / (8 mu) ((1 + B0) 3/2 + H^2 - 1) -- the arccos form loses 8e-8 there."""
    mu, B0, HH, W = 0.3, 1.0, 0.06, 0.6
    r = program([(1, (B0, HH, W, 0.0), mu, mu, 4)])[0]
    H = (1 + 2 * mu) / (1 + 2 * mu * np.sqrt(1 - W))
    want = W / 4 / (2 * mu) * ((1 + B0) * 1.5 + H * H - 1)
    assert abs(r[2] - want) <= 8 * np.finfo(float).eps * want
    assert r[1] == r[3]  # even in dphi
    lam = program([(0, (0.25, 0, 0, 0), 0.1, 0.9, 5)])[0]
    assert np.all(lam == 0.25)
