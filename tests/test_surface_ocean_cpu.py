"""The ocean surface model (RTD_SURFACE_OCEAN) on the host, against 50-digit truth, under the address / undefined-behaviour sanitizers.

1. tests/cpu/surface_ocean_main.cpp (a stand-alone program over csrc/rtd_surface.h, sanitizer runtimes linked in: no preload) gives
   rho by the header's routine for every row of tests/golden/surface_ocean/rho_U<U>_n<streams>.npz (tools/surface_ocean_truth.py):
   the pairs of double-Gauss nodes of 6 / 16 / 34 / 64 streams, mu = 1, mu' = 1, the azimuths 0, pi/2, pi, the glint's own scale and
   random ones, U = 0, 1, 5, 15 m/s.  The truth is rho in 50 digits from the float64 inputs (par, mu, mu', c, s) and the bound is that
   of tests/test_surface_cpu.py:

       |rho - truth| <= 16 x np_dist_all[0] x scale,

   np_dist_all[0] the worst distance of a plain NumPy float64 evaluation from the same truth over all files (5.5e-14 of the row's max
   |rho| as generated: the glint's exponent tan^2 b / sigma^2 reaches hundreds and carries its relative rounding into rho; read from
   the fixture and printed), scale the row's max |rho|.  No NaN anywhere; reciprocity to the same bound; the hemispherical albedo
   Sum_j 2 mu_j w_j q^0(mu_i, mu_j) of the glint alone <= 1 at every node (the fixtures hold it: worst 0.74 -- shadowing is always on).
   The header's rtd_ocean_cluster_b must be the b of the truth's rule, bit for bit.

2. tests/cpu/surface_ocean_host_main.cpp runs rtd_surface_ocean_kernel thread by thread over the stand-in HIP runtime (see there):
   tables against the 50-digit modes of the same rule within the derived bound, every refusal, windows."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "surface_ocean")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "rho_U*.npz")))
OCEAN = 4


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("surface_ocean") / "surface_ocean")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "cpu", "surface_ocean_main.cpp"), "-o", exe], check=True)

    def run(rows):
        """rows of (model, par[4], mu, mup, c, s) -> list of (rho, b) (None where the program answered "bad")"""
        text = "".join(f"{int(m)} {' '.join(float(v).hex() for v in par)} {float(a).hex()} {float(b).hex()} {float(c).hex()} {float(s).hex()}\n"
                       for m, par, a, b, c, s in rows)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(rows)
        return [None if ln == "bad" else tuple(float.fromhex(v) for v in ln.split()) for ln in lines]

    return run


def test_fixtures_cover_the_cases():
    assert {os.path.basename(f) for f in FILES} == {f"rho_U{u}_n{n}.npz" for u in (0, 1, 5, 15) for n in (6, 16, 34, 64)}
    for f in FILES:
        d = np.load(f)
        N = len(d["mu"]) - 1
        assert d["mu"][-1] == 1.0 and 1.0 in d["mup"] and d["rho"].shape == (N + 1, N + 3, 10) == d["c"].shape
        assert np.all(d["c"][..., :3] == [1.0, 0.0, -1.0]) and np.all(d["s"][..., :3] == [0.0, 1.0, 0.0])
        assert np.all(np.isfinite(d["rho"])) and np.all(d["rho"] >= d["params"][2] * (1 - 1e-15))


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_header_routine_against_truth_and_reciprocity(program, path):
    d = np.load(path)
    mu, mup, par, c, s = d["mu"], d["mup"], d["params"], d["c"], d["s"]
    tol = 16.0 * float(d["np_dist_all"][0])
    assert 1e-16 < tol < 2e-12  # a fixture that lost its distance would otherwise pass anything
    idx = [(i, j, k) for i in range(len(mu)) for j in range(len(mup)) for k in range(c.shape[2])]
    out = program([(OCEAN, par, mu[i], mup[j], c[i, j, k], s[i, j, k]) for i, j, k in idx] +
                  [(OCEAN, par, mup[j], mu[i], c[i, j, k], s[i, j, k]) for i, j, k in idx])
    got = np.array([v[0] for v in out]).reshape((2,) + c.shape)
    assert np.all(np.isfinite(got))  # no NaN anywhere: mu = 1, mu' = 1, exponentials that underflow
    err = np.abs(got[0] - d["rho"]) / d["scale"][:, :, None]
    rec = np.abs(got[1] - d["rho"]) / d["scale"][:, :, None]  # the swapped call against the same truth
    print(f"{os.path.basename(path)}: tolerance {tol:.3e} of the row's max |rho|; worst {err.max():.3e}, swapped {rec.max():.3e}")
    assert err.max() <= tol
    assert rec.max() <= tol
    assert np.all(got >= par[2])  # the glint adds to rho_w, never subtracts
    # the header's b is the b of the truth's rule, bit for bit
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import surface_ocean_truth as truth
    finally:
        sys.path.pop(0)
    b = np.array([v[1] for v in out[:len(idx)]]).reshape(c.shape)[..., 0]
    assert np.array_equal(b, truth.cluster_b(par[0], mu[:, None], mup[None, :]))
    assert np.all(b[mu == 1.0] == 1.0) and np.all(b[:, mup == 1.0] == 1.0) and np.all((b >= 2.0 ** -20) & (b <= 1.0))
    # albedo of the glint alone at every node (the rule at 4096 nodes): a surface reflects no more than it receives
    print(f"  albedo: worst {d['albedo'].max():.4f}")
    assert np.all(d["albedo"] <= 1.0) and np.all(d["albedo"] > 0.0)


def test_edges_and_bad_parameters(program):
    """mu = 1 and mu' = 1 (v infinite: L = 0, not NaN), the sun overhead seen from overhead at U = 0 (the specular point itself),
    underflow of the glint to rho_w exactly, and the parameter ranges."""
    par = (0.0, 1.34, 0.03, 0.0)
    rows = [(OCEAN, par, 1.0, 1.0, 1.0, 0.0), (OCEAN, par, 1.0, 0.3, 0.0, 1.0), (OCEAN, par, 0.3, 1.0, -1.0, 0.0), (OCEAN, par, 0.02, 0.02, -1.0, 0.0)]
    out = np.array([v[0] for v in program(rows)])
    assert np.all(np.isfinite(out))
    F0 = ((1.34 - 1) / (1.34 + 1)) ** 2  # normal incidence on a level facet: F / (4 sigma^2) + rho_w, no shadowing at mu = 1
    assert abs(out[0] - (F0 / (4 * 0.003) + 0.03)) <= 1e-14 * out[0]
    assert out[3] == 0.03  # backscatter at grazing angles: the exponential underflows, and 0 is the right answer
    bad = [(-1.0, 1.34, 0, 0), (float("nan"), 1.34, 0, 0), (float("inf"), 1.34, 0, 0), (5.0, 1.0, 0, 0), (5.0, 0.5, 0, 0), (5.0, 1.34, -0.1, 0),
           (5.0, 1.34, 0.0, float("nan"))]
    assert program([(OCEAN, p, 0.5, 0.5, 1.0, 0.0) for p in bad]) == [None] * len(bad)
    assert program([(5, (5.0, 1.34, 0, 0), 0.5, 0.5, 1.0, 0.0)]) == [None]
    good = [(0.0, 1.0000001, 0.0, 0), (30.0, 1.5, 1.0, 0)]
    assert all(v is not None for v in program([(OCEAN, p, 0.5, 0.5, 1.0, 0.0) for p in good]))


def test_mode_kernel_over_the_stand_in_runtime(tmp_path):
    d = np.load(os.path.join(GOLDEN, "modes_n6.npz"))
    N, C, NB, nphi = len(d["mu"]), len(d["mu0"]), d["q"].shape[1], int(d["nphi"])
    x, w = np.polynomial.legendre.leggauss(N)
    wq = (w[np.argsort(x)] / 2)
    assert np.array_equal(np.sort((x + 1) / 2), d["mu"]) and C == 6 and NB == 2 * N
    case = tmp_path / "case.txt"
    with open(case, "w") as f:
        f.write(f"{N} {NB} {nphi} {C} {float(d['np_dist_modes'][0]).hex()}\n")
        for a in (d["mu"], wq, d["mu0"], d["params"], d["q"], d["q0"]):
            f.write(" ".join(float(v).hex() for v in np.ravel(a)) + "\n")
    exe = host_program.build(tmp_path, "surface_ocean_host_main.cpp", "surface_ocean_host")
    r = host_program.run(exe, str(case))
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SURFACE OCEAN HOST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_front_end_takes_the_model_and_refuses_what_the_host_refuses():
    from pydisort_amd import _surface
    sf = _surface.surface_request(dict(model="ocean", params=(5.0, 1.34, 0.02)), ((), (3,)), "", 16, None)
    assert sf["model"] == OCEAN and sf["nphi"] == 512 and sf["NBDRF"] == 16 and sf["params"].tolist() == [[5.0, 1.34, 0.02, 0.0]]
    assert _surface.surface_request(dict(model="Ocean", params=np.tile((5.0, 1.34, 0.0), (3, 1)), nphi=64), ((), (3,)), "", 16, None)["nphi"] == 64
    assert _surface.surface_request(dict(model="hapke", params=(1.0, 0.06, 0.6)), ((), (3,)), "", 16, None)["nphi"] == 256  # (unchanged)
    for bad in ((-1.0, 1.34, 0.0), (np.nan, 1.34, 0.0), (np.inf, 1.34, 0.0), (5.0, 1.0, 0.0), (5.0, 1.34, -0.1)):
        with pytest.raises(ValueError, match="U >= 0, n > 1, rho_w >= 0"):
            _surface.surface_request(dict(model="ocean", params=bad), ((), (3,)), "", 16, None)
    for nphi in (511, 62, 33, 16386):
        with pytest.raises(ValueError, match="nphi"):
            _surface.surface_request(dict(model="ocean", params=(5.0, 1.34, 0.0), nphi=nphi), ((), (3,)), "", 16, None)
    with pytest.raises(ValueError, match="n > 1"):
        _surface.surface_reflectance("ocean", (5.0, 0.9, 0.0), 0.5, 0.5, 8)
