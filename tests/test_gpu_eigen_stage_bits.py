"""The eigen stage's outputs, bit for bit: tiny batches (tests/eigen_bits_cases.py) solved on the device and compared with
``np.array_equal`` -- no tolerance -- against tests/golden/eigen_bits/, which tests/golden/make_eigen_bits_goldens.py wrote on an
MI355X from the commit BEFORE the 16-stream-group eigen kernel lost its lane selects (bank-masked DPP merges in levels 8 and 4 of
the transposed reductions and in the pair-layout exchange, EXEC-masked multiplier and diagonal in the Cholesky steps).  Those
rewrites move data and mask lanes differently; they must not change the order of a floating-point operation, a Newton-step count
or a rounding, so every tensor the stage exports (G from Y, A and k; K; B; the thermal vector; GC behind the boundary-condition
solve) and u, u0 and the fluxes evaluated from it stay the same bits.  Run with ``-m gpu`` on an MI355X.

Cases: 32 streams x 4 Fourier modes at 1, 5 and 20 layers, beam only / beam + thermal polynomial / no beam / 1/mu0 5e-4 above an
eigenvalue; 18 and 30 streams (padding streams); one 16-stream and one 64-stream case that pin the instances next to the changed one;
66 streams (the one-problem-per-wavefront instance) and the 32-stream beam + thermal case under RTD_EIG_MFMA=1 (the matrix-core
assembly, solved in a fresh child process), whose fixtures come from the commit before the fused kernel was cut into stage functions.
"""
import os

import numpy as np
import pytest

import eigen_bits_cases as E

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eigen_bits")


@pytest.fixture(scope="module")
def amd():
    import pydisort_amd
    from pydisort_amd import _engine
    assert _engine.device_count() >= 1, "no HIP device visible"
    return pydisort_amd


def test_every_case_has_a_fixture_under_the_size_limit():
    for name in E.CASES:
        path = os.path.join(GOLDEN, name + ".npz")
        assert os.path.exists(path), path
        assert os.path.getsize(path) < 200_000, (path, os.path.getsize(path))


@pytest.mark.parametrize("name", list(E.CASES))
def test_eigen_stage_outputs_are_bit_identical(amd, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    kind = E.CASES[name][3]
    cfg = E.inputs(name, resonant_mu0=float(z["resonant_mu0"]) if kind == "resonant" else None)
    got = E.compute_in_child(name) if name in E.CHILD_ENV else E.compute(amd, cfg)
    if kind == "resonant":  # the case is what its name says: 1/mu0 within 1e-3 of an eigenvalue of column 1
        assert np.min(np.abs(np.abs(got["c1.K"][0, 0]) - 1.0 / cfg["mu0"][1])) < 1e-3
    names = [k for k in z.files if not k.endswith((".sha256", ".shape")) and k != "resonant_mu0"]
    assert sorted(names) == sorted(got), (sorted(names), sorted(got))
    differing = []
    for k in names:
        a = got[k]
        assert tuple(z[k + ".shape"]) == a.shape, (name, k, a.shape)
        if not np.array_equal(E.stored_part(a), z[k]):
            diff = np.abs(E.stored_part(a) - z[k])
            differing.append((k, "stored part", int(np.count_nonzero(diff)), float(np.nanmax(diff))))
        elif E.digest(a) != str(z[k + ".sha256"]):
            differing.append((k, "sha256 of the whole array"))
    assert not differing, (name, differing)
