"""The 18 ... 32-stream boundary-condition kernel's outputs, bit for bit: tiny batches (tests/bc32_bits_cases.py) solved on the
device and compared with ``np.array_equal`` -- no tolerance -- against tests/golden/bc32_bits/, which
tests/golden/make_bc32_bits_goldens.py wrote on an MI355X from the commit BEFORE rtd_bc_mfma_kernel's loads and stores went to a
wave-uniform base plus a 32-bit lane offset.  That rewrite changes how addresses are formed and nothing else: no floating-point
operation may change its operands, its contraction or its place, so the coefficients of every layer (through GC) and u, u0 and the
three fluxes at the interfaces stay the same bits, with and without the fused interface evaluation, on the speculative
elimination and on both forced pivoted paths.  Run with ``-m gpu`` on an MI355X.
"""
import os

import numpy as np
import pytest

import bc32_bits_cases as B

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bc32_bits")


@pytest.fixture(scope="module")
def amd():
    import pydisort_amd
    from pydisort_amd import _engine
    assert _engine.device_count() >= 1, "no HIP device visible"
    return pydisort_amd


def test_every_case_has_a_fixture_under_the_size_limit():
    for name in B.CASES:
        path = os.path.join(GOLDEN, name + ".npz")
        assert os.path.exists(path), path
        assert os.path.getsize(path) < 200_000, (path, os.path.getsize(path))


@pytest.mark.parametrize("name", list(B.CASES))
def test_bc32_outputs_are_bit_identical(amd, monkeypatch, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    force = B.CASES[name][3]
    if force is not None:
        monkeypatch.setenv("RTD_BC_FORCE_PIVOT", force)
    else:
        monkeypatch.delenv("RTD_BC_FORCE_PIVOT", raising=False)
    got = B.compute(amd, name)
    names = [k for k in z.files if not k.endswith((".sha256", ".shape"))]
    assert sorted(names) == sorted(got), (sorted(names), sorted(got))
    differing = []
    for k in names:
        a = got[k]
        assert tuple(z[k + ".shape"]) == a.shape, (name, k, a.shape)
        if not np.array_equal(B.stored_part(a), z[k]):
            diff = np.abs(B.stored_part(a) - z[k])
            differing.append((k, "stored part", int(np.count_nonzero(diff)), float(np.nanmax(diff))))
        elif B.digest(a) != str(z[k + ".sha256"]):
            differing.append((k, "sha256 of the whole array"))
    assert not differing, (name, differing)
