#!/usr/bin/env python3
"""Writes tests/golden/eigen_bits/<case>.npz: the bit-exact eigen-stage tensors and evaluated fields of the cases of
tests/eigen_bits_cases.py, as the library in the tree computes them on an MI355X.  Run it from a commit whose eigen stage is the
one to pin (the fixtures in the tree: the commit before the select-free reductions and Cholesky steps), never to make a failing
tests/test_gpu_eigen_stage_bits.py pass.  (q66_L2_wide and q32_L5_beam_thermal_mfma: the commit before the fused eigen kernel was
cut into stage functions.)

Usage: python tests/golden/make_eigen_bits_goldens.py [OUTPUT_DIR [CASE ...]]   (no CASE: every case)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pythonic-disort_amd"), os.path.dirname(HERE)]

import eigen_bits_cases as E  # noqa: E402


def resonant_mu0(amd, name):
    """mu0 with 1/mu0 = k + RESONANCE_OFFSET for the mode-0 eigenvalue k of column 1's only layer nearest to 2 (mu0 ~ 0.5)."""
    cfg = E.inputs(name)
    _, sol = amd.pydisort_batch(**cfg)
    K = np.abs(sol.plan.tensors(1)["K"][0, 0])
    sol.plan.close()
    k = K[np.argmin(np.abs(K - 2.0))]
    assert k > 1.05
    return 1.0 / (k + E.RESONANCE_OFFSET)


def main(out_dir, only=()):
    import pydisort_amd as amd
    os.makedirs(out_dir, exist_ok=True)
    for name, (_, _, _, kind) in E.CASES.items():
        if only and name not in only:
            continue
        extra = {}
        if kind == "resonant":
            extra["resonant_mu0"] = np.float64(resonant_mu0(amd, name))
        cfg = E.inputs(name, **{k: float(v) for k, v in extra.items()})
        got = E.compute_in_child(name) if name in E.CHILD_ENV else E.compute(amd, cfg)
        if kind == "resonant":  # the column is what its name says
            K = np.abs(got["c1.K"][0, 0])
            assert np.min(np.abs(K - 1.0 / cfg["mu0"][1])) < 1e-3
        rec = dict(extra)
        for k, a in got.items():
            assert np.all(np.isfinite(a)), (name, k)
            rec[k] = E.stored_part(a)
            rec[k + ".sha256"] = np.array(E.digest(a))
            rec[k + ".shape"] = np.array(a.shape)
        path = os.path.join(out_dir, name + ".npz")
        np.savez(path, **rec)
        print(f"{name}: {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 200_000, path


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "eigen_bits"), sys.argv[2:])
