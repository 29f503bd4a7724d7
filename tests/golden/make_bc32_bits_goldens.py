#!/usr/bin/env python3
"""Writes tests/golden/bc32_bits/<case>.npz: the bit-exact coefficients (through GC) and interface fields of the cases of
tests/bc32_bits_cases.py, as the library that RTD_LIB names (default: the one in the tree) computes them on an MI355X.  Run it with
the library of the commit whose boundary-condition kernel is the one to pin (the fixtures in the tree: the parent of the
scalar-base addressing), never to make a failing tests/test_gpu_bc32_bits.py pass.

Usage: RTD_LIB=/path/to/parent/librtd.so python tests/golden/make_bc32_bits_goldens.py [OUTPUT_DIR]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pythonic-disort_amd"), os.path.dirname(HERE)]

import bc32_bits_cases as B  # noqa: E402


def main(out_dir):
    import pydisort_amd as amd
    from pydisort_amd import _lib
    print("library:", _lib.LIB_PATH)
    os.makedirs(out_dir, exist_ok=True)
    for name, (_, _, _, force) in B.CASES.items():
        if force is None:
            os.environ.pop("RTD_BC_FORCE_PIVOT", None)
        else:
            os.environ["RTD_BC_FORCE_PIVOT"] = force
        got = B.compute(amd, name)
        rec = {}
        for k, a in got.items():
            assert np.all(np.isfinite(a)), (name, k)
            rec[k] = B.stored_part(a)
            rec[k + ".sha256"] = np.array(B.digest(a))
            rec[k + ".shape"] = np.array(a.shape)
        path = os.path.join(out_dir, name + ".npz")
        np.savez(path, **rec)
        print(f"{name}: {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 200_000, path


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "bc32_bits"))
