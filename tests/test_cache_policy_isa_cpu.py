"""The cache policy of the 32-stream hand-off is in the built code object.  The policy is a bit of the memory instruction (``nt``)
that the compiler takes from ``__builtin_nontemporal_load`` / ``_store``, and the optimiser can drop it without a word -- it did so
in a first form of this change, where a plain and a streamed copy of the same stores sat in the two arms of a branch and were merged
into plain ones.  So the gfx950 ISA of the shipped librtd.so is disassembled and counted:

* ``rtd_bc_mfma_kernel``: the backward sweep's operand loads -- ``load_set``, 16 loads (A, Y, H: 4 each; s, rho_b, k, E), inlined
  four times (the set taken at the turn, the one before the loop, two in the loop unrolled by two) -- are the kernel's 64 ``nt``
  loads; no other load and no store of it is streamed (the forward sweep's accesses are what those loads find in the cache);
* ``rtd_eigen_kernel<16,2>`` and ``<16,3>``: the 36 hand-off stores (Y 16, k, E, B 2, A 16) are ``nt``;
* the eigen instances of the other stream counts stream nothing (the 64-stream one reads its own stores back).

No GPU is needed: hipcc cross-compiles and llvm-objdump reads the offload bundle.
"""
import collections
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pythonic-disort_amd", "pydisort_amd", "librtd.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def accesses():
    """mangled kernel name -> Counter of (mnemonic family, streamed?) over its global loads and stores."""
    objdump = os.path.join(LLVM, "llvm-objdump")
    assert os.path.exists(objdump), objdump
    assert os.path.exists(LIB), LIB
    out = {}
    tmp = tempfile.mkdtemp(prefix="rtd_isa_")
    try:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(LIB, local)
        subprocess.run([objdump, "--offloading", local], capture_output=True, text=True, cwd=tmp, check=True)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            path = os.path.join(tmp, f)
            with open(path, "rb") as fh:  # (the symbol table is in the file: only the two code objects concerned are disassembled)
                blob = fh.read()
            if b"rtd_bc_mfma_kernel" not in blob and b"rtd_eigen_kernel" not in blob:
                continue
            name = None
            for line in subprocess.run([objdump, "-d", path], capture_output=True, text=True, check=True).stdout.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    name = m.group(1)
                    continue
                m = re.match(r"^\s+global_(load|store)_\w+\s([^/]*)", line)
                if m and name:
                    out.setdefault(name, collections.Counter())[(m.group(1), bool(re.search(r"\bnt\b", m.group(2))))] += 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def _one(accesses, pattern):
    names = [n for n in accesses if re.search(pattern, n) and not n.endswith(".kd")]
    assert len(names) == 1, (pattern, names)
    return accesses[names[0]]


def test_bc32_backward_operand_loads_are_streamed_and_nothing_else(accesses):
    c = _one(accesses, r"rtd_bc_mfma_kernel")
    assert c[("load", True)] == 64, c
    assert c[("load", False)] > 0 and c[("store", False)] > 0, c
    assert c[("store", True)] == 0, c


@pytest.mark.parametrize("jv", [2, 3])
def test_eigen16_handoff_stores_are_streamed(accesses, jv):
    c = _one(accesses, rf"rtd_eigen_kernelILi16ELi{jv}E")
    assert c[("store", True)] == 36, c
    assert c[("load", True)] == 0, c


@pytest.mark.parametrize("np_", [8, 32, 64])
def test_other_eigen_instances_stream_nothing(accesses, np_):
    c = _one(accesses, rf"rtd_eigen_kernelILi{np_}ELi2E")
    assert c[("store", True)] == 0 and c[("load", True)] == 0, c
    assert c[("store", False)] > 0, c
