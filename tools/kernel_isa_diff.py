#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 assembly of two builds: the proof that a source clean-up left the machine code alone.

Reads every *amdgcn*.s of the two directories (hipcc --cuda-device-only -S, or the -save-temps outputs: same file names on both
sides), cuts out each kernel -- from its label to its end label, which takes in the .amdhsa_kernel descriptor -- drops comments
and blank lines, renumbers the compiler's local labels, and prints `identical` or `differs` (with the first hunk of a unified
diff) per kernel, then the kernels found on one side only.  Exit status 1 on any difference.  Text only: it knows no instruction.

Usage: python tools/kernel_isa_diff.py DIR_A DIR_B"""
import difflib
import glob
import os
import re
import sys


def kernels(directory):
    """{file name:kernel name: normalised lines} (the extraction of bc_isa_census.kernel_lines, for every kernel of every file)"""
    found = {}
    for path in sorted(glob.glob(os.path.join(directory, "*amdgcn*.s"))):
        text = open(path).read()
        for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
            m = re.search(r"^" + re.escape(name) + r":.*?^\.Lfunc_end\d+:", text, re.M | re.S)
            lines = [ln.split(";")[0].strip() for ln in m.group(0).split("\n")]
            # .LBB<function>_<block>, .Lfunc_end<function>: the function number is the kernel's place in its file
            found[os.path.basename(path) + ":" + name] = [re.sub(r"\.L(BB|func_end|func_begin)\d+", r".L\1", ln) for ln in lines if ln]
    return found


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for key in sorted(set(a) & set(b)):
        if a[key] == b[key]:
            print(f"identical  {key}  ({len(a[key])} lines)")
            continue
        bad += 1
        print(f"differs    {key}")
        diff = difflib.unified_diff(a[key], b[key], sys.argv[1], sys.argv[2], lineterm="")
        hunks = 0
        for ln in diff:
            hunks += ln.startswith("@@")
            if hunks > 1:
                break
            print("    " + ln)
    for side, only in ((sys.argv[1], set(a) - set(b)), (sys.argv[2], set(b) - set(a))):
        for key in sorted(only):
            bad += 1
            print(f"only in {side}: {key}")
    print(f"{len(set(a) & set(b))} kernels on both sides, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
