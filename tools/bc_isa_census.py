#!/usr/bin/env python3
"""Static instruction census of one kernel in a gfx950 assembly file (hipcc -save-temps): vector instructions by class for the
whole kernel and for each loop (a backward branch and its target label), largest loops first.  Static counts: a loop's figure is
one trip through every block of its body, whichever path a wavefront takes.

Usage: python tools/bc_isa_census.py FILE.s [KERNEL_SUBSTRING]     (default kernel: rtd_bc_mfma_kernel)"""
import collections
import re
import sys

CLASSES = (
    ("mfma", re.compile(r"^v_mfma")),
    ("fp64", re.compile(r"^v_(add|mul|fma|fmac|max|min|rcp|rsq|sqrt|div_\w+|trig_preop|ldexp|frexp_\w+|fract|floor|ceil|rndne|trunc|cmp\w*|cvt)_\w*f64")),
    ("dpp_mov", re.compile(r"^v_mov_b32_dpp")),
    ("addr64", re.compile(r"^v_(lshl_add_u64|lshlrev_b64|ashrrev_i32|ashrrev_i64|add_co_u32|addc_co_u32|mad_[iu]64_[iu]32)")),
    ("select", re.compile(r"^v_cndmask")),
    ("mov", re.compile(r"^v_(mov_b32|mov_b64|accvgpr_\w+)")),
    ("int_other", re.compile(r"^v_(add|sub|and|or|xor|lshl|lshr|ashr|mul_lo|mul_hi|mad|bfe|perm|readlane|readfirstlane|writelane|mbcnt|min_[iu]|max_[iu]|cmp\w*_[iu])")),
)
MEM = (("global_load", re.compile(r"^global_load")), ("global_store", re.compile(r"^global_store")),
       ("global_saddr", re.compile(r"^global_(load|store)\S*\s.*\bs\[\d+:\d+\]")), ("scratch", re.compile(r"^scratch_")),
       ("lds", re.compile(r"^ds_")), ("s_nop", re.compile(r"^s_nop")), ("s_waitcnt", re.compile(r"^s_waitcnt")))


def kernel_lines(path, kernel):
    out, inside = [], False
    for line in open(path):
        if not inside:
            inside = bool(re.match(r"^\S*" + re.escape(kernel) + r"\S*:", line))
            continue
        text = line.split(";")[0].strip()
        if text:
            out.append(text)
        if text.startswith("s_endpgm"):
            break
    return out


def census(lines):
    c = collections.Counter()
    for t in lines:
        op = t.split()[0]
        if op.startswith("v_"):
            c["valu"] += 1
            if "dpp" in t and not op.startswith("v_mov_b32"):
                c["valu_with_dpp_source"] += 1
            for name, rx in CLASSES:
                if rx.match(op):
                    c[name] += 1
                    break
            else:
                c["valu_other"] += 1
        for name, rx in MEM:
            if rx.match(t):
                c[name] += 1
    return c


def loops(lines):
    labels = {t[:-1]: i for i, t in enumerate(lines) if re.match(r"^\.?\w+:$", t)}
    found = []
    for i, t in enumerate(lines):
        m = re.match(r"^s_c?branch\w*\s+(\.?\w+)$", t)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            found.append((labels[m.group(1)], i, m.group(1)))
    return found


def main():
    path = sys.argv[1]
    kernel = sys.argv[2] if len(sys.argv) > 2 else "rtd_bc_mfma_kernel"
    lines = kernel_lines(path, kernel)
    keys = ["valu"] + [n for n, _ in CLASSES] + ["valu_other", "valu_with_dpp_source"] + [n for n, _ in MEM]

    def show(title, c):
        print(f"{title}\n   " + "  ".join(f"{k} {c[k]}" for k in keys if c[k]))

    show(f"{kernel}: whole kernel, {len(lines)} lines", census(lines))
    for lo, hi, name in sorted(loops(lines), key=lambda r: r[0] - r[1])[:8]:
        show(f"loop {name}: lines {lo}..{hi}", census(lines[lo:hi + 1]))


if __name__ == "__main__":
    main()
