#!/usr/bin/env python3
"""kernel_asm_diff.py OLD_DIR NEW_DIR — per kernel symbol, is the machine code the same in two builds?

Each directory holds `hipcc --save-temps=obj` output (`make asm` writes build/).  Every device
assembly file (*-hip-amdgcn-*.s) is read; for each kernel symbol (one with an `.amdhsa_kernel` block) two
texts are compared between the directories:
  text  the function, from `.type <sym>,@function` to its `.Lfunc_end`, with `;` comments stripped and
        `.LBB<n>_` labels rewritten to `.LBB_` (the function number follows the kernel's position in
        its module)
  desc  the `.amdhsa_kernel <sym>` ... `.end_amdhsa_kernel` block (registers, scratch, LDS)
One line per symbol: `same` / `DIFF` / `missing` for each.  Exit status 1 unless every symbol is the same
in both.
"""
import glob
import os
import re
import sys


def kernels(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*-hip-amdgcn-*.s"))):
        lines = open(path).read().split("\n")
        text, cur = {}, None
        for ln in lines:
            m = re.match(r"\s*\.type\s+(\S+),@function", ln)
            if m:
                cur = m.group(1)
                text[cur] = []
            if cur is not None:
                ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0]).rstrip()
                if ln.startswith(".Lfunc_end"):
                    cur = None
                elif ln:
                    text[cur].append(ln)
        for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", "\n".join(lines), re.S):
            out[m.group(1)] = (text.get(m.group(1)), m.group(2))
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    word = lambda a, b, k: "missing" if a is None or b is None else "same" if a[k] == b[k] else "DIFF"
    bad = 0
    for sym in sorted(set(old) | set(new)):
        t, d = (word(old.get(sym), new.get(sym), k) for k in (0, 1))
        bad += (t, d) != ("same", "same")
        print(f"text {t:7s} desc {d:7s} {sym}")
    print(f"{len(set(old) | set(new))} kernels, {bad} not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
