#!/usr/bin/env python3
"""Per-kernel register / scratch / LDS table from hipcc's -Rpass-analysis=kernel-resource-usage remarks.

  tools/resource_usage.py [kernel.hip] [-I dir ...]     (default: every ICP unit of the Makefile's ICP_UNITS)

Compiles each file for gfx950 with the library's flags (nothing is written) and prints one line per
kernel: VGPRs, SGPRs, scratch bytes per lane, LDS bytes per block.  Used to check that a refactor
leaves a kernel's register allocation unchanged (diff two runs).
"""
import os
import re
import subprocess
import sys

from srchash import icp_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def usage(path, incs):
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
           "-fno-slp-vectorize", "-fPIC", "-I" + os.path.join(ROOT, "include")]
    cmd += ["-I" + d for d in incs] + ["-c", "-o", "/dev/null", path, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows, cur = [], None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass", line)
        if not m:
            continue
        txt = m.group(1)
        if txt.startswith("Function Name:"):
            cur = {"name": txt.split(":", 1)[1].strip()}
            rows.append(cur)
        elif cur is not None and ":" in txt:
            k, v = txt.split(":", 1)
            cur[k.strip()] = v.strip()
    return rows


def report(path, incs):
    rows = usage(path, incs)
    demangle = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True)
    names = demangle.stdout.splitlines() if demangle.returncode == 0 else [r["name"] for r in rows]
    for r, n in zip(rows, names):
        n = re.sub(r"\(.*\)$", "", n)
        print(f"{n:60s} VGPR {r.get('VGPRs', '?'):>4} SGPR {r.get('TotalSGPRs', '?'):>4} "
              f"scratch {r.get('ScratchSize [bytes/lane]', '?'):>4} LDS {r.get('LDS Size [bytes/block]', '?'):>6}")


def main():
    args = sys.argv[1:]
    if args and not args[0].startswith("-I"):
        paths = [args[0]]
    else:
        paths = [os.path.join(ROOT, "icp-4dradar_amd/csrc", u + ".hip") for u in icp_units()]
    for path in paths:
        report(path, [a[2:] for a in args if a.startswith("-I")] or [os.path.dirname(path)])


if __name__ == "__main__":
    main()
