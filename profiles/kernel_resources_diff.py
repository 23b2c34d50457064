#!/usr/bin/env python3
"""Pair every kernel of two builds by its mangled name and print their resources side by side.

    make -C lens-flare_amd EXTRA=-Rpass-analysis=kernel-resource-usage 2> remarks.txt      (a fresh build, on each tree)
    python profiles/kernel_resources_diff.py parent_remarks.txt remarks.txt > profiles/<feature>_resources.txt

Columns: VGPRs, SGPRs, VGPRs spilled, SGPRs spilled, scratch B/lane, LDS B/block, waves/SIMD.  No GPU needed."""
import re
import subprocess
import sys

FIELDS = ["VGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]"]


def parse(path):
    kernels, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = kernels.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[key] = int(val)
    return kernels


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"\(anonymous namespace\)::", "", d)
        d = re.sub(r"^void ", "", d)
        short[n] = re.sub(r"\(.*$", "", d)
    return short


def row(k):
    return " ".join(f"{k.get(f, -1):5d}" for f in FIELDS)


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    names = demangle(sorted(set(a) | set(b)))
    print("# columns: VGPRs, SGPRs, VGPRs spilled, SGPRs spilled, scratch B/lane, LDS B/block, waves/SIMD")
    print("# ---- kernels of the parent commit: parent | this tree")
    differ = 0
    for n in sorted(a, key=lambda n: names[n]):
        if n in b:
            same = a[n] == b[n]
            differ += not same
            print(f"{names[n]:64s} {row(a[n])} | {row(b[n])}  {'same' if same else 'DIFFERS'}")
        else:
            differ += 1
            print(f"{names[n]:64s} {row(a[n])} | (gone)")
    print(f"# {len(a)} kernels of the parent, {differ} differ or are gone")
    print("# ---- kernels new in this tree")
    for n in sorted(set(b) - set(a), key=lambda n: names[n]):
        print(f"{names[n]:64s} {row(b[n])}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
