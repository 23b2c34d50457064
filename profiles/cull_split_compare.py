#!/usr/bin/env python3
"""Is the device code of two sets of hipcc assembly listings the same, kernel by kernel?
    python3 profiles/cull_split_compare.py parent.s -- lf_cull.s lf_cull_prepass.s
Per kernel: the text from its label to its .Lfunc_end and its .amdhsa_kernel descriptor block (VGPRs, SGPRs, spills,
scratch, LDS), `;` comments stripped, the per-function ordinal taken out of local labels (.LBB49_27 -> .LBB_27: it
counts the functions of the file).  Required: the same kernel names on both sides, each kernel in exactly one file of
a side, the text equal.  Prints one line per kernel and the totals; exit status 1 on any difference."""
import re
import sys


def kernels(path):
    """{name: [normalised lines of its body + its descriptor block]}"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    out = {}
    for name in names:
        a = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d = next(i for i, l in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"$", l))
        e = next(i for i in range(d, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        text = []
        sets = [l.strip() for l in lines if l.strip().startswith(".set " + name + ".")]     # the resource symbols the descriptor refers to
        for l in lines[a:b + 1] + lines[d:e + 1] + sets:
            l = re.sub(r"(\.L(?:BB|func_end|func_begin|tmp))\d+", r"\1", l.split(";")[0]).rstrip()
            if l:
                text.append(l)
        out[name] = text
    return out


def side(paths):
    seen = {}
    for p in paths:
        for name, text in kernels(p).items():
            if name in seen:
                sys.exit(f"{name} is in {seen[name][0]} and in {p}")
            seen[name] = (p, text)
    return seen


def main():
    cut = sys.argv.index("--")
    old, new = side(sys.argv[1:cut]), side(sys.argv[cut + 1:])
    bad = sorted(set(old) ^ set(new))
    n_lines = n_diff = 0
    for name in sorted(set(old) & set(new)):
        a, b = old[name][1], new[name][1]
        d = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
        n_lines += len(a)
        n_diff += d
        res = " ".join(re.split(r"\.|amdhsa_", l)[-1].replace(",", "") for l in b if re.search(r"\.(num_vgpr|numbered_sgpr|private_seg_size), |amdhsa_group_segment_fixed_size", l))
        print(f"{name} | {new[name][0].split('/')[-1]} | lines {len(a)} differing {d} | {res}")
    print(f"kernels {len(old)} -> {len(new)}, only on one side: {bad or 'none'}; lines compared {n_lines}, differing {n_diff}")
    sys.exit(1 if bad or n_diff else 0)


if __name__ == "__main__":
    main()
