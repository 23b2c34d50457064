#!/usr/bin/env python3
"""Static counts of the culled march's vector instructions and lane moves (profiles/march_moves_resources.txt).

  hipcc <the Makefile's FLAGS> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
        lens-flare_amd/csrc/lf_cull.hip -o lf_cull.s 2> remarks.txt
  python3 profiles/march_moves_count.py lf_cull.s remarks.txt [--loops 'k_march_cull<3, false, 1, 0>']

Prints, for every k_march_cull / k_march_items instantiation, the compiler's resource line (VGPRs, SGPRs, VGPRs
spilled, SGPRs spilled, scratch bytes/lane, LDS bytes/block, waves/SIMD) and the number of lane moves in its text
(v_readlane_b32 + v_writelane_b32: how the compiler reloads and saves a spilled SGPR, one vector issue slot each).
With --rows it lists, for every instantiation, the loops that load a 16-dword record (the row loops): those with the weight
record's loads beside it (a second 16-dword load in the parent, single dwords in this tree) are the re-march row.
With --loops it lists the natural loops of one kernel (a label and a later branch back to it), innermost marked by
nesting depth, each with its vector instructions, lane moves, v_mov, square roots and scalar loads: the regions of
the table are read off that list (the loop with the weighted event's divisions-free Fresnel fraction and one root pair
is the re-march row; the loop with K root pairs and no lane move in front of the 16-dword load is the first march).
"""
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    res = out.stdout.split("\n")
    short = []
    for r in res[: len(names)]:
        r = r.replace("(anonymous namespace)::", "")
        r = re.sub(r"^void ", "", r)
        short.append(r.split("(")[0])
    return short


def functions(asm):
    """name -> list of lines of the function's text"""
    fn, cur, out = None, [], {}
    for ln in asm:
        m = re.match(r"^(_Z\w+):", ln)
        if m and fn is None:
            fn, cur = m.group(1), []
            continue
        if fn is not None:
            if ln.startswith(".Lfunc_end"):
                out[fn] = cur
                fn = None
            else:
                cur.append(ln)
    return out


def is_instr(ln):
    s = ln.strip()
    return bool(s) and not s.startswith((".", ";", "//")) and not s.endswith(":")


def opcode(ln):
    return ln.strip().split()[0]


def tally(lines):
    t = dict(vector=0, lane=0, vmov=0, sqrt=0, smem=0, salu=0)
    for ln in lines:
        if not is_instr(ln):
            continue
        op = opcode(ln)
        if op.startswith("v_"):
            t["vector"] += 1
            if op.startswith(("v_readlane", "v_writelane")):
                t["lane"] += 1
            if op.startswith("v_mov_b32") or op.startswith("v_accvgpr"):
                t["vmov"] += 1
            if op.startswith("v_sqrt"):
                t["sqrt"] += 1
        elif op.startswith(("s_load", "s_buffer_load")):
            t["smem"] += 1
        elif op.startswith("s_"):
            t["salu"] += 1
    return t


def loops(lines):
    labels = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            labels[m.group(1)] = i
    found = {}
    for i, ln in enumerate(lines):
        if not is_instr(ln):
            continue
        op = opcode(ln)
        if op.startswith(("s_cbranch", "s_branch")):
            tgt = ln.strip().split()[-1]
            if tgt in labels and labels[tgt] < i:
                found[tgt] = max(found.get(tgt, 0), i)
    res = sorted((labels[t], e, t) for t, e in found.items())
    return res


def resources(remarks):
    """mangled name -> 'VGPRs SGPRs vspill sspill scratch lds occ'"""
    out, name, cur = {}, None, {}
    keys = ["VGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
            "Occupancy [waves/SIMD]"]
    for ln in remarks:
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            name, cur = m.group(1), {}
            out[name] = cur
            continue
        m = re.search(r"remark:\s+(.*?): (\d+)", ln)
        if m and name:
            cur[m.group(1).strip()] = m.group(2)
    return {n: " ".join(c.get(k, "?") for k in keys) for n, c in out.items()}


def main():
    asm = open(sys.argv[1]).read().split("\n")
    res = resources(open(sys.argv[2]).read().split("\n"))
    fns = functions(asm)
    names = [n for n in fns if "k_march_cull" in n or "k_march_items" in n]
    short = dict(zip(names, demangle(names)))
    print("# kernel: VGPRs SGPRs VGPRs-spilled SGPRs-spilled scratch-B/lane LDS-B/block waves/SIMD | lane moves in the text")
    for n in sorted(names, key=lambda n: short[n]):
        print("%-36s %s | %d" % (short[n], res.get(n, "?"), tally(fns[n])["lane"]))
    if "--rows" in sys.argv:
        print("# row loops (the innermost loop around a 16-dword record load): vector, lane moves, roots, 16-dword loads, 1-dword loads")
        for n in sorted(names, key=lambda n: short[n]):
            lines = fns[n]
            ls = loops(lines)
            def ops(a, b):
                return [opcode(ln) for ln in lines[a:b + 1] if is_instr(ln)]
            for a, b, t in ls:
                body = ops(a, b)
                x16, x1 = body.count("s_load_dwordx16"), body.count("s_load_dword")
                if x16 == 0:
                    continue
                # the innermost loop around the record load (a film kernel's row holds a small loop of its own)
                if any(a2 >= a and b2 <= b and (a2, b2) != (a, b) and "s_load_dwordx16" in ops(a2, b2) for a2, b2, _ in ls):
                    continue
                tt = tally(lines[a:b + 1])
                kind = "re-march row" if (x16 >= 2 or x1 >= 4) else "first march"
                print("%-32s %-13s v=%d lane=%d sqrt=%d x16=%d x1=%d" % (short[n], kind, tt["vector"], tt["lane"], tt["sqrt"], x16, x1))
    if "--loops" in sys.argv:
        want = sys.argv[sys.argv.index("--loops") + 1]
        n = [n for n in names if short[n] == want][0]
        lines = fns[n]
        ls = loops(lines)
        print("# loops of %s: first line..last line (of the kernel's text), depth: vector, lane moves, v_mov, roots, scalar loads, scalar ALU" % want)
        print("# (a loop's counts include the loops nested inside it; 'own' = without them)")
        for a, b, t in ls:
            depth = sum(1 for a2, b2, _ in ls if a2 <= a and b2 >= b) - 1
            inner = [(a2, b2) for a2, b2, _ in ls if a2 >= a and b2 <= b and (a2, b2) != (a, b)]
            own = [ln for i, ln in enumerate(lines[a:b + 1], a) if not any(a2 <= i <= b2 for a2, b2 in inner)]
            tt, to = tally(lines[a:b + 1]), tally(own)
            print("%s%6d..%6d d%d: all v=%d lane=%d mov=%d sqrt=%d smem=%d salu=%d | own v=%d lane=%d mov=%d sqrt=%d smem=%d salu=%d" % (
                "  " * depth, a, b, depth, tt["vector"], tt["lane"], tt["vmov"], tt["sqrt"], tt["smem"], tt["salu"],
                to["vector"], to["lane"], to["vmov"], to["sqrt"], to["smem"], to["salu"]))
        tt = tally(lines)
        print("whole kernel: v=%d lane=%d mov=%d sqrt=%d smem=%d salu=%d" % (tt["vector"], tt["lane"], tt["vmov"], tt["sqrt"], tt["smem"], tt["salu"]))


if __name__ == "__main__":
    main()
