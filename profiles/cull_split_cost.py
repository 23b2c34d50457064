#!/usr/bin/env python3
"""Does the host side of the cull pre-pass cost what it did?  The c3 frame of bench.py (mask_filter_cost.py's context)
through a liblensflare_hip.so built from the parent commit and through this tree's, in ONE process, the legs alternated
`--rounds` times (and which of the two goes first in a round, too).  Every round gives each leg a new context: its first frame builds the cached tree (the `cull_cache_build`
slot, one event), then `--steps` frames are timed under a synchronize (frame time) and through the library's events (the
`cull_prepass` slot per frame).  Nothing the GPU executes differs between the two, so every figure of this tree must lie
within the parent's own spread over the rounds: within = |median - parent's median| <= parent's max - min.
Usage (repo root, one MI355X): python3 profiles/cull_split_cost.py --parent-lib PATH > profiles/cull_split_c3.json"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_filter_cost as m  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="liblensflare_hip.so built from the parent commit")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    args = ap.parse_args()
    pkgs = {"parent": m.package_on(args.parent_lib), "tree": m.g.load_package()}
    got = {leg: {"frame_ms": [], "cull_prepass_ms": [], "cull_cache_build_ms": []} for leg in pkgs}
    for r in range(args.rounds):
        for leg, pkg in (list(pkgs.items()) if r % 2 == 0 else list(pkgs.items())[::-1]):     # (who goes first alternates)
            lf, frame = m.context(pkg, None)
            lf.timing_enable(True)
            frame()
            lf.synchronize()
            n, ms = lf.timing_get("cull_cache_build")
            assert n == 1, (leg, n)
            got[leg]["cull_cache_build_ms"].append(ms)
            lf.timing_reset()
            for _ in range(args.steps):
                t0 = time.perf_counter()
                frame()
                lf.synchronize()
                got[leg]["frame_ms"].append((time.perf_counter() - t0) * 1e3)
            n, ms = lf.timing_get("cull_prepass")
            assert n == args.steps and lf.timing_get("cull_cache_build")[0] == 0, (leg, n)
            got[leg]["cull_prepass_ms"].append(ms / n)
            lf.close()
    out = {"what": "c3 frame (1920 x 1080, 256 spp, dgauss11.lens, pentagon mask, table rebuilt every frame), the parent commit's "
                   "library and this tree's alternated in one process, a new context per leg and round: wall-clock frame time, "
                   "the cull_prepass slot per frame (mean of a round), the cull_cache_build slot (one build per round)",
           "steps": args.steps, "rounds": args.rounds}
    for leg, d in got.items():
        out[leg] = {k: {"ms": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4),
                        "max": round(max(v), 4)} for k, v in d.items()}
    out["tree_minus_parent_median_ms"] = {k: round(out["tree"][k]["median"] - out["parent"][k]["median"], 4) for k in got["tree"]}
    out["within_parent_spread"] = {k: bool(abs(out["tree"][k]["median"] - out["parent"][k]["median"]) <=
                                           out["parent"][k]["max"] - out["parent"][k]["min"]) for k in got["tree"]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
