#!/usr/bin/env python3
"""What single-layer coatings cost: the c3 frame of bench.py (1920 x 1080, 256 spp, primary + 45 pairs x 3 wavelengths,
pentagon mask, cull table rebuilt every frame) on the bare double Gauss (dgauss11.lens) and on the same lens with a
quarter-wave MgF2 film on its eight glass-air interfaces (dgauss11_coated.lens), in ONE process: two contexts, the legs
alternated `--rounds` times, each leg `--warmup` frames and then `--steps` frames each timed under a synchronize (the
bench's frame: find_sun_pos, the sun hand-over, lf_trace_ghosts, the flare layer).  Prints one JSON record with the spread
of each leg and the ratio of the medians.
Usage (repo root, one MI355X): python3 profiles/coating_cost.py [--steps 3 --warmup 1 --rounds 4] > profiles/coating_cost.json"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

SUN_NS = (0.521445, 0.517156)      # bench.py
W, H, SPP = 1920, 1080, 256


def context(pkg, lens_file):
    lens = pkg.load_lens_file(lens_file)
    mask = pkg.load_aperture_png("pentbig500_14.png")
    efl = pkg.paraxial_efl(lens)
    lf = pkg.LensFlare(0)
    lf.set_frame(W, H)
    lf.set_params(1, 25.0, 1.0)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_aperture(pkg.APERTURE_GHOST, mask)
    lf.set_lens(lens)                      # (applies the file's coatings, if it has any)
    lf.set_ghost_pairs(None, True)
    lf.set_jitter_counter(0x1e45f1a4e)
    lf.set_march_culling(2)
    hf = 2 * math.degrees(math.atan(0.5 * lens["sensor_width_mm"] / efl))
    vf = 2 * math.degrees(math.atan(math.tan(math.radians(hf) / 2) * H / W))
    lf.set_camera([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [0, 0, 0], hf, vf)
    ex, ey = math.tan(math.radians(hf) / 2), math.tan(math.radians(vf) / 2)
    lights = [[(2 * SUN_NS[0] - 1) * ex * 10, (2 * SUN_NS[1] - 1) * ey * 10, -10.0, 1.0, 0.9, 0.5]]
    lf.set_band(0, H)

    def frame():
        lf.find_sun_pos(lights)
        lf.set_sun_from_flares(0, efl, 0.05)
        lf.trace_ghosts(SPP, 0x1e45f1a4e)
        lf.render_flare_layer()
    return lf, frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    pkg = g.load_package()
    legs = {"uncoated": context(pkg, "dgauss11.lens"), "coated": context(pkg, "dgauss11_coated.lens")}
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, (lf, frame) in legs.items():
            for _ in range(args.warmup):
                frame()
            lf.synchronize()
            for _ in range(args.steps):
                t0 = time.perf_counter()
                frame()
                lf.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {"what": "c3 frame, bare dgauss11.lens against dgauss11_coated.lens (8 quarter-wave MgF2 films), one process, "
                   "legs alternated", "W": W, "H": H, "spp": SPP, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds}
    for name, v in ms.items():
        out[name] = {"ms": [round(x, 3) for x in v], "median_ms": round(statistics.median(v), 3),
                     "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                     "stdev_ms": round(statistics.stdev(v), 3) if len(v) > 1 else 0.0}
    out["coated_over_uncoated_median"] = round(out["coated"]["median_ms"] / out["uncoated"]["median_ms"], 4)
    lf_c = legs["coated"][0]
    lf_c.reset_counters()
    legs["coated"][1]()
    out["coated_march_stats"] = lf_c.march_stats()
    print(json.dumps(out))
    for lf, _ in legs.values():
        lf.close()


if __name__ == "__main__":
    main()
