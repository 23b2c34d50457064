#!/usr/bin/env python3
"""What the bilinear stop mask costs: the c3 frame of bench.py (1920 x 1080, 256 spp, primary + 45 pairs x 3 wavelengths,
pentagon mask, cull table rebuilt every frame) under LF_MASK_NEAREST and under LF_MASK_BILINEAR (lf_set_mask_filter), in
ONE process: one context per leg, the legs alternated `--rounds` times, each leg `--warmup` frames and then `--steps`
frames each timed under a synchronize (the bench's frame: find_sun_pos, the sun hand-over, lf_trace_ghosts, the flare
layer).  `--parent-lib` adds a third leg: the same frame (nearest) through a liblensflare_hip.so built from the parent
commit, loaded beside this tree's -- nothing a default frame launches has changed, so the two nearest legs may differ
by run-to-run noise only: within_noise = this tree's median <= the parent's + 3 x the larger standard deviation.
Prints one JSON record with the spread of each leg and the ratios of the medians.
Usage (repo root, one MI355X): python3 profiles/mask_filter_cost.py [--parent-lib PATH] > profiles/mask_filter_cost.json"""
import argparse
import importlib.util
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


def package_on(lib_path):
    """a second instance of the package's Python, bound to another build of the library"""
    spec = importlib.util.spec_from_file_location("lens_flare_amd_parent", os.path.join(g.PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[g.PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["lens_flare_amd_parent"] = mod
    spec.loader.exec_module(mod)
    mod.LIB_PATH = os.path.abspath(lib_path)
    return mod


def context(pkg, mask_filter):
    lens = pkg.load_lens_file("dgauss11.lens")
    mask = pkg.load_aperture_png("pentbig500_14.png")
    efl = pkg.paraxial_efl(lens)
    lf = pkg.LensFlare(0)
    lf.set_frame(W, H)
    lf.set_params(1, 25.0, 1.0)
    if mask_filter is not None:
        lf.set_mask_filter(mask_filter)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_aperture(pkg.APERTURE_GHOST, mask)
    lf.set_lens(lens)
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
    ap.add_argument("--parent-lib", default=None, help="liblensflare_hip.so built from the parent commit")
    args = ap.parse_args()
    pkg = g.load_package()
    legs = {}
    if args.parent_lib:
        legs["parent_nearest"] = context(package_on(args.parent_lib), None)
    legs["nearest"] = context(pkg, pkg.MASK_NEAREST)
    legs["bilinear"] = context(pkg, pkg.MASK_BILINEAR)
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
    out = {"what": "c3 frame, dgauss11.lens, pentagon mask under LF_MASK_NEAREST against LF_MASK_BILINEAR "
                   "(and nearest on the parent commit's library), one process, legs alternated",
           "W": W, "H": H, "spp": SPP, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}
    for name, v in ms.items():
        out[name] = {"ms": [round(x, 3) for x in v], "median_ms": round(statistics.median(v), 3),
                     "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                     "stdev_ms": round(statistics.stdev(v), 3) if len(v) > 1 else 0.0}
    out["bilinear_over_nearest_median"] = round(out["bilinear"]["median_ms"] / out["nearest"]["median_ms"], 4)
    if args.parent_lib:
        p, n = out["parent_nearest"], out["nearest"]
        out["nearest_over_parent_median"] = round(n["median_ms"] / p["median_ms"], 4)
        out["nearest_within_noise_of_parent"] = bool(n["median_ms"] <= p["median_ms"] + 3.0 * max(p["stdev_ms"], n["stdev_ms"]))
    for name in ("nearest", "bilinear"):
        lf, frame = legs[name]
        lf.reset_counters()
        frame()
        out[name + "_march_stats"] = lf.march_stats()
        out[name + "_counters"] = {k: lf.counters()[k] for k in ("rays_hit_light", "rays_clipped_stop")}
    print(json.dumps(out, indent=1))
    for lf, _ in legs.values():
        lf.close()


if __name__ == "__main__":
    main()
