#!/usr/bin/env python3
"""What several lights in one pass of the march cost: the c3 frame of bench.py (1920 x 1080, 256 spp, primary + 45 pairs x 3
wavelengths, pentagon mask; lf_set_march_culling(2): the table resolved and audited inside every timed frame) in ONE process,
the legs alternated `--rounds` times, `--steps` timed frames per leg and round after `--warmup` untimed ones.  A timed frame
is: install the lights, lf_trace_ghosts, synchronize (no flare layer: the lights' starbursts cost the same either way).

  one light        this tree's library against the parent commit's (--parent-lib, built from the parent's sources), the same
                   single sun: nothing a single-light frame launches has changed, so the two must agree within their own
                   run-to-run spread (both standard deviations are recorded)
  K = 2, 4, 8      K lights in ONE launch (lf_set_lights) against the same lights as K launches under lf_set_ghost_accumulate,
                   one lf_set_sun each: ms, the table's started fraction, executed events, rays that hit a light
  resolve          the pre-pass's time (lf_timing_get cull_prepass: the cached tree's resolve) with 1, 2, 4, 8 lights

Lights: light 0 is the bench's sun, the others are spread over the frame; 0.05 rad each.
Usage (repo root, one MI355X): python3 profiles/multi_light_cost.py --parent-lib <liblensflare_hip.so of the parent> > profiles/multi_light_cost.json"""
import argparse
import ctypes as C
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
W, H, SPP, KEY = 1920, 1080, 256, 0x1e45f1a4e
RAD = [1.0, 0.9, 0.5]
# normalised screen positions of lights 1 .. 7 (light 0: the bench's sun)
SPREAD = [(0.25, 0.30), (0.78, 0.70), (0.70, 0.22), (0.22, 0.75), (0.50, 0.15), (0.88, 0.45), (0.12, 0.50)]


def context(pkg, lib=None):
    lf = pkg.LensFlare.__new__(pkg.LensFlare) if lib is not None else pkg.LensFlare(0)
    if lib is not None:          # the parent commit's library behind the same wrapper (it lacks only the new calls)
        lib.lf_last_error.restype = C.c_char_p
        lib.lf_last_error.argtypes = [C.c_void_p]
        lf.lib, lf.W, lf.H, lf._owned, lf.ctx = lib, 0, 0, True, C.c_void_p()
        assert lib.lf_create(C.byref(lf.ctx), 0) == 0
    lens = pkg.load_lens_file("dgauss11.lens")
    mask = pkg.load_aperture_png("pentbig500_14.png")
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(2)
    lf.set_band(0, H)
    lf.timing_enable(True)
    return lf, lens


def directions(pkg, lens, n):
    efl = pkg.paraxial_efl(lens)
    sw = lens["sensor_width_mm"]
    sh = sw * H / W
    pos = [SUN_NS] + SPREAD
    return [[(nx - 0.5) * sw / efl, (ny - 0.5) * sh / efl, -1.0] for nx, ny in pos[:n]]


def summary(v):
    return {"ms": [round(x, 3) for x in v], "median_ms": round(statistics.median(v), 3), "mean_ms": round(statistics.mean(v), 3),
            "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "stdev_ms": round(statistics.stdev(v), 3) if len(v) > 1 else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    pkg = g.load_package()
    lf, lens = context(pkg)
    dirs = directions(pkg, lens, 8)

    def one_launch(ctx, n):
        def frame():
            if n == 1:
                ctx.set_sun(dirs[0], RAD, 0.05)
            else:
                ctx.set_lights(dirs[:n], [RAD] * n, [0.05] * n)
            ctx.set_ghost_accumulate(False)
            ctx.trace_ghosts(SPP, KEY)
        return frame

    def k_launches(ctx, n):
        def frame():
            for k in range(n):
                ctx.set_sun(dirs[k], RAD, 0.05)
                ctx.set_ghost_accumulate(k > 0)
                ctx.trace_ghosts(SPP, KEY)
            ctx.set_ghost_accumulate(False)
        return frame

    legs = {"one_light_this_tree": (lf, one_launch(lf, 1))}
    if args.parent_lib:
        parent, _ = context(pkg, C.CDLL(os.path.abspath(args.parent_lib)))
        legs["one_light_parent"] = (parent, one_launch(parent, 1))
    for n in (2, 4, 8):
        legs[f"{n}_lights_one_launch"] = (lf, one_launch(lf, n))
        legs[f"{n}_lights_{n}_launches"] = (lf, k_launches(lf, n))
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, (ctx, frame) in legs.items():
            for _ in range(args.warmup):
                frame()
            ctx.synchronize()
            for _ in range(args.steps):
                t0 = time.perf_counter()
                frame()
                ctx.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {"what": "c3 frame (1920 x 1080, 256 spp, 46 paths x 3 wavelengths), cull table resolved and audited in every timed frame; "
                   "a frame = install the lights + lf_trace_ghosts + synchronize; one process, legs alternated",
           "W": W, "H": H, "spp": SPP, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "frames_per_leg": args.steps * args.rounds, "light_directions": dirs, "angular_radius": 0.05, "legs": {}}
    for name, (ctx, frame) in legs.items():
        rec = summary(ms[name])
        # what one frame of the leg starts and executes (counters of ONE more frame)
        ctx.reset_counters()
        ctx.timing_reset()
        frame()
        ctx.synchronize()
        c = ctx.counters()
        rec.update(started_fraction=round(ctx.cull_started_fraction(), 6), executed_events=ctx.march_stats()["executed_events"],
                   rays_launched=c["rays_launched"], rays_hit_light=c["rays_hit_light"], culled=ctx.cull_info()["culled"],
                   cull_prepass_ms_per_launch=round(ctx.timing_get("cull_prepass")[1] / max(1, ctx.timing_get("cull_prepass")[0]), 4),
                   cull_audit_ms_per_launch=round(ctx.timing_get("cull_audit")[1] / max(1, ctx.timing_get("cull_audit")[0]), 4),
                   march_ms=round(ctx.timing_get("march")[1], 3))
        out["legs"][name] = rec
    L = out["legs"]
    if args.parent_lib:
        a, b = L["one_light_this_tree"], L["one_light_parent"]
        out["one_light_this_tree_minus_parent_mean_ms"] = round(a["mean_ms"] - b["mean_ms"], 3)
        out["one_light_agree_within_spread"] = abs(a["mean_ms"] - b["mean_ms"]) <= a["stdev_ms"] + b["stdev_ms"]
    for n in (2, 4, 8):
        one, many = L[f"{n}_lights_one_launch"], L[f"{n}_lights_{n}_launches"]
        out[f"{n}_lights_one_launch_over_{n}_launches_median"] = round(one["median_ms"] / many["median_ms"], 4)
        out[f"{n}_lights_one_launch_over_one_light_median"] = round(one["median_ms"] / L["one_light_this_tree"]["median_ms"], 4)
    # the pre-pass (the cached tree's resolve) by the number of lights
    out["resolve_ms_by_lights"] = {"1": L["one_light_this_tree"]["cull_prepass_ms_per_launch"]}
    for n in (2, 4, 8):
        out["resolve_ms_by_lights"][str(n)] = L[f"{n}_lights_one_launch"]["cull_prepass_ms_per_launch"]
    print(json.dumps(out))
    for ctx in {id(c): c for c, _ in legs.values()}.values():
        ctx.close()


if __name__ == "__main__":
    main()
