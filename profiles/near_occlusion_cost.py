#!/usr/bin/env python3
"""What ghost occlusion costs for a point light (lf_set_ghost_occlusion_reach, LF_OCCLUSION_REACH_LIGHT: the kVarNear | kVarOccl
kernels): the c3 frame of bench.py (1920 x 1080, 256 spp, primary + 45 pairs x 3 wavelengths, pentagon mask;
lf_set_march_culling(2): the table resolved and audited inside every timed frame) in ONE process, the legs alternated
`--rounds` times, `--steps` timed frames per leg and round after `--warmup` untimed ones (profiles/ghost_occlusion_cost.py's
scheme).  A timed frame is: lf_set_lights_ex, lf_trace_ghosts, synchronize.  The lamp stands 1 m from the front vertex in the
bench's sun direction, 0.05 rad.

  off             the lamp, occlusion off: the kVarNear kernels of the parent commit
  off_parent      the same frame through the parent commit's library (--parent-lib)
  on_below        the lamp under REACH_LIGHT, maxplanck.dae (50 801 triangles) wholly below the beam: every shadow ray walks, none is blocked
  on_half         a wall half way to the lamp whose edge crosses the lamp's direction: about half of the shadow rays are blocked
  on_front        the wall covers the lamp: every shadow ray is blocked
  on_behind       the wall 2 m away, behind the lamp: every shadow ray walks to the lamp and ends there, none is blocked
  sun_on_below    the sun in the lamp's direction under occlusion, the scene of on_below: the kVarOccl kernels of the parent commit

The pass condition is only that `off` agrees with `off_parent` within the measured spread (the kernels are the parent's); the
new kernels' times are written down as measured, not held to a bar.  As measured on one MI355X (profiles/near_occlusion_cost.json,
medians of 12 frames, standard deviations 0.04 .. 0.16 ms): off 40.39 ms, off_parent 40.43 ms (means 40.40 / 40.45), on_below
212.17 ms, on_half 216.40 ms (148.9 M of 298.1 M shadow tests blocked), on_front 223.42 ms, on_behind 212.01 ms, sun_on_below
163.73 ms (310.7 M tests).

Usage (repo root, one MI355X): python3 profiles/near_occlusion_cost.py --parent-lib <the parent's liblensflare_hip.so> > profiles/near_occlusion_cost.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

SUN_NS = (0.521445, 0.517156)      # bench.py
W, H, SPP, KEY = 1920, 1080, 256, 0x1e45f1a4e
RAD = [1.0, 0.9, 0.5]
WPM = 0.001
LAMP_MM = 1000.0
LEGS = ("off", "on_below", "on_half", "on_front", "on_behind", "sun_on_below")


def quad(c, u, v, hu0, hu1, hv):
    """two triangles: c + s u + t v, s in [hu0, hu1], t in [-hv, hv]"""
    p = [c + s * u + t * v for s, t in ((hu0, -hv), (hu1, -hv), (hu1, hv), (hu0, hv))]
    n = [0.0, 0.0, 1.0]
    row = lambda a, b, d: tuple(list(a) + list(b) + list(d) + n * 3) + ("d", 0.5, 0.5, 0.5)      # noqa: E731
    return [row(p[0], p[1], p[2]), row(p[0], p[2], p[3])]


def context(pkg, leg, lib=None):
    lf = pkg.LensFlare.__new__(pkg.LensFlare) if lib is not None else pkg.LensFlare(0)
    if lib is not None:          # the parent commit's library behind the same wrapper (it lacks only the new calls)
        lib.lf_last_error.restype = C.c_char_p
        lib.lf_last_error.argtypes = [C.c_void_p]
        lf.lib, lf.W, lf.H, lf._owned, lf.ctx = lib, 0, 0, True, C.c_void_p()
        assert lib.lf_create(C.byref(lf.ctx), 0) == 0
    lens = pkg.load_lens_file("dgauss11.lens")
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, pkg.load_aperture_png("pentbig500_14.png"))
    lf.set_lens(lens)
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(2)
    lf.set_band(0, H)
    lf.timing_enable(True)
    efl, sw = pkg.paraxial_efl(lens), lens["sensor_width_mm"]
    sun = np.array([(SUN_NS[0] - 0.5) * sw / efl, (SUN_NS[1] - 0.5) * sw * H / W / efl, -1.0])
    s = sun / np.sqrt((sun * sun).sum())
    lamp = LAMP_MM * s                                   # lens millimetres, the front vertex at the origin
    if leg != "off":
        z_ref = pkg.paraxial_entrance_pupil(lens)[0]
        u = np.array([-s[2], 0.0, s[0]]); u /= np.sqrt((u * u).sum())
        v = np.cross(s, u)
        pos = np.zeros(3)
        at = lambda mm: (mm * s - np.array([0.0, 0.0, z_ref])) * WPM      # noqa: E731  (lens mm along the lamp's direction -> world)
        if leg.endswith("_below"):
            lf.load_collada(os.path.join(ROOT, "lens-flare_amd", "data", "maxplanck.dae"))
            lo, hi, _ = lf.scene_bounds()
            ext = hi - lo
            # over the model, looking along -z: the beam (the lobe's 0.05 rad around the light + the front element) sinks less
            # than 0.1 per unit of length, the camera stands that much above the model's top all along it
            pos = np.array([0.5 * (lo[0] + hi[0]), hi[1] + 0.1 * (ext[2] + 0.5) + 0.1, hi[2] + 0.5])
        elif leg == "on_half":
            lf.set_scene([], quad(at(0.5 * LAMP_MM), u, v, -4.0, 0.0, 4.0), [])
        elif leg == "on_front":
            lf.set_scene([], quad(at(0.5 * LAMP_MM), u, v, -4.0, 4.0, 4.0), [])
        else:
            lf.set_scene([], quad(at(2.0 * LAMP_MM), u, v, -4.0, 4.0, 4.0), [])
        lf.set_camera(np.eye(3).reshape(-1), pos, 40.0, 27.0)
        lf.set_ghost_occlusion(True, WPM)
        lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_LIGHT)

    def frame():
        if leg.startswith("sun_"):
            lf.set_lights_ex([pkg.LIGHT_DIRECTIONAL], [sun], [RAD], [0.05])
        else:
            lf.set_lights_ex([pkg.LIGHT_POINT], [lamp], [RAD], [0.05])
        lf.trace_ghosts(SPP, KEY)
    return lf, frame


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
    legs = {name: context(pkg, name) for name in LEGS}
    if args.parent_lib:
        legs["off_parent"] = context(pkg, "off", C.CDLL(os.path.abspath(args.parent_lib)))
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
    out = {"what": "c3 frame (1920 x 1080, 256 spp, 46 paths x 3 wavelengths), a lamp 1 m away in the bench's sun direction, cull table "
                   "resolved and audited in every timed frame; a frame = lf_set_lights_ex + lf_trace_ghosts + synchronize; one process, "
                   "legs alternated",
           "W": W, "H": H, "spp": SPP, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "frames_per_leg": args.steps * args.rounds, "legs": {}}
    for name, (ctx, frame) in legs.items():
        rec = summary(ms[name])
        ctx.reset_counters()
        ctx.timing_reset()
        frame()
        ctx.synchronize()
        c = ctx.counters()
        rec.update(executed_events=ctx.march_stats()["executed_events"], rays_launched=c["rays_launched"],
                   rays_hit_light=c["rays_hit_light"], culled=ctx.cull_info()["culled"], march_ms=round(ctx.timing_get("march")[1], 3))
        if name != "off_parent":
            st = ctx.ghost_occlusion_stats()
            rec.update(shadow_tests=st["tested"], shadow_tests_blocked=st["blocked"], march_variant=ctx.get_ghost_occlusion()["march_variant"])
        if name.endswith("_below"):
            rec["scene_primitives"] = int(ctx.scene_bounds()[2])
        out["legs"][name] = rec
    L = out["legs"]
    for name in LEGS[1:]:
        out[f"{name}_over_off_median"] = round(L[name]["median_ms"] / L["off"]["median_ms"], 4)
    if args.parent_lib:
        out["off_minus_off_parent_mean_ms"] = round(L["off"]["mean_ms"] - L["off_parent"]["mean_ms"], 3)
        out["off_agrees_with_off_parent_within_spread"] = (abs(L["off"]["mean_ms"] - L["off_parent"]["mean_ms"])
                                                           <= L["off"]["stdev_ms"] + L["off_parent"]["stdev_ms"])
    print(json.dumps(out))
    for ctx, _ in legs.values():
        ctx.close()


if __name__ == "__main__":
    main()
