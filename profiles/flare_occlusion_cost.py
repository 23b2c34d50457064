#!/usr/bin/env python3
"""What flare occlusion costs: the reference-faithful 1080p flare frame of profiles/flare_frame_timing.py (find_sun_pos ->
paraxial ghosts -> flare layer, counter jitter, pentagon mask) in ONE process, the legs alternated `--rounds` times, `--steps`
timed frames per leg and round after `--warmup` untimed ones (profiles/ghost_occlusion_cost.py's scheme).  A timed frame is:
lf_find_sun_pos, lf_generate_ghost_buffer, lf_render_flare_layer, synchronize -- wall clock
around it, and the library's own HIP events per kernel.

  off               the setting off: the kernels of the parent commit
  off_parent        the same frame through the parent commit's library (--parent-lib)
  on_<scene>_R<R>_n<n>   on, R rays per flare, n flares, from the front element of the double-Gauss prescription, with the tree
                    of pyramid.dae / maxplanck.dae resident and the camera placed above it: every shadow ray walks, none is blocked
  on_<scene>_at_R1024_n<n>   the camera in front of the model instead, looking at it: the rays descend the tree (the
                    visibilities found are in the record)

Usage (repo root, one MI355X): python3 profiles/flare_occlusion_cost.py --parent-lib <the parent's liblensflare_hip.so> > profiles/flare_occlusion_cost.json"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

W, H = 1920, 1080
HF = 50.0
VF = 2 * math.degrees(math.atan(math.tan(math.radians(HF) / 2) * H / W))
WPM, ALPHA = 0.001, 0.00465
KERNELS = ("frame_setup", "ghost_raster", "flare_layer", "flare_visibility")


def context(pkg, scene, R, n, lib=None, at=False):
    lf = pkg.LensFlare.__new__(pkg.LensFlare) if lib is not None else pkg.LensFlare(0)
    if lib is not None:          # the parent commit's library behind the same wrapper (it lacks only the new calls)
        lib.lf_last_error.restype = C.c_char_p
        lib.lf_last_error.argtypes = [C.c_void_p]
        lf.lib, lf.W, lf.H, lf._owned, lf.ctx = lib, 0, 0, True, C.c_void_p()
        assert lib.lf_create(C.byref(lf.ctx), 0) == 0
    lf.timing_enable(True)
    lf.set_frame(W, H)
    lf.set_params(1, 25.0, 1.0)
    lf.set_aperture(pkg.APERTURE_STARBURST, pkg.load_aperture_png("pentbig500_14.png"))
    lf.set_aperture(pkg.APERTURE_GHOST, pkg.load_aperture_png("octagonbokeh.png"))
    lf.set_jitter_counter(0x1e45f1a4e)
    pos = np.zeros(3)
    if scene:
        lf.load_collada(os.path.join(ROOT, "lens-flare_amd", "data", scene + ".dae"))
        lo, hi, _ = lf.scene_bounds()
        ext = hi - lo
        # over the model, looking along -z: no beam of the frame sinks faster than tan(vFov / 2) + a little per unit of
        # length; the camera stands that much above the model's top all along it
        pos = np.array([0.5 * (lo[0] + hi[0]), hi[1] + (math.tan(math.radians(VF) / 2) + 0.05) * (ext[2] + 0.5) + 0.1, hi[2] + 0.5])
        if at:   # in front of the model and below its middle, looking at it: the upper half of the frame is full of it
            d = 1.2 * float(max(ext))
            pos = np.array([0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]) - 0.4 * d * math.tan(math.radians(VF) / 2), hi[2] + d])
    lf.set_camera(np.eye(3), pos, HF, VF)
    ex, ey = math.tan(math.radians(HF) / 2), math.tan(math.radians(VF) / 2)
    # the flares in the upper half of the frame (above the horizon of the camera's own height)
    spots = [(0.62, 0.58), (0.3, 0.7), (0.8, 0.9), (0.45, 0.62), (0.2, 0.55), (0.7, 0.75), (0.55, 0.95), (0.9, 0.6)][:max(n, 1)]
    lights = [[pos[0] + (2 * x - 1) * ex * 1e6, pos[1] + (2 * y - 1) * ey * 1e6, pos[2] - 1e6, 1.0, 0.9, 0.5] for x, y in spots]
    if R:
        lf.set_lens(pkg.load_lens_file("dgauss11.lens"))
        lf.set_flare_occlusion(True, R, ALPHA, pkg.FLARE_ORIGIN_FRONT_ELEMENT, WPM)

    def frame():
        lf.find_sun_pos(lights)
        lf.generate_ghost_buffer()
        lf.render_flare_layer()
    return lf, frame


def summary(v):
    return {"ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4), "mean_ms": round(statistics.mean(v), 4),
            "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "stdev_ms": round(statistics.stdev(v), 4) if len(v) > 1 else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    pkg = g.load_package()
    legs = {"off": context(pkg, None, 0, 1)}
    if args.parent_lib:
        legs["off_parent"] = context(pkg, None, 0, 1, C.CDLL(os.path.abspath(args.parent_lib)))
    for scene in ("pyramid", "maxplanck"):
        for n in (1, 8):
            legs[f"off_{scene}_n{n}"] = context(pkg, scene, 0, n)
            for R in (256, 1024, 4096):
                legs[f"on_{scene}_R{R}_n{n}"] = context(pkg, scene, R, n)
            legs[f"on_{scene}_at_R1024_n{n}"] = context(pkg, scene, 1024, n, at=True)
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
    out = {"what": "the 1080p reference flare frame (find_sun_pos + generate_ghost_buffer + render_flare_layer + synchronize, counter "
                   "jitter); wall clock per frame and HIP-event device time per kernel; one process, legs alternated",
           "W": W, "H": H, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "frames_per_leg": args.steps * args.rounds,
           "legs": {}}
    for name, (ctx, frame) in legs.items():
        rec = summary(ms[name])
        ctx.timing_reset()
        for _ in range(args.steps):
            frame()
        ctx.synchronize()
        dev = 0.0
        for k in KERNELS:
            if k == "flare_visibility" and name == "off_parent":
                continue
            n, t = ctx.timing_get(k)
            rec[k + "_ms"] = round(t / n, 5) if n else None
            rec[k + "_entries_per_frame"] = n / args.steps
            dev += t / args.steps
        rec["device_ms_per_frame"] = round(dev, 5)
        if name.startswith("on_"):
            fv = ctx.flare_visibility()
            rec.update(flares=fv["n"], visibility=[float(v) for v in fv["visibility"]], scene_primitives=int(ctx.scene_bounds()[2]))
        out["legs"][name] = rec
    L = out["legs"]
    for name in L:
        if name.startswith("on_"):
            base = "off_" + name.split("_")[1] + "_" + name.split("_")[-1]
            out[f"{name}_minus_{base}_device_ms"] = round(L[name]["device_ms_per_frame"] - L[base]["device_ms_per_frame"], 5)
            out[f"{name}_minus_{base}_wall_median_ms"] = round(L[name]["median_ms"] - L[base]["median_ms"], 4)
    if args.parent_lib:
        out["off_minus_off_parent_mean_ms"] = round(L["off"]["mean_ms"] - L["off_parent"]["mean_ms"], 4)
        out["off_minus_off_parent_device_ms"] = round(L["off"]["device_ms_per_frame"] - L["off_parent"]["device_ms_per_frame"], 5)
        out["off_agrees_with_off_parent_within_spread"] = (abs(L["off"]["mean_ms"] - L["off_parent"]["mean_ms"])
                                                           <= L["off"]["stdev_ms"] + L["off_parent"]["stdev_ms"])
    print(json.dumps(out, indent=1))
    for ctx, _ in legs.values():
        ctx.close()


if __name__ == "__main__":
    main()
