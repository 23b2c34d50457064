#!/usr/bin/env python3
"""What multi-layer coating stacks cost: the c3 frame of bench.py (1920 x 1080, 256 spp, primary + 45 pairs x 3 wavelengths,
pentagon mask; lf_set_march_culling(2): the table resolved and audited inside every timed frame) in ONE process, the legs
alternated `--rounds` times, `--steps` timed frames per leg and round after `--warmup` untimed ones.  A timed frame is:
lf_set_sun, lf_trace_ghosts, synchronize.

  bare            dgauss11.lens: the kVarBare kernels
  single_film     dgauss11_coated.lens (eight quarter-wave MgF2 films): the kVarCoat kernels
  stacks          dgauss11_multicoated.lens (eight three-layer stacks): the kVarCoat | kVarStack kernels
  bare_parent     the bare frame through the parent commit's library (--parent-lib, built from the parent's sources)

Nothing the bare and the single-film legs launch has changed, so both are compared with the parent's bare leg in the same
run: the bare legs' means must agree within their own run-to-run spread (the sum of the two standard deviations this run
shows), and so must the single-film leg's surcharge over the bare frame when the parent's library renders the coated lens
too (single_film_parent).  The stack's own cost is recorded as its ratio to the single-film frame.
Usage (repo root, one MI355X): python3 profiles/coating_stack_cost.py --parent-lib <liblensflare_hip.so of the parent> > profiles/coating_stack_cost.json"""
import argparse
import ctypes as C
import json
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


def context(pkg, lens_file, lib=None):
    lf = pkg.LensFlare.__new__(pkg.LensFlare) if lib is not None else pkg.LensFlare(0)
    if lib is not None:          # the parent commit's library behind the same wrapper (it lacks only the new calls)
        lib.lf_last_error.restype = C.c_char_p
        lib.lf_last_error.argtypes = [C.c_void_p]
        lf.lib, lf.W, lf.H, lf._owned, lf.ctx = lib, 0, 0, True, C.c_void_p()
        assert lib.lf_create(C.byref(lf.ctx), 0) == 0
    lens = pkg.load_lens_file(lens_file)
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, pkg.load_aperture_png("pentbig500_14.png"))
    lf.set_lens(lens)              # (applies the file's films or stacks, if it has any)
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(2)
    lf.set_band(0, H)
    lf.timing_enable(True)
    efl, sw = pkg.paraxial_efl(lens), lens["sensor_width_mm"]
    sun = [(SUN_NS[0] - 0.5) * sw / efl, (SUN_NS[1] - 0.5) * sw * H / W / efl, -1.0]

    def frame():
        lf.set_sun(sun, RAD, 0.05)
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
    legs = {"bare": context(pkg, "dgauss11.lens"), "single_film": context(pkg, "dgauss11_coated.lens"),
            "stacks": context(pkg, "dgauss11_multicoated.lens")}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        legs["bare_parent"] = context(pkg, "dgauss11.lens", parent)
        legs["single_film_parent"] = context(pkg, "dgauss11_coated.lens", parent)
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
                   "a frame = lf_set_sun + lf_trace_ghosts + synchronize; one process, legs alternated",
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
        out["legs"][name] = rec
    L = out["legs"]
    out["stacks_over_single_film_median"] = round(L["stacks"]["median_ms"] / L["single_film"]["median_ms"], 4)
    out["stacks_over_bare_median"] = round(L["stacks"]["median_ms"] / L["bare"]["median_ms"], 4)
    out["single_film_over_bare_median"] = round(L["single_film"]["median_ms"] / L["bare"]["median_ms"], 4)
    if args.parent_lib:
        for a, b in (("bare", "bare_parent"), ("single_film", "single_film_parent")):
            out[f"{a}_minus_{b}_mean_ms"] = round(L[a]["mean_ms"] - L[b]["mean_ms"], 3)
            out[f"{a}_agrees_with_{b}_within_spread"] = abs(L[a]["mean_ms"] - L[b]["mean_ms"]) <= L[a]["stdev_ms"] + L[b]["stdev_ms"]
    print(json.dumps(out))
    for ctx, _ in legs.values():
        ctx.close()


if __name__ == "__main__":
    main()
