"""c3 frame (1920 x 1080, 256 spp, 46 paths x 3 wavelengths): the sun through this tree and through the parent commit's library,
the sun replaced by a point light 1 m away in the same direction, 2 and 4 mixed lights; started fraction with and without the
widening.  One process, legs alternated.
    python3 profiles/near_light_cost.py --parent-lib PATH [--out FILE]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "lens-flare_amd")


def load(name, lib_path=None):
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "__init__.py"), submodule_search_locations=[PKG])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    if lib_path:
        mod.LIB_PATH = lib_path
    return mod


ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True, help="liblensflare_hip.so built from the parent commit")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "near_light_cost.json"))
args = ap.parse_args()
new = load("lens_flare_amd")
old = load("lens_flare_amd_parent", os.path.abspath(args.parent_lib))
W, H, SPP, KEY = 1920, 1080, 256, 0x1e45f1a4e
ROUNDS, FRAMES = 4, 3
lens = new.load_lens_file("dgauss11.lens")
mask = new.load_aperture_png("pentbig500_14.png")
efl = new.paraxial_efl(lens)
sw = lens["sensor_width_mm"]
sun = np.array([(0.521445 - 0.5) * sw / efl, (0.517156 - 0.5) * sw * H / W / efl, -1.0])
unit = sun / np.linalg.norm(sun)
RAD = [1.0, 0.9, 0.5]
DIRS = [[-0.17871973878065694, -0.08042388245129563, -1.0], [0.20016610743433583, 0.0804238824512956, -1.0],
        [0.14297579102452554, -0.1125934354318139, -1.0]]      # (profiles/multi_light_cost.json's lights 1 .. 3)


def at(direction, dist):
    d = np.asarray(direction, np.float64)
    return list(dist * d / np.linalg.norm(d))


def context(pkg):
    lf = pkg.LensFlare(0)
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(2)
    lf.timing_enable(True)
    return lf


ctx_new, ctx_old = context(new), context(old)
ALPHA = 0.05
LEGS = {
    "sun_this_tree": (ctx_new, lambda c: c.set_sun(list(sun), RAD, ALPHA)),
    "sun_parent": (ctx_old, lambda c: c.set_sun(list(sun), RAD, ALPHA)),
    "lamp_1m": (ctx_new, lambda c: c.set_lights_ex([1], [at(sun, 1000.0)], [RAD], [ALPHA])),
    "lamp_300mm": (ctx_new, lambda c: c.set_lights_ex([1], [at(sun, 300.0)], [RAD], [ALPHA])),
    "lamp_100mm": (ctx_new, lambda c: c.set_lights_ex([1], [at(sun, 100.0)], [RAD], [ALPHA])),
    "2_mixed": (ctx_new, lambda c: c.set_lights_ex([0, 1], [list(sun), at(DIRS[0], 1000.0)], [RAD] * 2, [ALPHA] * 2)),
    "2_directional": (ctx_new, lambda c: c.set_lights([list(sun), DIRS[0]], [RAD] * 2, [ALPHA] * 2)),
    "4_mixed": (ctx_new, lambda c: c.set_lights_ex([0, 1, 0, 1], [list(sun), at(DIRS[0], 1000.0), DIRS[1], at(DIRS[2], 2000.0)], [RAD] * 4, [ALPHA] * 4)),
    "4_directional": (ctx_new, lambda c: c.set_lights([list(sun)] + DIRS, [RAD] * 4, [ALPHA] * 4)),
}
out = {"what": "c3 frame (1920 x 1080, 256 spp, 46 paths x 3 wavelengths), cull table rebuilt and audited in every timed frame; a frame = "
               "install the lights + lf_trace_ghosts + synchronize; one process, legs alternated",
       "W": W, "H": H, "spp": SPP, "rounds": ROUNDS, "frames_per_round": FRAMES, "angular_radius": ALPHA, "sun": list(sun), "legs": {}}
ms = {k: [] for k in LEGS}
info = {}
for k, (c, install) in LEGS.items():        # warm-up: every leg once
    install(c)
    c.trace_ghosts(SPP, KEY)
    c.synchronize()
for r in range(ROUNDS):
    for k, (c, install) in LEGS.items():
        for f in range(FRAMES):
            t0 = time.perf_counter()
            install(c)
            c.trace_ghosts(SPP, KEY)
            c.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
        info[k] = dict(started_fraction=round(c.cull_started_fraction(), 6), culled=c.cull_info()["culled"], reason=c.cull_reason(),
                       audit=c.cull_audit(), rays_hit_light=c.counters()["rays_hit_light"])
        c.reset_counters()
for k in LEGS:
    v = ms[k]
    out["legs"][k] = dict(ms=[round(x, 3) for x in v], median_ms=round(statistics.median(v), 3), mean_ms=round(statistics.mean(v), 3),
                          min_ms=round(min(v), 3), max_ms=round(max(v), 3), stdev_ms=round(statistics.stdev(v), 3), **info[k])
# the started fraction with and without the widening (a table wrong by construction: counted, not used)
wid = {}
for name, dist in (("lamp_1m", 1000.0), ("lamp_300mm", 300.0), ("lamp_100mm", 100.0)):
    row = {}
    for knob in (0, 1):
        ctx_new.test_knob("cull_no_widening", knob)
        ctx_new.set_lights_ex([1], [at(sun, dist)], [RAD], [ALPHA])
        ctx_new.reset_counters()
        ctx_new.trace_ghosts(SPP, KEY)
        ctx_new.synchronize()
        row["not_widened" if knob else "widened"] = dict(started_fraction=round(ctx_new.cull_started_fraction(), 6), reason=ctx_new.cull_reason(),
                                                         audit_lit=ctx_new.cull_audit()["lit"])
    ctx_new.test_knob("cull_no_widening", 0)
    wid[name] = row
ctx_new.set_sun(list(sun), RAD, ALPHA)
ctx_new.trace_ghosts(SPP, KEY)
wid["sun"] = dict(started_fraction=round(ctx_new.cull_started_fraction(), 6))
out["started_fraction_by_distance"] = wid
a, b = out["legs"]["sun_this_tree"], out["legs"]["sun_parent"]
out["sun_this_tree_minus_parent_mean_ms"] = round(a["mean_ms"] - b["mean_ms"], 3)
out["sun_agree_within_spread"] = abs(a["mean_ms"] - b["mean_ms"]) <= 2 * max(a["stdev_ms"], b["stdev_ms"])
with open(args.out, "w") as f:
    json.dump(out, f)
    f.write("\n")
print(json.dumps({k: (v["median_ms"], v["started_fraction"], v["reason"]) for k, v in out["legs"].items()}))
print(json.dumps(wid))
ctx_new.close()
ctx_old.close()
