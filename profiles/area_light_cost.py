"""c3 frame (1920 x 1080, 256 spp, 46 paths x 3 wavelengths): the sun through this tree and through the parent commit's library (the
kernels are the parent's), a 40 x 24 mm rectangle 300 mm away and a 500 x 500 mm panel 3 m away in the sun's direction against the
point light at the same centre, and the same four under ghost occlusion with LF_OCCLUSION_REACH_LIGHT behind a wall that covers
half the beam at half the distance.  One process, legs alternated.
    python3 profiles/area_light_cost.py --parent-lib PATH [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "area_light_cost.json"))
args = ap.parse_args()
new = load("lens_flare_amd")
old = load("lens_flare_amd_parent", os.path.abspath(args.parent_lib))
W, H, SPP, KEY = 1920, 1080, 256, 0x1e45f1a4e
ROUNDS, FRAMES = 4, 3
WPM = 0.001
lens = new.load_lens_file("dgauss11.lens")
mask = new.load_aperture_png("pentbig500_14.png")
efl = new.paraxial_efl(lens)
sw = lens["sensor_width_mm"]
sun = np.array([(0.521445 - 0.5) * sw / efl, (0.517156 - 0.5) * sw * H / W / efl, -1.0])
unit = sun / np.linalg.norm(sun)
z_ref = new.paraxial_entrance_pupil(lens)[0]
RAD = [1.0, 0.9, 0.5]
ALPHA = 0.05


def rect(dist, wx, wy):
    """a rectangle wx x wy mm square to the axis, its centre `dist` mm away in the sun's direction, facing the lens"""
    return np.concatenate([dist * unit, [0.0, 0.0, 1.0], [wx, 0.0, 0.0], [0.0, wy, 0.0]]).astype(np.float32)


def half_wall(dist):
    """world triangles: the half plane x < the beam's centre, `dist` lens millimetres in front of the front vertex"""
    z = (-dist - z_ref) * WPM
    x1 = dist * unit[0] / -unit[2] * WPM
    p = [(-4.0, -4.0, z), (x1, -4.0, z), (x1, 4.0, z), (-4.0, 4.0, z)]
    n = (0.0, 0.0, 1.0)
    row = lambda a, b, c: tuple(a + b + c + n + n + n) + ("d", 0.5, 0.5, 0.5)      # noqa: E731
    return [row(p[0], p[1], p[2]), row(p[0], p[2], p[3])]


def context(pkg, wall_at=None):
    lf = pkg.LensFlare(0)
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(2)
    lf.timing_enable(True)
    if wall_at is not None:
        lf.set_scene([], half_wall(wall_at), [])
        lf.set_camera(np.eye(3).reshape(-1), [0.0, 0.0, 0.0], 40.0, 27.0)
        lf.set_ghost_occlusion(True, WPM)
        lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_LIGHT)
    return lf


ctx_new, ctx_old, ctx_near, ctx_far = context(new), context(old), context(new, 150.0), context(new, 1500.0)
R300, R3M = rect(300.0, 40.0, 24.0), rect(3000.0, 500.0, 500.0)
area = lambda g: (lambda c: c.set_lights_geom([new.LIGHT_AREA], [g], [RAD], [0.0]))                    # noqa: E731
lamp = lambda g: (lambda c: c.set_lights_ex([new.LIGHT_POINT], [g[:3]], [RAD], [ALPHA]))               # noqa: E731
LEGS = {
    "sun_this_tree": (ctx_new, lambda c: c.set_sun(list(sun), RAD, ALPHA)),
    "sun_parent": (ctx_old, lambda c: c.set_sun(list(sun), RAD, ALPHA)),
    "lamp_300mm": (ctx_new, lamp(R300)),
    "rect_40x24_300mm": (ctx_new, area(R300)),
    "lamp_3m": (ctx_new, lamp(R3M)),
    "panel_500x500_3m": (ctx_new, area(R3M)),
    "lamp_300mm_occluded": (ctx_near, lamp(R300)),
    "rect_40x24_300mm_occluded": (ctx_near, area(R300)),
    "lamp_3m_occluded": (ctx_far, lamp(R3M)),
    "panel_500x500_3m_occluded": (ctx_far, area(R3M)),
}
out = {"what": "c3 frame (1920 x 1080, 256 spp, 46 paths x 3 wavelengths), cull table rebuilt and audited in every timed frame; a frame = "
               "install the lights + lf_trace_ghosts + synchronize; one process, legs alternated; occluded: LF_OCCLUSION_REACH_LIGHT behind a "
               "wall over half the beam at half the light's distance",
       "W": W, "H": H, "spp": SPP, "rounds": ROUNDS, "frames_per_round": FRAMES, "angular_radius_of_the_point_lights": ALPHA, "sun": list(sun),
       "legs": {}}
ms = {k: [] for k in LEGS}
info = {}
for k, (c, install) in LEGS.items():        # warm-up: every leg once
    install(c)
    c.trace_ghosts(SPP, KEY)
    c.synchronize()
for r in range(ROUNDS):
    for k, (c, install) in LEGS.items():
        c.reset_counters()
        for f in range(FRAMES):
            t0 = time.perf_counter()
            install(c)
            c.trace_ghosts(SPP, KEY)
            c.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
        info[k] = dict(started_fraction=round(c.cull_started_fraction(), 6), culled=c.cull_info()["culled"], reason=c.cull_reason(),
                       audit=c.cull_audit(), rays_hit_light=c.counters()["rays_hit_light"] // FRAMES,
                       march_variant=c.get_ghost_occlusion()["march_variant"] if c is not ctx_old else 0)
        if k.endswith("_occluded"):
            info[k]["occlusion"] = c.ghost_occlusion_stats()
for k in LEGS:
    v = ms[k]
    out["legs"][k] = dict(ms=[round(x, 3) for x in v], median_ms=round(statistics.median(v), 3), mean_ms=round(statistics.mean(v), 3),
                          min_ms=round(min(v), 3), max_ms=round(max(v), 3), stdev_ms=round(statistics.stdev(v), 3), **info[k])
a, b = out["legs"]["sun_this_tree"], out["legs"]["sun_parent"]
out["sun_this_tree_minus_parent_mean_ms"] = round(a["mean_ms"] - b["mean_ms"], 3)
out["sun_agree_within_spread"] = abs(a["mean_ms"] - b["mean_ms"]) <= 2 * max(a["stdev_ms"], b["stdev_ms"])
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({k: (v["median_ms"], v["stdev_ms"], v["started_fraction"], v["reason"]) for k, v in out["legs"].items()}))
for c in (ctx_new, ctx_old, ctx_near, ctx_far):
    c.close()
