"""c3 frame (1920 x 1080, 256 spp, 3 wavelengths), one MI355X, one process, medians of 8 frames (4 rounds x 2) with min and max.
WHAT THIS ADDS (numbers to record, not bars) -- sensor ghosts of dgauss11_decentred.lens, reflectance 0.05:
  posed_only / posed_add       under LF_SENSOR_SURFACES_POSED, LF_SENSOR_GHOSTS_ONLY / _ADD: k_march_sensor<VAR, 3>
  cleared_only / cleared_add   the same prescription with its pose records cleared (it keeps its toroid's biconic record):
                               k_march_sensor<VAR, 2>.  posed_over_cleared: the ratios of the medians, of the frame and of the
                               "march_sensor" slot alone (under ADD the ordinary march of a posed lens is most of the frame).
WHAT MUST NOT MOVE -- this tree's library and the parent commit's take turns (they swap places every round) on
  default              the default frame of dgauss11.lens
  sensor_only / _add   dgauss11_sensor.lens under LF_SENSOR_GHOSTS_ONLY / _ADD (the setting at its default)
  decentred_off        dgauss11_decentred.lens with sensor ghosts off
Each pair must give the parent's frame and counters bit for bit, and this tree's median must lie inside the parent leg's own
min - max over its 8 frames: the kernels are the same code (the script fails on any of the three).
A frame = lf_trace_ghosts + synchronize.
    python3 profiles/sensor_pose_cost.py --parent-lib PATH [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensor_pose_cost.json"))
args = ap.parse_args()
new = load("lens_flare_amd")
old = load("lens_flare_amd_parent", os.path.abspath(args.parent_lib))
W, H, SPP, KEY = 1920, 1080, 256, 0x1e45f1a4e
ROUNDS, FRAMES = 4, 2
plain = new.load_lens_file("dgauss11.lens")
sens = new.load_lens_file("dgauss11_sensor.lens")
posed = new.load_lens_file("dgauss11_decentred.lens")
cleared = {k: v for k, v in posed.items() if k != "poses"}
mask = new.load_aperture_png("pentbig500_14.png")
efl = new.paraxial_efl(plain)
sw = plain["sensor_width_mm"]
sun = [(0.521445 - 0.5) * sw / efl, (0.517156 - 0.5) * sw * H / W / efl, -1.0]


def context(pkg, lens, mode=None, refl=None, surfaces=None):
    lf = pkg.LensFlare(0)
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    lf.set_sun(sun, [1.0, 0.9, 0.5], 0.05)
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(2)
    if refl is not None:
        lf.set_sensor_reflectance(np.full(3, refl, np.float32))
    if surfaces is not None:
        lf.set_sensor_ghost_surfaces(surfaces)
    if mode is not None:
        lf.set_sensor_ghosts(mode)
    lf.timing_enable(True)
    return lf


PAIRS = {"default": (plain, None), "sensor_only": (sens, new.SENSOR_GHOSTS_ONLY), "sensor_add": (sens, new.SENSOR_GHOSTS_ADD),
         "decentred_off": (posed, None)}
legs = {}
for tag, (lens, mode) in PAIRS.items():
    legs[tag + "_this_tree"] = (new, context(new, lens, mode))
    legs[tag + "_parent"] = (old, context(old, lens, mode))
ADDED = ("posed_only", "posed_add", "cleared_only", "cleared_add")
legs["posed_only"] = (new, context(new, posed, new.SENSOR_GHOSTS_ONLY, 0.05, new.SENSOR_SURFACES_POSED))
legs["posed_add"] = (new, context(new, posed, new.SENSOR_GHOSTS_ADD, 0.05, new.SENSOR_SURFACES_POSED))
legs["cleared_only"] = (new, context(new, cleared, new.SENSOR_GHOSTS_ONLY, 0.05))
legs["cleared_add"] = (new, context(new, cleared, new.SENSOR_GHOSTS_ADD, 0.05))
times = {k: [] for k in legs}
kernel_ms = {k: [] for k in legs}
info = {}
for _, lf in legs.values():                      # warm-up
    lf.trace_ghosts(SPP, KEY); lf.synchronize()
for rnd in range(ROUNDS):
    order = []
    for tag in PAIRS:
        pair = [tag + "_this_tree", tag + "_parent"]
        order += pair if rnd % 2 == 0 else pair[::-1]
    order += list(ADDED)
    for name in order:
        pkg, lf = legs[name]
        for _ in range(FRAMES):
            lf.reset_counters()
            lf.timing_reset()
            t0 = time.perf_counter()
            lf.trace_ghosts(SPP, KEY)
            lf.synchronize()
            times[name].append(round((time.perf_counter() - t0) * 1e3, 3))
            kernel_ms[name].append(round(lf.timing_get("march_sensor")[1], 3))
        info[name] = dict(reason=lf.cull_reason(), counters=lf.counters(), executed_events=lf.executed_events(),
                          sensor_ghost_stats=lf.sensor_ghost_stats(), march_launches=lf.timing_get("march")[0],
                          march_sensor_launches=lf.timing_get("march_sensor")[0])
out = dict(what=__doc__.split("\n    python3")[0], W=W, H=H, spp=SPP, rounds=ROUNDS, frames_per_round=FRAMES, sun=sun, legs={})
for name, ms in times.items():
    k = kernel_ms[name]
    out["legs"][name] = dict(ms=ms, median_ms=round(statistics.median(ms), 3), min_ms=min(ms), max_ms=max(ms),
                             stdev_ms=round(statistics.pstdev(ms), 3),
                             march_sensor_ms=dict(ms=k, median_ms=round(statistics.median(k), 3), min_ms=min(k), max_ms=max(k)),
                             **info[name])
ok = True
for tag in PAIRS:
    a, b = tag + "_this_tree", tag + "_parent"
    same_frame = bool(np.array_equal(legs[a][1].read_buffer(new.GHOST_BUFFER), legs[b][1].read_buffer(old.GHOST_BUFFER)))
    same_counters = bool(info[a] == info[b])
    A, B = out["legs"][a], out["legs"][b]
    inside = bool(B["min_ms"] <= A["median_ms"] <= B["max_ms"])
    out[tag + "_this_tree_vs_parent"] = dict(frame_equal=same_frame, counters_equal=same_counters, median_within_parents_min_max=inside)
    ok = ok and same_frame and same_counters and inside
for mode in ("only", "add"):
    p, c = out["legs"]["posed_" + mode], out["legs"]["cleared_" + mode]
    out["posed_over_cleared_" + mode] = dict(frame=round(p["median_ms"] / c["median_ms"], 3),
                                             march_sensor=round(p["march_sensor_ms"]["median_ms"] / c["march_sensor_ms"]["median_ms"], 3))
only = legs["posed_only"][1].read_buffer(new.GHOST_BUFFER)
out["posed_add_equals_ordinary_plus_only"] = bool(np.array_equal(
    legs["posed_add"][1].read_buffer(new.GHOST_BUFFER), legs["decentred_off_this_tree"][1].read_buffer(new.GHOST_BUFFER) + only))
out["posed_only_frame_max"] = float(only.max())
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps({k: [v["median_ms"], v["min_ms"], v["max_ms"], v["march_sensor_ms"]["median_ms"]] for k, v in out["legs"].items()}))
print(json.dumps({k: v for k, v in out.items() if k.endswith("_vs_parent") or k.startswith("posed_")}))
for _, lf in legs.values():
    lf.close()
sys.exit(0 if ok else 1)
