"""The scene term under lens camera mode 1 at 4K (3840 x 2160, 256 samples per pixel asked, the adaptive early-out on: the frame of
profiles/lenscam_surfaces_cost.py), data/pyramid.dae, one MI355X, one process, medians of 8 frames (4 rounds x 2) with min and max:
  plain / asph / anam _this_tree and _parent
                      dgauss11.lens under the default setting, dgauss11_asph.lens and dgauss11_anamorphic.lens under
                      LF_LENSCAM_SURFACES_ALL, through this tree's library and through the parent commit's; the two legs of a
                      pair take turns (they swap places every round); the frame and the scene counters must be the parent's bit
                      for bit; the kernels are the same code, so the margin for this tree's median is the parent leg's own
                      min - max spread (the script fails if a frame, a counter or that margin is missed)
  decentred_posed     dgauss11_decentred.lens under LF_LENSCAM_SURFACES_POSED: k_scene_lens<false, false, false, 3>
  decentred_cleared   the same prescription with its pose records cleared, under ALL: k_scene_lens<false, false, false, 2>
                      (it keeps its toroid's biconic record).  Their ratio is a number to record, not a bar.
  *_soft              the last two with the direct lighting sampled over the hemisphere (the SOFT instantiations, 1 wave per SIMD)
A frame = lf_render_scene_term + synchronize.
    python3 profiles/lenscam_poses_cost.py --parent-lib PATH [--out FILE]"""
import argparse
import importlib.util
import json
import math
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lenscam_poses_cost.json"))
args = ap.parse_args()
new = load("lens_flare_amd")
old = load("lens_flare_amd_parent", os.path.abspath(args.parent_lib))
W, H, SPP, KEY = 3840, 2160, 256, 0x1e45f1a4e
SUN_NS = (0.521445, 0.517156)               # bench.py's
ROUNDS, FRAMES = 4, 2
mask = new.load_aperture_png("pentbig500_14.png")


def context(pkg, lens_name, surfaces, soft=False, clear_poses=False):
    lens = pkg.load_lens_file(lens_name)
    if clear_poses:
        lens = {k: v for k, v in lens.items() if k != "poses"}
    lf = pkg.LensFlare(0)
    lf.set_frame(W, H)
    lf.set_params(SPP, 25.0, 1.0)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_aperture(pkg.APERTURE_GHOST, mask)
    lf.set_lens(lens)
    lf.set_jitter_counter(KEY)
    efl = pkg.paraxial_efl(lens)
    hf = 2 * math.degrees(math.atan(0.5 * lens["sensor_width_mm"] / efl))
    vf = 2 * math.degrees(math.atan(math.tan(math.radians(hf) / 2) * H / W))
    camera, suns = lf.load_collada(os.path.join(pkg.DATA, "pyramid.dae"))
    pos = np.array(camera["pos"], float) if camera else np.zeros(3)
    lf.set_camera(pkg.aim_camera(pos, suns[0][:3], SUN_NS, hf, vf), pos, hf, vf)
    if soft:
        lf.set_direct_hemisphere_sample(True)
    lf.set_lens_camera_surfaces(surfaces)
    lf.set_lens_camera(1, 0.001, 0.0)
    lf.set_band(0, H)
    return lf


PAIRS = {"plain": ("dgauss11.lens", 0), "asph": ("dgauss11_asph.lens", 1), "anam": ("dgauss11_anamorphic.lens", 1)}
legs = {}
for tag, (lens_name, surfaces) in PAIRS.items():
    legs[tag + "_this_tree"] = (new, context(new, lens_name, surfaces))
    legs[tag + "_parent"] = (old, context(old, lens_name, surfaces))
legs["decentred_posed"] = (new, context(new, "dgauss11_decentred.lens", new.LENSCAM_SURFACES_POSED))
legs["decentred_cleared"] = (new, context(new, "dgauss11_decentred.lens", new.LENSCAM_SURFACES_ALL, clear_poses=True))
legs["decentred_posed_soft"] = (new, context(new, "dgauss11_decentred.lens", new.LENSCAM_SURFACES_POSED, soft=True))
legs["decentred_cleared_soft"] = (new, context(new, "dgauss11_decentred.lens", new.LENSCAM_SURFACES_ALL, soft=True, clear_poses=True))
times = {k: [] for k in legs}
info = {}
for _, lf in legs.values():                   # warm-up (and the calibration)
    lf.render_scene_term(); lf.synchronize()
for rnd in range(ROUNDS):
    order = []
    for tag in PAIRS:
        pair = [tag + "_this_tree", tag + "_parent"]
        order += pair if rnd % 2 == 0 else pair[::-1]
    order += [k for k in legs if k not in order]
    for name in order:
        lf = legs[name][1]
        for _ in range(FRAMES):
            lf.reset_scene_counters()
            t0 = time.perf_counter()
            lf.render_scene_term()
            lf.synchronize()
            times[name].append(round((time.perf_counter() - t0) * 1e3, 3))
        info[name] = dict(counters=lf.scene_counters())
out = dict(what=__doc__.split("\n    python3")[0], W=W, H=H, spp=SPP, rounds=ROUNDS, frames_per_round=FRAMES, legs={})
for name, ms in times.items():
    c = info[name]["counters"]
    out["legs"][name] = dict(ms=ms, median_ms=round(statistics.median(ms), 3), min_ms=min(ms), max_ms=max(ms),
                             stdev_ms=round(statistics.pstdev(ms), 3), samples_per_pixel_taken=round(c["lens_samples"] / (W * H), 2),
                             **info[name])
ok = True
for tag in PAIRS:
    a, b = tag + "_this_tree", tag + "_parent"
    same_frame = bool(np.array_equal(legs[a][1].read_buffer(new.SCENE_BUFFER), legs[b][1].read_buffer(old.SCENE_BUFFER)))
    same_counters = bool(info[a]["counters"] == info[b]["counters"])
    A, B = out["legs"][a], out["legs"][b]
    out[tag + "_this_tree_vs_parent"] = dict(frame_equal=same_frame, counters_equal=same_counters,
                                             median_within_parents_min_max=bool(B["min_ms"] <= A["median_ms"] <= B["max_ms"]),
                                             median_not_above_parents_max=bool(A["median_ms"] <= B["max_ms"]))
    # (the two acceptance conditions of a pair: the parent's bits, and this tree's median inside the parent leg's own spread)
    ok = ok and same_frame and same_counters and out[tag + "_this_tree_vs_parent"]["median_within_parents_min_max"]
for soft in ("", "_soft"):
    p, c = out["legs"]["decentred_posed" + soft], out["legs"]["decentred_cleared" + soft]
    out["posed_over_cleared" + soft] = round(p["median_ms"] / c["median_ms"], 3)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps({k: [v["median_ms"], v["min_ms"], v["max_ms"], v["samples_per_pixel_taken"]] for k, v in out["legs"].items()}))
print(json.dumps({k: v for k, v in out.items() if k.endswith("_vs_parent") or k.startswith("posed_over")}))
for _, lf in legs.values():
    lf.close()
sys.exit(0 if ok else 1)
