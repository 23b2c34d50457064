"""The scene term under lens camera mode 1 at 4K (3840 x 2160, 256 samples per pixel asked, the adaptive early-out on: the shape
of bench.py's c4_1gpu frame and of the "7.6 ms at 4K" figure), data/pyramid.dae, one MI355X, one process, medians of 8 frames
(4 rounds x 2) with min and max:
  plain_this_tree / plain_parent   dgauss11.lens under the default setting through this tree's library and through the parent
                      commit's; the two legs take turns (they swap places every round), the frame and the scene counters must be
                      the parent's bit for bit (the script fails otherwise); the kernel is the same code, so the margin for this
                      tree's median is the parent's own min - max spread
  plain_all           dgauss11.lens under LF_LENSCAM_SURFACES_ALL: it launches the same kernel
  asph_all / anam_all dgauss11_asph.lens and dgauss11_anamorphic.lens under ALL: k_scene_lens<false, false, false, 1 / 2>,
                      bound to 2 waves per SIMD.  Numbers to record, not bars.
  *_soft              the same three lenses with the direct lighting sampled over the hemisphere (lf_set_direct_hemisphere_sample):
                      the SOFT instantiations -- SURF = 0 at 3 waves per SIMD with its scratch, SURF = 1 / 2 at 1 wave without
A frame = lf_render_scene_term + synchronize.
    python3 profiles/lenscam_surfaces_cost.py --parent-lib PATH [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lenscam_surfaces_cost.json"))
args = ap.parse_args()
new = load("lens_flare_amd")
old = load("lens_flare_amd_parent", os.path.abspath(args.parent_lib))
W, H, SPP, KEY = 3840, 2160, 256, 0x1e45f1a4e
SUN_NS = (0.521445, 0.517156)               # bench.py's
ROUNDS, FRAMES = 4, 2
mask = new.load_aperture_png("pentbig500_14.png")


def context(pkg, lens_name, surfaces_all, soft):
    lens = pkg.load_lens_file(lens_name)
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
    if surfaces_all:
        lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_ALL)
    lf.set_lens_camera(1, 0.001, 0.0)
    lf.set_band(0, H)
    return lf


legs = {"plain_this_tree": context(new, "dgauss11.lens", False, False), "plain_parent": context(old, "dgauss11.lens", False, False),
        "plain_all": context(new, "dgauss11.lens", True, False),
        "asph_all": context(new, "dgauss11_asph.lens", True, False), "anam_all": context(new, "dgauss11_anamorphic.lens", True, False),
        "plain_soft": context(new, "dgauss11.lens", True, True),
        "asph_all_soft": context(new, "dgauss11_asph.lens", True, True),
        "anam_all_soft": context(new, "dgauss11_anamorphic.lens", True, True)}
PAIR = ("plain_this_tree", "plain_parent")
times = {k: [] for k in legs}
info = {}
for lf in legs.values():                      # warm-up (and the calibration)
    lf.render_scene_term(); lf.synchronize()
for rnd in range(ROUNDS):
    order = list(PAIR if rnd % 2 == 0 else PAIR[::-1]) + [k for k in legs if k not in PAIR]
    for name in order:
        lf = legs[name]
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
a, b = PAIR
same_frame = bool(np.array_equal(legs[a].read_buffer(new.SCENE_BUFFER), legs[b].read_buffer(old.SCENE_BUFFER)))
same_counters = info[a]["counters"] == info[b]["counters"]
all_frame = bool(np.array_equal(legs[a].read_buffer(new.SCENE_BUFFER), legs["plain_all"].read_buffer(new.SCENE_BUFFER)))
A, B = out["legs"][a], out["legs"][b]
out["plain_this_tree_vs_parent"] = dict(frame_equal=same_frame, counters_equal=bool(same_counters),
                                        median_within_parents_min_max=bool(A["median_ms"] <= B["max_ms"]))
out["plain_all_vs_default"] = dict(frame_equal=all_frame, counters_equal=bool(info["plain_all"]["counters"] == info[a]["counters"]))
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps({k: [v["median_ms"], v["min_ms"], v["max_ms"], v["samples_per_pixel_taken"]] for k, v in out["legs"].items()}))
print(json.dumps({k: v for k, v in out.items() if k.endswith("_vs_parent") or k.endswith("_vs_default")}))
for lf in legs.values():
    lf.close()
sys.exit(0 if same_frame and same_counters and all_frame else 1)
