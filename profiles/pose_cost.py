"""c3 frame (1920 x 1080, 256 spp, 3 wavelengths), one MI355X, one process, medians of 8 frames (4 rounds x 2) with min and max:
  decentred / decentred_cleared   dgauss11_decentred.lens (11 interfaces, 45 pairs + the primary path; four pose records, one
                      biconic record) through k_march_asph<VAR, true, true>, and the same prescription with its poses cleared
                      (lf_set_lens_poses(NULL): the biconic record stays) through k_march_asph<VAR, true>.  Both go through the
                      per-path Newton march, so their ratio is the price of the transform: a number to record, not a bar
  default_this_tree / default_parent   the default launch (culled) of dgauss11.lens through this tree's library and through the
                      parent commit's
  asph_this_tree / asph_parent         dgauss11_asph.lens (k_march_asph<VAR>) through both
  anam_this_tree / anam_parent         dgauss11_anamorphic.lens (k_march_asph<VAR, true>) through both
The two legs of a pair take turns (they swap places every round).  The three pairs must give the parent's frame and counters
bit for bit, and each median of this tree must lie inside the parent leg's own min - max over its 8 frames: nothing those
frames launch has changed (the script fails otherwise).
A frame = lf_trace_ghosts + synchronize.
    python3 profiles/pose_cost.py --parent-lib PATH [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_cost.json"))
ap.add_argument("--compile-times", default=None, help="JSON text recorded beside the frames (compile times of both trees)")
args = ap.parse_args()
new = load("lens_flare_amd")
old = load("lens_flare_amd_parent", os.path.abspath(args.parent_lib))
W, H, SPP, KEY = 1920, 1080, 256, 0x1e45f1a4e
ROUNDS, FRAMES = 4, 2
plain = new.load_lens_file("dgauss11.lens")
asph = new.load_lens_file("dgauss11_asph.lens")
anam = new.load_lens_file("dgauss11_anamorphic.lens")
posed = new.load_lens_file("dgauss11_decentred.lens")
mask = new.load_aperture_png("pentbig500_14.png")
efl = new.paraxial_efl(plain)
sw = plain["sensor_width_mm"]
sun = [(0.521445 - 0.5) * sw / efl, (0.517156 - 0.5) * sw * H / W / efl, -1.0]


def context(pkg, lens, cull, clear_poses=False):
    lf = pkg.LensFlare(0)
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    if "poses" in lens and pkg is old:
        raise SystemExit("the parent's library knows no pose records")
    lf.set_lens(lens)
    if clear_poses:
        lf.set_lens_poses(None)
    lf.set_sun(sun, [1.0, 0.9, 0.5], 0.05)
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(cull)
    return lf


legs = {"decentred": context(new, posed, 1), "decentred_cleared": context(new, posed, 1, True),
        "default_this_tree": context(new, plain, 2), "default_parent": context(old, plain, 2),
        "asph_this_tree": context(new, asph, 1), "asph_parent": context(old, asph, 1),
        "anam_this_tree": context(new, anam, 1), "anam_parent": context(old, anam, 1)}
PAIRS = (("default_this_tree", "default_parent"), ("asph_this_tree", "asph_parent"), ("anam_this_tree", "anam_parent"))
times = {k: [] for k in legs}
info = {}
for lf in legs.values():                      # warm-up
    lf.trace_ghosts(SPP, KEY); lf.synchronize()
for rnd in range(ROUNDS):
    order = ["decentred", "decentred_cleared"] if rnd % 2 == 0 else ["decentred_cleared", "decentred"]
    for a, b in PAIRS:
        order += [a, b] if rnd % 2 == 0 else [b, a]
    for name in order:
        lf = legs[name]
        for _ in range(FRAMES):
            lf.reset_counters()
            t0 = time.perf_counter()
            lf.trace_ghosts(SPP, KEY)
            lf.synchronize()
            times[name].append(round((time.perf_counter() - t0) * 1e3, 3))
        info[name] = dict(reason=lf.cull_reason(), counters=lf.counters(), executed_events=lf.executed_events())
    print("round", rnd, {k: v[-1] for k, v in times.items()}, flush=True)
out = dict(what=__doc__.split("\n    python3")[0], W=W, H=H, spp=SPP, rounds=ROUNDS, frames_per_round=FRAMES, sun=sun, legs={})
for name, ms in times.items():
    out["legs"][name] = dict(ms=ms, median_ms=round(statistics.median(ms), 3), min_ms=min(ms), max_ms=max(ms),
                             stdev_ms=round(statistics.pstdev(ms), 3), **info[name])
out["price_of_the_transform"] = round(out["legs"]["decentred"]["median_ms"] / out["legs"]["decentred_cleared"]["median_ms"], 4)
if args.compile_times:
    out["compile_times"] = json.loads(args.compile_times)
ok = True
for a, b in PAIRS:
    same_frame = bool(np.array_equal(legs[a].read_buffer(new.GHOST_BUFFER), legs[b].read_buffer(old.GHOST_BUFFER)))
    same_counters = info[a]["counters"] == info[b]["counters"] and info[a]["executed_events"] == info[b]["executed_events"]
    A, B = out["legs"][a], out["legs"][b]
    inside = bool(B["min_ms"] <= A["median_ms"] <= B["max_ms"])
    out[a + "_vs_parent"] = dict(frame_equal=same_frame, counters_equal=bool(same_counters), median_within_parents_min_max=inside)
    ok = ok and same_frame and same_counters and inside
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps({k: [v["median_ms"], v["min_ms"], v["max_ms"]] for k, v in out["legs"].items()}))
print(json.dumps({k: v for k, v in out.items() if k.endswith("_vs_parent") or k == "price_of_the_transform"}))
for lf in legs.values():
    lf.close()
sys.exit(0 if ok else 1)
