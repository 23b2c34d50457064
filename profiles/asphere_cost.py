"""c3 frame (1920 x 1080, 256 spp, 46 paths x 3 wavelengths), one MI355X, one process, legs alternated (the two default legs swap places every round):
  tree         dgauss11.lens through the path tree (lf_set_march_culling(0))
  asph_force   the same lens through k_march_asph under lf_test_knob("asph_force"): every curved glass row on the Newton path
  asph_lens    dgauss11_asph.lens (two aspheric interfaces)
  default_this_tree / default_parent   the default launch (culled) of dgauss11.lens through this tree's library and through the
               parent commit's: the default path is the parent's
A frame = lf_trace_ghosts + synchronize.
    python3 profiles/asphere_cost.py --parent-lib PATH [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asphere_cost.json"))
args = ap.parse_args()
new = load("lens_flare_amd")
old = load("lens_flare_amd_parent", os.path.abspath(args.parent_lib))
W, H, SPP, KEY = 1920, 1080, 256, 0x1e45f1a4e
ROUNDS, FRAMES = 4, 2
plain = new.load_lens_file("dgauss11.lens")
asph = new.load_lens_file("dgauss11_asph.lens")
mask = new.load_aperture_png("pentbig500_14.png")
efl = new.paraxial_efl(plain)
sw = plain["sensor_width_mm"]
sun = [(0.521445 - 0.5) * sw / efl, (0.517156 - 0.5) * sw * H / W / efl, -1.0]


def context(pkg, lens, cull, force=0):
    lf = pkg.LensFlare(0)
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    lf.set_sun(sun, [1.0, 0.9, 0.5], 0.05)
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(cull)
    if force:
        lf.test_knob("asph_force", 1)
    return lf


legs = {"tree": context(new, plain, 0), "asph_force": context(new, plain, 0, 1), "asph_lens": context(new, asph, 1),
        "default_this_tree": context(new, plain, 2), "default_parent": context(old, plain, 2)}
times = {k: [] for k in legs}
info = {}
for lf in legs.values():                      # warm-up
    lf.trace_ghosts(SPP, KEY); lf.synchronize()
for rnd in range(ROUNDS):
    # (the frame after a leg of seconds runs ~1 ms slow whichever library it is: the two default legs take turns behind asph_lens)
    order = list(legs) if rnd % 2 == 0 else list(legs)[:3] + ["default_parent", "default_this_tree"]
    for name in order:
        lf = legs[name]
        for _ in range(FRAMES):
            lf.reset_counters()
            t0 = time.perf_counter()
            lf.trace_ghosts(SPP, KEY)
            lf.synchronize()
            times[name].append(round((time.perf_counter() - t0) * 1e3, 3))
        info[name] = dict(reason=lf.cull_reason(), counters=lf.counters(), executed_events=lf.executed_events())
out = dict(what=__doc__.split("\n    python3")[0], W=W, H=H, spp=SPP, rounds=ROUNDS, frames_per_round=FRAMES, sun=sun, legs={})
for name, ms in times.items():
    out["legs"][name] = dict(ms=ms, median_ms=round(statistics.median(ms), 3), min_ms=min(ms), max_ms=max(ms),
                             stdev_ms=round(statistics.pstdev(ms), 3), **info[name])
a = legs["default_this_tree"].read_buffer(new.GHOST_BUFFER)
b = legs["default_parent"].read_buffer(old.GHOST_BUFFER)
out["default_frame_equals_parent"] = bool(np.array_equal(a, b))
t = legs["tree"].read_buffer(new.GHOST_BUFFER); f = legs["asph_force"].read_buffer(new.GHOST_BUFFER)
lit = t > 2e-5
out["asph_force_vs_tree_max_rel"] = float(np.max(np.abs(f - t)[lit] / t[lit]))
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps({k: v["median_ms"] for k, v in out["legs"].items()}), out["default_frame_equals_parent"], out["asph_force_vs_tree_max_rel"])
for lf in legs.values():
    lf.close()
