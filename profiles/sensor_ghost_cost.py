"""c3 frame (1920 x 1080, 256 spp, 3 wavelengths), one MI355X, one process, medians of 8 frames (4 rounds x 2) with min and max:
  default_this_tree / default_parent   the default launch (culled) of dgauss11.lens through this tree's library and through the
                      parent commit's, sensor ghosts OFF: the two legs take turns (they swap places every round) and must give
                      the parent's frame and counters bit for bit; the kernels are the same code, so this tree's median
                      must lie inside the parent's own min - max over its 8 frames (the script fails on either)
  sensor_add          dgauss11_sensor.lens, LF_SENSOR_GHOSTS_ADD: the default launch, then k_march_sensor over the ten sensor paths
  sensor_only         dgauss11_sensor.lens, LF_SENSOR_GHOSTS_ONLY: k_march_sensor alone
The sensor legs are numbers to record, not bars: the sensor paths are unculled and every one is marched alone from the sensor.
events_per_s of a sensor leg: the sensor paths' nominal events -- rays started times the path's 3 n - 2 i rows, what an
enumeration that kills no ray would execute -- over the "march_sensor" slot's time; the launch executes fewer (a wave stops
when no lane lives), so this is the rate a user can size a frame by, not the kernel's issue rate.
A frame = lf_trace_ghosts + synchronize.
    python3 profiles/sensor_ghost_cost.py --parent-lib PATH [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensor_ghost_cost.json"))
args = ap.parse_args()
new = load("lens_flare_amd")
old = load("lens_flare_amd_parent", os.path.abspath(args.parent_lib))
W, H, SPP, KEY = 1920, 1080, 256, 0x1e45f1a4e
ROUNDS, FRAMES = 4, 2
plain = new.load_lens_file("dgauss11.lens")
sens = new.load_lens_file("dgauss11_sensor.lens")
mask = new.load_aperture_png("pentbig500_14.png")
efl = new.paraxial_efl(plain)
sw = plain["sensor_width_mm"]
sun = [(0.521445 - 0.5) * sw / efl, (0.517156 - 0.5) * sw * H / W / efl, -1.0]


def context(pkg, lens, mode=None):
    lf = pkg.LensFlare(0)
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens({k: v for k, v in lens.items() if pkg is new or k != "sensor_reflectance"})
    lf.set_sun(sun, [1.0, 0.9, 0.5], 0.05)
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(2)
    if mode is not None:
        lf.set_sensor_ghosts(mode)
        lf.timing_enable(True)
    return lf


legs = {"default_this_tree": context(new, plain), "default_parent": context(old, plain),
        "sensor_add": context(new, sens, new.SENSOR_GHOSTS_ADD), "sensor_only": context(new, sens, new.SENSOR_GHOSTS_ONLY)}
PAIR = ("default_this_tree", "default_parent")
SENSOR = ("sensor_add", "sensor_only")
n_surf = int(sens["n"])
rows_per_sample = sum(3 * n_surf - 2 * i for i in range(n_surf) if i != int(sens["stop"]))
times = {k: [] for k in legs}
kernel_ms = {k: [] for k in SENSOR}
info = {}
for lf in legs.values():                      # warm-up
    lf.trace_ghosts(SPP, KEY); lf.synchronize()
for rnd in range(ROUNDS):
    order = list(PAIR) if rnd % 2 == 0 else list(PAIR[::-1])
    order += list(SENSOR)
    for name in order:
        lf = legs[name]
        for _ in range(FRAMES):
            lf.reset_counters()
            if name in SENSOR:
                lf.timing_reset()
            t0 = time.perf_counter()
            lf.trace_ghosts(SPP, KEY)
            lf.synchronize()
            times[name].append(round((time.perf_counter() - t0) * 1e3, 3))
            if name in SENSOR:
                kernel_ms[name].append(round(lf.timing_get("march_sensor")[1], 3))
        info[name] = dict(reason=lf.cull_reason(), counters=lf.counters(), executed_events=lf.executed_events())
        if name in SENSOR:
            info[name]["sensor_ghost_stats"] = lf.sensor_ghost_stats()
out = dict(what=__doc__.split("\n    python3")[0], W=W, H=H, spp=SPP, rounds=ROUNDS, frames_per_round=FRAMES, sun=sun,
           sensor_rows_per_sample_and_wavelength=rows_per_sample, legs={})
for name, ms in times.items():
    out["legs"][name] = dict(ms=ms, median_ms=round(statistics.median(ms), 3), min_ms=min(ms), max_ms=max(ms),
                             stdev_ms=round(statistics.pstdev(ms), 3), **info[name])
for name in SENSOR:
    k = kernel_ms[name]
    L = out["legs"][name]
    L["march_sensor_ms"] = dict(ms=k, median_ms=round(statistics.median(k), 3), min_ms=min(k), max_ms=max(k))
    nominal = W * H * SPP * 3 * rows_per_sample
    L["nominal_sensor_events"] = nominal
    L["events_per_s"] = round(nominal / (statistics.median(k) * 1e-3), 1)
a, b = PAIR
same_frame = bool(np.array_equal(legs[a].read_buffer(new.GHOST_BUFFER), legs[b].read_buffer(old.GHOST_BUFFER)))
same_counters = info[a]["counters"] == info[b]["counters"] and info[a]["executed_events"] == info[b]["executed_events"]
A, B = out["legs"][a], out["legs"][b]
out["default_vs_parent"] = dict(frame_equal=same_frame, counters_equal=bool(same_counters),
                                median_within_parents_min_max=bool(B["min_ms"] <= A["median_ms"] <= B["max_ms"]))
only = legs["sensor_only"].read_buffer(new.GHOST_BUFFER)
add = legs["sensor_add"].read_buffer(new.GHOST_BUFFER)
out["add_equals_default_plus_only"] = bool(np.array_equal(add, legs[a].read_buffer(new.GHOST_BUFFER) + only))
out["sensor_only_frame_max"] = float(only.max())
ok = same_frame and same_counters and out["default_vs_parent"]["median_within_parents_min_max"]
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps({k: [v["median_ms"], v["min_ms"], v["max_ms"]] for k, v in out["legs"].items()}))
print(json.dumps({k: out[k] for k in ("default_vs_parent", "add_equals_default_plus_only")}))
print(json.dumps({k: [out["legs"][k]["march_sensor_ms"]["median_ms"], out["legs"][k]["events_per_s"]] for k in SENSOR}))
for lf in legs.values():
    lf.close()
sys.exit(0 if ok else 1)
