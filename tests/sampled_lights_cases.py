"""The input sets of tests/test_gpu_sampled_lights.py (device = float64 oracle under the device's Philox counters,
1e-9 per channel) and of the CPU test that proves these sets honour their fragility caps on the oracle alone
(tests/test_oracle_vs_reference.py).  Everything here is seeded and evaluated by the oracle once per process.

A probe GROUP is a few hundred single rays through lf_scene_trace_ray ('trace': closest hit + the whole
radiance) or lf_scene_shade ('shade': one member of the integrator for an intersection given by the caller), all
under one scene / light list / ns_area_light, each with its own `seq`.  A FRAME goes through
lf_render_scene_term with the pixel-and-sample counters."""
import functools
import math

import numpy as np

from oracle import lfo

KEY = 20240611
TOL = 1e-9                 # |got - want| <= TOL |want| per channel: the bar of the project's delta-light frames
PROBE_CAP, PIXEL_CAP = 0.005, 0.01     # fragile share a group / a frame may leave out


def _quad(p0, p1, p2, p3, n, kind, rgb, normals=None):
    n4 = normals if normals is not None else [n, n, n, n]
    a = tuple(p0) + tuple(p1) + tuple(p2) + tuple(n4[0]) + tuple(n4[1]) + tuple(n4[2]) + (kind,) + tuple(rgb)
    b = tuple(p0) + tuple(p2) + tuple(p3) + tuple(n4[0]) + tuple(n4[2]) + tuple(n4[3]) + (kind,) + tuple(rgb)
    return [a, b]


def _cube(x0, x1, y0, y1, z0, z1, rgb):
    c = lambda x, y, z: (x, y, z)  # noqa: E731
    f = []
    f += _quad(c(x0, y0, z1), c(x1, y0, z1), c(x1, y1, z1), c(x0, y1, z1), (0, 0, 1), "d", rgb)
    f += _quad(c(x1, y0, z0), c(x0, y0, z0), c(x0, y1, z0), c(x1, y1, z0), (0, 0, -1), "d", rgb)
    f += _quad(c(x1, y0, z1), c(x1, y0, z0), c(x1, y1, z0), c(x1, y1, z1), (1, 0, 0), "d", rgb)
    f += _quad(c(x0, y0, z0), c(x0, y0, z1), c(x0, y1, z1), c(x0, y1, z0), (-1, 0, 0), "d", rgb)
    f += _quad(c(x0, y1, z1), c(x1, y1, z1), c(x1, y1, z0), c(x0, y1, z0), (0, 1, 0), "d", rgb)
    f += _quad(c(x0, y0, z0), c(x1, y0, z0), c(x1, y0, z1), c(x0, y0, z1), (0, -1, 0), "d", rgb)
    return f


# a yard open to the sky: a floor with bent vertex normals, a box of 12 triangles, three spheres (one of them a black
# stub BSDF) and one emissive quad overhead
_bent = [(0.08, 1.0, 0.0), (0.0, 1.0, 0.06), (-0.05, 1.0, 0.0), (0.0, 1.0, -0.07)]
TRIS = (_quad((-3, 0, 3), (3, 0, 3), (3, 0, -3), (-3, 0, -3), (0, 1, 0), "d", (0.6, 0.55, 0.5), normals=_bent)
        + _cube(0.3, 0.9, 0.0, 0.6, -0.9, -0.3, (0.3, 0.6, 0.4))
        + _quad((-0.3, 1.6, -0.3), (0.3, 1.6, -0.3), (0.3, 1.6, 0.3), (-0.3, 1.6, 0.3), (0, -1, 0), "e", (6.0, 5.0, 4.0)))
SPHERES = [(-0.5, 0.35, 0.1, 0.35, "d", 0.8, 0.3, 0.3), (0.2, 0.2, 0.6, 0.2, "d", 0.3, 0.4, 0.8),
           (-0.9, 0.9, -0.6, 0.25, "m", 0.0, 0.0, 0.0)]

# The frames see the spheres as emitters (and one black stub): a diffuse sphere's limb and its terminators are where a
# sample's radiance is small and moves by more than 1e-9 relative under the 1e-12 shifts -- at 64 samples a pixel that
# is several fragile pixels per frame, above the cap.  Diffuse spheres are shaded by the probe groups above; here the
# spheres still occlude, cast shadows and are what the -H directions find.
FRAME_SPHERES = [(-0.5, 0.35, 0.1, 0.35, "e", 0.5, 0.2, 0.2), (0.2, 0.2, 0.6, 0.2, "e", 0.1, 0.2, 0.5),
                 (-0.9, 0.9, -0.6, 0.25, "m", 0.0, 0.0, 0.0)]


def _unit(v):
    v = np.asarray(v, float)
    return (v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])).tolist()


SUN = [0.0, 0.9, 0.85, 0.7] + _unit([0.3, 0.8, 0.5]) + [0.0] * 9
POINT = [1.0, 3.0, 3.0, 3.0, 1.2, 1.4, 1.0] + [0.0] * 9
# pos, dir, dim_x, dim_y: straight down from under the emissive quad (the plane y = 1.5)
AREA = [3.0, 12.0, 11.0, 9.0, 0.0, 1.5, 0.0, 0.0, -1.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.5]
# dim_x . dim_y != 0 and neither is a unit vector: area = |dim_x| |dim_y| (light.cpp:80), not |dim_x x dim_y|
AREA_SKEW = [3.0, 7.0, 8.0, 10.0, -1.2, 1.0, 0.8] + _unit([0.5, -0.7, -0.4]) + [0.6, 0.2, 0.1, 0.3, 0.1, -0.5]
HEMI = [2.0, 0.6, 0.7, 0.9] + [0.0] * 12
ENV = [4.0] + [0.0] * 15


def env_map(w, h, kind="smooth", seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "random":
        return np.ascontiguousarray(rng.uniform(0.05, 2.0, (h, w, 3)))
    if kind == "sparse":           # one bright texel, every other row nothing but zeros
        m = np.zeros((h, w, 3))
        m[h // 2, (2 * w) // 3] = (30.0, 26.0, 18.0)
        return m
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    th = (j + 0.5) / h
    m = np.stack([0.25 + 0.3 * th, 0.35 + 0.3 * th, 0.7 - 0.2 * th], -1) * (1.0 + 0.25 * np.sin(6 * np.pi * i / w)[..., None])
    patch = np.exp(-(((i - 0.7 * w) / (0.05 * w)) ** 2 + ((j - 0.28 * h) / (0.08 * h)) ** 2))
    return np.ascontiguousarray(m + patch[..., None] * np.array([40.0, 34.0, 22.0]))


def _trace_rays(rng, n, sky=0.3):
    """origins above the yard; most rays aim at the objects, the rest anywhere (many of those leave for the sky)"""
    o = np.stack([rng.uniform(-2, 2, n), rng.uniform(0.3, 2.2, n), rng.uniform(-2, 2, n)], -1)
    tgt = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-0.2, 0.8, n), rng.uniform(-1.5, 1.5, n)], -1)
    d = tgt - o
    free = rng.uniform(size=n) < sky
    d[free] = rng.normal(size=(int(free.sum()), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d, np.zeros((n, 1)), np.full((n, 1), np.inf)], 1)


def _shade_inputs(rng, n, y_range=(0.05, 1.3), normals="any", kinds=(0, 1, 2)):
    """intersections `the host found itself': a ray, t, a normal and a material, the hit point above the floor"""
    hit = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(*y_range, n), rng.uniform(-1.5, 1.5, n)], -1)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = rng.uniform(0.5, 3.0, n)
    o = hit - d * t[:, None]
    if normals == "any":
        nn = rng.normal(size=(n, 3))
        nn[:, 1] = np.abs(nn[:, 1]) + 0.2           # mostly facing up, where the light is
        nn *= rng.uniform(0.5, 2.0, (n, 1))         # (make_coord_space normalises)
    else:
        nn = np.tile(np.asarray(normals, float), (n // len(normals) + 1, 1))[:n]
    kind = np.asarray(kinds)[rng.integers(0, len(kinds), n)].astype(float)
    mats = np.concatenate([kind[:, None], rng.uniform(0.1, 0.9, (n, 3))], 1)
    rays = np.concatenate([o, d, np.zeros((n, 1)), np.full((n, 1), np.inf)], 1)
    return rays, t, nn, mats


def _group(name, mode, rows, seed, n=240, ns=4, hemisphere=False, env=None, what=3, **kw):
    rng = np.random.default_rng(seed)
    g = dict(name=name, mode=mode, rows=rows, ns=ns, hemisphere=hemisphere, env=env, what=what,
             spheres=FRAME_SPHERES if name.startswith("H_") else SPHERES,   # (-H finds emitters: give it some)
             seq=(np.uint64(seed) << np.uint64(20)) + np.arange(n, dtype=np.uint64) * np.uint64(7919) + np.uint64(1))
    if mode == "trace":
        g["rays"] = _trace_rays(rng, n, **kw)
    else:
        g["rays"], g["t"], g["n"], g["mats"] = _shade_inputs(rng, n, **kw)
    return g


# seq values whose Philox block (key KEY, light 0, sample 0) holds a word that random_uniform clamps: word 0 < 430 (->
# 1e-7), word 1 < 430, word 0 > 4294967252 (-> 0.99999999), word 1 > 4294967252; found by a search over seq = 0, 1, ...
CLAMPED_SEQ = [(2085100, 0, "lo"), (20446373, 0, "lo"), (6806762, 1, "lo"), (19271136, 1, "lo"),
               (49895159, 0, "hi"), (111975003, 0, "hi"), (226241802, 1, "hi"), (284655401, 1, "hi")]


@functools.lru_cache(maxsize=None)
def groups():
    mixed = [SUN, AREA, POINT, AREA_SKEW]        # the sampled lights at indices 1 and 3; total_samples = 2 + 2 ns
    G = []
    # ---- area lights
    for ns in (1, 2, 5, 16):
        G.append(_group(f"area_mixed_ns{ns}", "trace", mixed, 11 + ns, ns=ns))
    G.append(_group("area_skew_alone", "trace", [AREA_SKEW], 31))
    G.append(_group("area_shade_materials", "shade", mixed, 32, what=3))
    G.append(_group("area_shade_one_bounce", "shade", mixed, 33, what=1))
    G.append(_group("zero_bounce", "shade", mixed, 34, what=0))
    # hit points in front of (below), behind (above) and exactly in the plane y = 1.5 of AREA: cos_l <, >, = 0
    side = _group("area_sides", "shade", mixed, 35, n=300, kinds=(0, 2))
    rng = np.random.default_rng(36)
    k = np.arange(300) % 3
    hit_y = np.where(k == 0, rng.uniform(0.2, 1.3, 300), np.where(k == 1, rng.uniform(1.7, 2.2, 300), 1.5))
    o, d, t = side["rays"][:, 0:3], side["rays"][:, 3:6], side["t"]
    d[k == 2, 1] = 0.0                                # o.y + 0 t = 1.5 exactly
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    hit = o + d * t[:, None]
    o[:, 1] += hit_y - hit[:, 1]
    o[k == 2, 1] = 1.5
    # (in the plane the area light adds exactly 0 and +-1e-12 under the shifts: the normals there face the sun, so that
    # the sum they are compared against is not 0)
    side["n"][k == 2] = np.asarray(SUN[4:7]) + rng.uniform(-0.3, 0.3, (100, 3))
    side["in_plane"] = k == 2
    G.append(side)
    # ---- hemisphere light: normals up, down and sideways (the wo.z < 0 skip, the axes of sampleToWorld)
    G.append(_group("hemi_trace", "trace", [HEMI], 41))
    G.append(_group("hemi_with_sun", "trace", [SUN, HEMI], 42, ns=3))
    G.append(_group("hemi_normals", "shade", [HEMI], 43, normals=[(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1),
                                                                 (0, 0, -1), (0.3, 0.2, -0.9)], kinds=(0, 2)))
    # ---- environment light
    for nm, w, h, kind in (("2x2", 2, 2, "random"), ("5x3", 5, 3, "random"), ("64x32", 64, 32, "smooth"),
                           ("sparse", 6, 5, "sparse")):
        # (2 x 2: the two rows are theta = 0, where the pdf is infinite, and pi / 2, a horizontal wi whose cosine against an
        # axis-aligned face is 6e-17 either way -- shaded with normals off the axes instead of traced)
        if w == 2:
            G.append(_group(f"env_{nm}", "shade", [ENV], 50 + w, env=env_map(w, h, kind), kinds=(0, 2)))
        else:
            G.append(_group(f"env_{nm}", "trace", [ENV], 50 + w, env=env_map(w, h, kind), sky=0.4))
    G.append(_group("env_with_sun", "trace", [SUN, ENV], 58, env=env_map(5, 3, "random"), ns=2))
    # draws that random_uniform clamps at 1e-7 and 0.99999999 (the first and last bins; row 0 has sin(theta) = 0)
    cl = _group("env_clamped_draws", "shade", [ENV], 59, n=len(CLAMPED_SEQ) * 4, ns=1, env=env_map(5, 3, "random"),
                normals=[(0, 1, 0), (0, -1, 0), (1, 0.2, 0), (-0.3, 0.1, -1)], kinds=(0,))
    cl["seq"] = np.repeat(np.array([s for s, _, _ in CLAMPED_SEQ], np.uint64), 4)
    G.append(cl)
    # miss rays for sample_dir: both poles and either side of the phi seam (atan2(-z, x) = +-pi: x < 0, z = +-0)
    ms = _group("env_sample_dir", "trace", [ENV], 60, n=64, env=env_map(5, 3, "random"))
    rng = np.random.default_rng(61)
    dirs = [(0, 1, 0), (0, -1, 0), (1e-9, 1, 0), (0, 1, -1e-9), (-1e-7, -1, 1e-8), (-1, 0.3, 0.0), (-1, 0.3, -0.0),
            (-1, 0.3, 1e-12), (-1, 0.3, -1e-12), (-1, 0.5, 1e-3), (-1, 0.5, -1e-3), (1, 0.4, 0.0), (1, 0.4, 1e-9)]
    for q, dd in enumerate(dirs):
        # downwards from beside the floor, upwards from above everything: nothing is hit
        ms["rays"][q, 0:3] = (3.5, 1.0, 3.5) if dd[1] < 0 else (rng.uniform(-1, 1), 2.5, rng.uniform(-1, 1))
        ms["rays"][q, 3:6] = dd
    ms["rays"][len(dirs):, 0:3] = (0.0, 2.5, 0.0)            # the rest: anywhere into the upper half
    ms["rays"][len(dirs):, 4] = np.abs(ms["rays"][len(dirs):, 4])
    G.append(ms)
    # ---- the -H estimator: lights.size() * ns_area_light directions, emission of kind-1 surfaces only
    G.append(_group("H_one_light", "trace", [AREA], 71, hemisphere=True, sky=0.1))
    G.append(_group("H_three_lights", "trace", [SUN, AREA, POINT], 72, hemisphere=True, ns=3, sky=0.1))
    G.append(_group("H_shade_by_name", "shade", [SUN, AREA], 73, what=2, y_range=(0.05, 1.5)))
    G.append(_group("H_no_lights", "trace", [], 74, n=60, hemisphere=True, sky=0.0))
    for g in G:
        desc = lfo.scene_desc(g["spheres"], TRIS, g["rows"], g["ns"], g["hemisphere"], g["env"])
        ctr = lfo.seq_counter(g["seq"])
        if g["mode"] == "trace":
            g["want"], g["fragile"] = lfo.scene_rays(desc, g["rays"], ctr, KEY)
        else:
            g["want"], g["fragile"] = lfo.scene_shade(desc, g["what"], g["rays"], g["t"], g["n"], g["mats"], ctr, KEY)
    return G


def look_at(pos, target):
    f = np.array(target, float) - np.array(pos, float)
    f /= np.linalg.norm(f)
    r = np.cross(f, [0, 1, 0]); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    return np.stack([r, u, -f], axis=1).reshape(-1)


CAM_POS = [0.4, 1.1, 3.2]
CAM_C2W = look_at(CAM_POS, [0.0, 0.45, 0.0])


def _fov(W, H, hf=48.0):
    return hf, 2 * math.degrees(math.atan(math.tan(math.radians(hf) / 2) * H / W))


FRAMES = [
    dict(name="area_24x16", W=24, H=16, rows=[SUN, AREA, POINT, AREA_SKEW], ns=2, hemisphere=False, env=None, spb=32, key=9001),
    dict(name="hemi_21x13", W=21, H=13, rows=[HEMI, POINT], ns=2, hemisphere=False, env=None, spb=32, key=9002),
    dict(name="env_21x13", W=21, H=13, rows=[SUN, ENV], ns=3, hemisphere=False, env=("smooth", 15, 7), spb=32, key=9003),
    dict(name="H_24x16", W=24, H=16, rows=[AREA], ns=2, hemisphere=True, env=None, spb=32, key=9004),
    dict(name="area_21x13_one_batch", W=21, H=13, rows=[AREA, POINT], ns=2, hemisphere=False, env=("random", 5, 3),
         spb=100, key=9005),
]
NS_AA, MAX_TOL = 64, 0.05


@functools.lru_cache(maxsize=None)
def frames():
    out = []
    for f in FRAMES:
        f = dict(f)
        f["env_map"] = env_map(f["env"][1], f["env"][2], f["env"][0]) if f["env"] else None
        f["hfov"], f["vfov"] = _fov(f["W"], f["H"])
        desc = lfo.scene_desc(FRAME_SPHERES, TRIS, f["rows"], f["ns"], f["hemisphere"], f["env_map"])
        f["want"], f["flags"], f["n_samples"] = lfo.scene_frame(desc, f["W"], f["H"], NS_AA, CAM_C2W, CAM_POS, f["hfov"],
                                                                f["vfov"], key=f["key"], samples_per_batch=f["spb"],
                                                                max_tol=MAX_TOL)
        out.append(f)
    return out
