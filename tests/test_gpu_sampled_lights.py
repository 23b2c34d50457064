"""The scene term's SAMPLED lights on the device, draw for draw against float64: AreaLight,
InfiniteHemisphereLight, the importance-sampled EnvironmentLight and the -H uniform-hemisphere estimator
(shade_hit<true> in csrc/lf_scene.hip) draw every sample from Philox4x32-10 with an explicit counter (DESIGN.md
section 8), so the serial float64 restatement oracle/lf_scene_oracle.c can consume exactly the same draws.  That
restatement is pinned to the real reference from the reference's own MT19937 stream
(tests/test_oracle_vs_reference.py), which makes the chain reference = oracle = device, each to rounding:

    |device - oracle| <= 1e-9 |oracle|   per channel, per probe and per pixel

-- the bar of the project's delta-light frames; the expected deviation is libm's, ~1e-13.  A probe or pixel the oracle
calls fragile (its value hangs on a discrete decision that one ulp can flip: sampled_lights_cases.py) is left out,
at most 0.5 % of a group and 1 % of a frame; the CPU suite proves those caps on the oracle alone.  The statistical
tests (test_gpu_area_lights.py, test_gpu_env_light.py) stay: they compare with the reference's own renders."""
import numpy as np
import pytest

import sampled_lights_cases as slc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="module")
def lf(pkg):
    ctx = pkg.LensFlare(0)
    yield ctx
    ctx.close()


def _install(lf, spheres, rows, ns, hemisphere, env, key):
    lf.set_scene(spheres, slc.TRIS, [])
    lf.set_environment_map(env)
    lf.set_scene_lights(np.asarray(rows, np.float64).reshape(-1, 16))
    lf.set_light_samples(ns)
    lf.set_direct_hemisphere_sample(hemisphere)
    lf.set_jitter_counter(key)


def _deviation(got, want):
    """largest |got - want| / |want| over the channels; NaN where both are NaN counts as equal, 0 == 0 as equal"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        dev = np.abs(got - want) / np.abs(want)
    dev[(got == want) | both_nan] = 0.0
    dev[np.isnan(dev)] = np.inf            # NaN on one side only
    return dev


def _check(name, dev, fragile, cap, what):
    n, k = len(fragile), int(fragile.sum())
    worst = float(dev[~fragile].max()) if k < n else 0.0
    print(f"{name}: {n} {what}, {k} fragile, largest deviation {worst:.3e}")
    assert k <= cap * n, (name, k, n)
    assert worst <= slc.TOL, (name, worst, int(np.argmax(np.where(fragile, 0.0, dev))))


GROUPS = [g["name"] for g in slc.groups()]


@pytest.mark.parametrize("name", GROUPS)
def test_single_ray_probes_equal_the_oracle_draw_for_draw(lf, name):
    """lf_scene_trace_ray (hit, t, normal AND the radiance) and lf_scene_shade (what = 0 .. 3) against the oracle under
    the probe counter (seq low word, seq high word | 2^31); the groups: sampled_lights_cases.groups()."""
    g = next(g for g in slc.groups() if g["name"] == name)
    _install(lf, g["spheres"], g["rows"], g["ns"], g["hemisphere"], g["env"], slc.KEY)
    n = len(g["seq"])
    if g["mode"] == "trace":
        got = np.zeros((n, 8))
        for i in range(n):
            r = g["rays"][i]
            o = lf.scene_trace_ray(r[0:3], r[3:6], r[6], r[7], seq=int(g["seq"][i]))
            got[i] = [float(o["hit"]), o["t"], *o["n"], *o["radiance"]]
        sure = ~g["fragile"]
        assert np.array_equal(got[sure, 0], g["want"][sure, 0]), name          # the same rays hit
        dev = _deviation(got[:, 1:], g["want"][:, 1:])
    else:
        got = np.zeros((n, 3))
        for i in range(n):
            r = g["rays"][i]
            got[i] = lf.scene_shade(g["what"], r[0:3], r[3:6], g["t"][i], g["n"][i], g["mats"][i], r[6], r[7],
                                    seq=int(g["seq"][i]))
        dev = _deviation(got, g["want"])
    _check(name, dev.max(axis=1), g["fragile"], slc.PROBE_CAP, "probes")


def _render(pkg, f, band=None, interleave=None, ns_aa=slc.NS_AA):
    ctx = pkg.LensFlare(0)
    try:
        ctx.set_frame(f["W"], f["H"])
        ctx.set_params(ns_aa, 25.0, 1.0)
        ctx.set_sampling(f["spb"], slc.MAX_TOL, 0.01, 100.0)
        ctx.set_camera(slc.CAM_C2W, slc.CAM_POS, f["hfov"], f["vfov"])
        _install(ctx, slc.FRAME_SPHERES, f["rows"], f["ns"], f["hemisphere"], f["env_map"], f["key"])
        if band:
            ctx.set_band(*band)
        if interleave:
            ctx.set_row_interleave(*interleave)
        ctx.render_scene_term()
        return ctx.read_buffer(pkg.SCENE_BUFFER)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", [f["name"] for f in slc.FRAMES])
def test_frames_equal_the_oracle_draw_for_draw(pkg, name):
    """lf_render_scene_term, pinhole camera, counter jitter: every pixel of a 24 x 16 / 21 x 13 frame (a wave is an
    8 x 8 tile: partial tiles on both axes) at ns_aa 64 with batches of 32 and tolerance 0.05 -- pixels stop at 32, at
    64 or run out -- and once with samples_per_batch > ns_aa; each of the four estimators once."""
    f = next(f for f in slc.frames() if f["name"] == name)
    got = _render(pkg, f)
    frag = (f["flags"] != 0).reshape(-1)
    dev = _deviation(got, f["want"]).reshape(-1, 3).max(axis=1)
    _check(name, dev, frag, slc.PIXEL_CAP, "pixels")


def test_band_split_and_row_interleave_of_an_odd_frame(pkg):
    """the 21 x 13 environment-light frame in two bands that cut a tile row, and dealt to three ranks by rows: every
    part writes its own rows only, and together they are the oracle's frame"""
    f = next(f for f in slc.frames() if f["name"] == "env_21x13")
    frag = (f["flags"] != 0).reshape(-1)
    for label, parts in (("bands", [dict(band=(0, 5)), dict(band=(5, 13))]),
                         ("interleave", [dict(interleave=(k, 3)) for k in range(3)])):
        total = np.zeros_like(f["want"])
        owned = np.zeros(f["H"], int)
        for p in parts:
            part = _render(pkg, f, **p)
            owned += (part != 0).any(axis=(1, 2))
            total += part
        assert (owned == 1).all(), (label, owned)       # (every row of this frame is lit)
        dev = _deviation(total, f["want"]).reshape(-1, 3).max(axis=1)
        _check(f"env_21x13 {label}", dev, frag, slc.PIXEL_CAP, "pixels")
