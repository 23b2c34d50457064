"""The float64 tracer (oracle/lf_geo_f64.c) under a LIGHT LIST (lfo.g64_set_lights, g64_trace(lights=...)), CPU only: what makes
it a reference for the ghosts of point lights, area lights and several lights (tests/test_gpu_lights_f64.py).  The tracer is
"parity unpinned" by construction, so it is anchored here before it judges anything: (1) one directional light through the list
IS the sun of the sun_* arguments, bit for bit, and without a list the tracer is what it was; (2) the primary image of a lamp
and of a rectangle is the sum over the tracer's own exit rays, the light test written again in numpy (uv64 of
tests/test_area_ghosts_cpu.py, a numpy lobe); (3) a lamp far away is the directional light within its parallax; (4) lights
add, a rectangle is its two halves, the whole sky lights every ray; (5) the rectangles' edge band stays the exception on every
frame tests/test_gpu_lights_f64.py uses.

THE FRAMES of the GPU tests are defined here (FRAMES), so that (5) measures exactly what those tests render."""
import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo
from test_area_ghosts_cpu import RECTS, AREA, geom_of, uv64

DIRECTIONAL, POINT = 0, 1
MASK = "pentbig500_14.png"
RAD, RAD2, RAD3 = [1.0, 0.5, 0.25], [0.5, 1.0, 0.125], [0.25, 0.125, 1.0]          # powers of two: weight x radiance is exact
# (kind, geometry, radiance, angular radius), as tests/test_gpu_area_ghosts.py installs them
SUN = (DIRECTIONAL, [0.012, 0.004, -1.0], RAD2, 0.03)
SUN_B = (DIRECTIONAL, [0.0, 0.01, -1.0], RAD, 0.02)          # overlaps SUN: 0.0134 rad apart, lobes of 0.03 and 0.02
LAMP = (POINT, [1.5, -1.0, -90.0], RAD3, 0.05)
PANEL = (AREA, geom_of(RECTS[0]), RAD, 0.0)
TILTED = (AREA, geom_of(RECTS[1]), RAD, 0.0)                  # the 12 x 8 mm tilted parallelogram at 90 mm: its outline crosses the frame
BEHIND = (AREA, geom_of(RECTS[1], (0.0, 0.0, -1.0)), RAD, 0.0)
SKY = (AREA, geom_of(RECTS[3]), RAD, 0.0)
OFF_AXIS = np.array([0.012, -0.007, -1.0])


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def crop(lens, W, pitch_of=1920):
    """the sensor crop of tests/test_gpu_area_ghosts.py: W pixels at the pitch of a 36 mm sensor of `pitch_of` pixels"""
    c = dict(lens)
    c["sensor_width_mm"] = 36.0 * W / pitch_of
    return c


def r_f_of(lens):
    h0, R0 = float(lens["semi_aperture"][0]), abs(float(lens["radius"][0]))
    return float(np.hypot(h0, R0 - np.sqrt(R0 * R0 - h0 * h0)))


def lamp_off_axis(lens):
    """a lamp 4.6 r_f from the front vertex, off the axis (the near limit is 4 r_f)"""
    return (POINT, (4.6 * r_f_of(lens) * OFF_AXIS / np.linalg.norm(OFF_AXIS)).astype(np.float32), RAD, 0.03)


# name -> (lens file, W, H, key, lights); every frame is the 64-pixel crop of the 36 mm / 1920 sensor, primary + all 45 pairs
FRAMES = {
    "lamp_near": ("dgauss11.lens", 64, 48, 0x64A1, lambda lens: [LAMP]),
    "lamp_off_axis": ("dgauss11.lens", 64, 48, 0x64A2, lambda lens: [lamp_off_axis(lens)]),
    "tilted": ("dgauss11.lens", 64, 48, 0x64A3, lambda lens: [TILTED]),
    "behind": ("dgauss11.lens", 64, 48, 0x64A4, lambda lens: [BEHIND]),
    "mixed": ("dgauss11.lens", 64, 48, 0x64A5, lambda lens: [SUN, LAMP, PANEL]),
    "two_suns": ("dgauss11.lens", 64, 48, 0x64A6, lambda lens: [SUN, SUN_B]),
    "coated": ("dgauss11_coated.lens", 64, 48, 0x64A7, lambda lens: [PANEL, SUN]),
    "bilinear": ("dgauss11.lens", 64, 48, 0x64A8, lambda lens: [LAMP]),
}


def frame_of(pkg, name):
    """-> (lens, W, H, key, lights) of FRAMES[name]"""
    fname, W, H, key, lights = FRAMES[name]
    lens = crop(pkg.load_lens_file(fname), W)
    return lens, W, H, key, lights(lens)


@pytest.fixture(scope="module")
def mask():
    return load_texels(MASK)


def _trace(lens, W, H, spp, key, mask, lights, pairs=None, include_primary=True):
    # (the sun_* arguments are ignored under a list: a black sun straight ahead)
    return lfo.g64_trace(lens, W, H, 0, H, spp, key, pairs, include_primary, mask, [0.0, 0.0, -1.0], [0.0, 0.0, 0.0], 0.05,
                         lights=lights)


# ---- 1. the sun through the list ----------------------------------------------------------------------------------------------
def test_one_directional_light_through_the_list_is_the_sun_bit_for_bit(mask):
    lens = _pkg().load_lens_file("dgauss11.lens")
    W, H, spp, key = 32, 24, 16, 0x5117
    sun, rad, alpha = [0.03, 0.02, -1.0], [1.0, 0.9, 0.5], 0.05
    img, frag, c = lfo.g64_trace(lens, W, H, 0, H, spp, key, None, True, mask, sun, rad, alpha)
    assert img.max() > 0 and frag.max() > 0 and c["rays_hit_light"] > 0 and c["light_edge_pairs"] == 0
    # without a list the tracer is the parent commit's: the image sum of this frame as that commit's tracer gives it
    assert float(img.sum()).hex() == "0x1.eb353ddc402dbp-5", float(img.sum()).hex()
    assert float(frag.sum()).hex() == "0x1.845be3a081deap-11" and (c["rays_hit_light"], c["rays_fragile"]) == (6238, 7905)
    # the list takes the values as the device stores them: the direction lf_set_sun has normalised and narrowed
    L = lfo.g64_lens(lens, sun, rad, alpha)
    stored = [(DIRECTIONAL, list(L.sun_dir), list(L.sun_radiance), L.sun_angular_radius)]
    img2, frag2, c2 = _trace(lens, W, H, spp, key, mask, stored)
    assert np.array_equal(img, img2) and np.array_equal(frag, frag2)
    assert c2 == c
    # ... and the list is cleared again afterwards
    img3, _, c3 = lfo.g64_trace(lens, W, H, 0, H, spp, key, None, True, mask, sun, rad, alpha)
    assert np.array_equal(img, img3) and c3 == c


def test_the_c_call_still_fills_eight_counters_only(mask):
    """a binding written before the light list hands g64_trace an array of EIGHT counters: the C call must write no ninth slot
    (the ninth counter has its own getter), with and without a list"""
    import ctypes as C
    lens = crop(_pkg().load_lens_file("dgauss11.lens"), 64)
    L = lfo.g64_lens(lens)
    W, H, spp = 16, 8, 4
    pairs = np.ascontiguousarray(lfo.all_pairs(lens, True), np.int32)
    m = np.ascontiguousarray(mask, np.float32)
    image, frag = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    key = (C.c_uint32 * 2)(7, 0)
    guard = 0xA5A5A5A5A5A5A5A5
    for lights in (None, [TILTED]):
        cnt = (C.c_uint64 * 12)(*([guard] * 12))
        lfo.g64_set_lights(lights)
        try:
            lfo.lib().g64_trace(C.byref(L), W, H, 0, H, spp, key, 6, pairs.ctypes.data_as(C.POINTER(C.c_int)), len(pairs),
                                m.ctypes.data_as(C.POINTER(C.c_float)), m.shape[1], m.shape[0],
                                image.ctypes.data_as(C.POINTER(C.c_double)), frag.ctypes.data_as(C.POINTER(C.c_double)), cnt, 2)
        finally:
            lfo.g64_set_lights(None)
        assert cnt[0] == W * H * spp * len(pairs) * 3 and all(v != guard for v in cnt[:8])
        assert all(v == guard for v in cnt[8:]), [hex(v) for v in cnt[8:]]
    lfo.lib().g64_light_edge_pairs.restype = C.c_uint64
    assert lfo.lib().g64_light_edge_pairs() > 0          # (the tilted rectangle's band, read beside the array)


# ---- 2. the primary image, independently in numpy ---------------------------------------------------------------------------------
def _lobe_numpy(P, d, light):
    kind, g, _, alpha = light
    g = np.asarray(g, np.float32).astype(np.float64)
    s = g[None, :3] - P if kind == POINT else np.broadcast_to(g[:3], P.shape)
    s = s / np.linalg.norm(s, axis=1)[:, None]
    q = (1.0 - (d * s).sum(1)) / (1.0 - np.cos(float(np.float32(alpha))))
    return np.where(q < 1.0, (1.0 - q) ** 2, 0.0)


def _band_numpy(g, P, d):
    """(inside, in the edge band) of rectangle g for the float64 rays (P, unit d): uv64's (u, v), the band as lf_geo_f64.c
    states it -- within eps_exit + t eps_dir + eps_test |P - C| millimetres of an edge segment, in the rectangle's plane"""
    eps_exit, eps_dir, eps_test = lfo.g64_light_eps()
    g = np.asarray(g, np.float32).astype(np.float64)
    C, e1, e2 = g[0:3], g[6:9], g[9:12]
    # (uv64 takes float32 rays; these are float64, so its expressions again on them)
    n = np.cross(e1, e2)
    t = ((C[None, :] - P) @ n) / (d @ n)
    w = P + t[:, None] * d - C[None, :]
    G = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
    u, v = np.linalg.solve(G, np.stack([w @ e1, w @ e2]))
    dirn = g[3:6] / np.linalg.norm(g[3:6])
    facing = d @ dirn
    assert (np.abs(facing) > 1e-3).all() and (t > 0).all()          # (no ray of these frames is near the plane's horizon)
    area = np.linalg.norm(n)
    du, dv = (np.abs(u) - 0.5) * area / np.linalg.norm(e2), (np.abs(v) - 0.5) * area / np.linalg.norm(e1)
    eps = eps_exit + t * eps_dir + eps_test * np.linalg.norm(P - C[None, :], axis=1)
    inside = (np.abs(u) <= 0.5) & (np.abs(v) <= 0.5) & (facing < 0)
    edge = (((np.abs(du) < eps) & (dv < eps)) | ((np.abs(dv) < eps) & (du < eps))) & (facing < 0)
    return inside, edge


def test_uv_of_the_band_is_uv64():
    """_band_numpy's (u, v) on float64 rays is uv64's on the same rays rounded to float32 inputs (it rounds nothing else)"""
    rng = np.random.default_rng(0x64B0)
    P = np.concatenate([rng.uniform(-10, 10, (256, 2)), rng.uniform(0, 2, (256, 1))], 1).astype(np.float32).astype(np.float64)
    aim = np.asarray(RECTS[1][0]) + rng.uniform(-0.7, 0.7, (256, 1)) * np.asarray(RECTS[1][1]) + rng.uniform(-0.7, 0.7, (256, 1)) * np.asarray(RECTS[1][2])
    d = (aim - P).astype(np.float32).astype(np.float64)
    u, v, t, cd = uv64(geom_of(RECTS[1]), np.concatenate([P, d], 1).astype(np.float32))
    inside, _ = _band_numpy(geom_of(RECTS[1]), P, d / np.linalg.norm(d, axis=1)[:, None])
    want = (np.abs(u) <= 0.5) & (np.abs(v) <= 0.5) & (t > 0) & (cd < 0)
    assert np.array_equal(inside, want) and 40 < want.sum() < 216


@pytest.mark.parametrize("name", ["lamp", "tilted"])
def test_primary_image_is_the_sum_over_the_tracers_exit_rays(mask, name):
    W, H, spp, key = 64, 48, 64, 0x64B1
    lens = crop(_pkg().load_lens_file("dgauss11.lens"), W)
    light = LAMP if name == "lamp" else TILTED
    img, frag, c = _trace(lens, W, H, spp, key, mask, [light], pairs=[], include_primary=True)
    want, wfrag = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    n_edge = 0
    for lam in range(3):          # (three wavelengths, lambda_rgb the identity: wavelength l is channel l)
        smp = lfo.g64_lens_samples(lens, W, H, spp, key, lam, np.arange(W * H), mask).reshape(W * H * spp, 10)
        P, d, w, w_pot, fragile = smp[:, 0:3], smp[:, 3:6], smp[:, 6], smp[:, 7], smp[:, 8]
        assert (fragile < 2).all()
        if light[0] == AREA:
            inside, edge = _band_numpy(light[1], P, d)
            shade, reach = inside.astype(np.float64), (inside | edge).astype(np.float64)
            own = np.where((fragile == 0) & edge, w, 0.0)          # a firm ray in the band: its weight, whichever way it fell
            n_edge += int(((w > 0) & edge).sum())
        else:
            shade = reach = _lobe_numpy(P, d, light)
            own = 0.0
        rad = float(np.float32(light[2][lam]))
        want[..., lam] = (w * shade * rad).reshape(H, W, spp).sum(2) / spp
        wfrag[..., lam] = ((np.where(fragile > 0, w_pot * reach, 0.0) + own) * rad).reshape(H, W, spp).sum(2) / spp
    assert want.max() > 0 and 20 < (want[..., 0] > 0).sum()
    assert np.abs(img - want).max() <= 1e-12 * want.max(), np.abs(img - want).max() / want.max()
    assert np.abs(frag - wfrag).max() <= 1e-12 * max(wfrag.max(), want.max())
    if light[0] == AREA:
        # (the outline crosses the frame's rays: a good part of them passes inside it and a good part outside)
        assert 0.05 * c["rays_reached_scene"] < c["rays_hit_light"] < 0.95 * c["rays_reached_scene"]
        assert c["light_edge_pairs"] == n_edge > 0
        print(f"primary path, {name}: {c['rays_hit_light']} rays inside, {n_edge} in the band ({n_edge / c['rays_hit_light']:.3%})")
        assert n_edge <= 0.01 * c["rays_hit_light"]
    else:
        assert c["light_edge_pairs"] == 0


# ---- 3. a distant lamp ------------------------------------------------------------------------------------------------------------
def test_a_lamp_far_away_is_the_directional_light_within_its_parallax(mask):
    """DESIGN.md section 5 ("Point lights"): from every point P of the front element |unit(L - P) - unit(L)| <= delta =
    r_f / (|L| - r_f).  With q = (1 - cos(theta)) / (1 - cos(alpha)) and the factor max(0, 1 - q)^2 -- continuous at the lobe's
    edge -- |d factor / d theta| = 2 (1 - q) sin(theta) / (1 - cos(alpha)) <= 2 sin(alpha + delta) / (1 - cos(alpha)) wherever
    either factor is not 0, so per ray |factor_lamp - factor_sun| <= B = 2 sin(alpha + delta) delta / (1 - cos(alpha)), and per
    pixel B times the summed weight x radiance of the rays that leave the lens: the image of the whole sky at the same radiance."""
    W, H, spp, key = 64, 48, 16, 0x64C1
    lens = crop(_pkg().load_lens_file("dgauss11.lens"), W)
    dist, alpha = 1e7, 0.05
    L = (dist * OFF_AXIS / np.linalg.norm(OFF_AXIS)).astype(np.float32)
    lamp, _, cl = _trace(lens, W, H, spp, key, mask, [(POINT, L, RAD, alpha)])
    sun, _, cs = _trace(lens, W, H, spp, key, mask, [(DIRECTIONAL, L, RAD, alpha)])
    sky, _, _ = _trace(lens, W, H, spp, key, mask, [SKY])
    delta = r_f_of(lens) / (dist - r_f_of(lens))
    B = 2.0 * np.sin(alpha + delta) * delta / (1.0 - np.cos(alpha))
    err = np.abs(lamp - sun)
    print(f"lamp at {dist:g} mm: delta {delta:.2e} rad, bound {B:.2e} x sky, largest |lamp - sun| / sky {np.max(err[sky > 0] / sky[sky > 0]):.2e}")
    assert sun.max() > 0 and not np.array_equal(lamp, sun)
    assert (err <= B * sky + 1e-15 * sun.max()).all()
    # (the bound is not slack by orders of magnitude: the parallax is seen)
    assert err.max() > 1e-3 * B * sky.max()


# ---- 4. additivity ----------------------------------------------------------------------------------------------------------------
def test_lights_add_a_rectangle_is_its_halves_and_the_sky_lights_every_ray(mask):
    W, H, spp, key = 64, 48, 16, 0x64D1
    lens = crop(_pkg().load_lens_file("dgauss11.lens"), W)
    lights = [SUN, LAMP, TILTED]
    both, fboth, cb = _trace(lens, W, H, spp, key, mask, lights)
    singles = [_trace(lens, W, H, spp, key, mask, [l]) for l in lights]
    total = singles[0][0] + singles[1][0] + singles[2][0]
    assert all(s[0].max() > 0 for s in singles)
    assert np.abs(both - total).max() <= 1e-13 * both.max()
    assert np.abs(fboth - (singles[0][1] + singles[1][1] + singles[2][1])).max() <= 1e-13 * max(fboth.max(), both.max())
    assert cb["rays_hit_light"] == sum(s[2]["rays_hit_light"] for s in singles)
    assert cb["light_edge_pairs"] == singles[2][2]["light_edge_pairs"] > 0 == singles[0][2]["light_edge_pairs"]
    for name in lfo.G64_COUNTERS[:6] + ("rays_fragile",):          # (the rays and their fates do not depend on a light)
        assert all(s[2][name] == cb[name] for s in singles), name
    # a rectangle is its two halves, up to the rays on the seam: they lie in both halves' bands
    C, e1, e2 = (np.asarray(x, np.float64) for x in RECTS[1])
    halves = [(AREA, geom_of((C + s * e1 / 4, e1 / 2, e2)), RAD, 0.0) for s in (-1, 1)]
    whole = singles[2][0]
    h = [_trace(lens, W, H, spp, key, mask, [x]) for x in halves]
    seam = np.minimum(h[0][1], h[1][1])
    assert (np.abs(whole - (h[0][0] + h[1][0])) <= seam + 1e-13 * whole.max()).all()
    two, _, c2 = _trace(lens, W, H, spp, key, mask, halves)
    assert np.abs(two - (h[0][0] + h[1][0])).max() <= 1e-13 * whole.max()
    assert abs(c2["rays_hit_light"] - singles[2][2]["rays_hit_light"]) <= c2["light_edge_pairs"]
    # the whole sky lights every ray that reaches the scene
    _, _, csky = _trace(lens, W, H, spp, key, mask, [SKY])
    assert csky["rays_hit_light"] == csky["rays_reached_scene"] > 0 and csky["light_edge_pairs"] == 0
    # ... and a rectangle seen from behind none
    # (its `frag` is not empty: a ray that could not be followed -- a grazing miss -- is bound by factor 1 for every light)
    back, fback, cback = _trace(lens, W, H, spp, key, mask, [BEHIND])
    assert not back.any() and cback["rays_hit_light"] == 0 and cback["light_edge_pairs"] == 0
    assert (fback <= singles[2][1]).all()          # (... the same rays and the same bound as in the rectangle's own frame)


# ---- 5. the fragility caps on the tracer alone --------------------------------------------------------------------------------------
def test_the_bands_constants_are_ten_times_the_measured_deviation(mask):
    """eps_exit, eps_dir = 10 x the largest float32-versus-float64 deviation of the exit point / unit exit direction over the
    primary path and all 45 pairs x 3 wavelengths of the tracer's own sample rays of one 64 x 48 x 64 spp frame of the lens
    every frame here uses (a film moves no ray: the coated file has the same prescription); fragile rays skipped"""
    pkg = _pkg()
    lens = crop(pkg.load_lens_file("dgauss11.lens"), 64)
    coated = pkg.load_lens_file("dgauss11_coated.lens")
    assert all(np.array_equal(lens[k], coated[k]) for k in ("radius", "thickness", "semi_aperture", "ior"))
    assert {FRAMES[n][1] for n in FRAMES} == {64}
    e_pos, e_dir, n, fates = lfo.g64_exit_deviation(lens, 64, 48, 64, 0xE95, mask)
    eps_exit, eps_dir, eps_test = lfo.g64_light_eps()
    print(f"{n} rays compared: exit point {e_pos:.3e} mm, direction {e_dir:.3e}; eps_exit {eps_exit:.3e}, eps_dir {eps_dir:.3e}")
    assert n > 4e6 and fates == 0
    assert 10.0 * e_pos <= eps_exit <= 10.1 * e_pos and 10.0 * e_dir <= eps_dir <= 10.1 * e_dir
    assert eps_test == 2.4e-7          # (4 * 2^-24: the float32 test's own rounding, tests/test_area_ghosts_cpu.py)



@pytest.mark.parametrize("name", ["tilted", "mixed", "coated"])
def test_edge_band_stays_the_exception_on_the_gpu_tests_frames(mask, name):
    """every frame of tests/test_gpu_lights_f64.py that holds a rectangle, ghosts included (64 of its 256 spp: a share), per
    area light: the (ray, light) pairs in the band are at most 1 % of that light's lit pairs"""
    lens, W, H, key, lights = frame_of(_pkg(), name)
    lfo.g64_set_films(lens.get("coatings"))
    try:
        for light in lights:
            if light[0] != AREA:
                continue
            img, _, c = _trace(lens, W, H, 64, key, mask, [light])
            share = c["light_edge_pairs"] / c["rays_hit_light"]
            print(f"{name}: {c['rays_hit_light']} lit pairs, {c['light_edge_pairs']} in the band ({share:.3%}), {(img >= 2e-5).sum()} lit values")
            assert share <= 0.01 and (img >= 2e-5).sum() >= 150
    finally:
        lfo.g64_set_films(None)
