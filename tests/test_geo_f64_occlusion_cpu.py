"""The float64 tracer (oracle/lf_geo_f64.c) under an OCCLUDER LIST (lfo.g64_set_occlusion, g64_trace(occlusion=...)), CPU only:
what makes it a reference for occluded ghost frames (tests/test_gpu_occlusion_f64.py).  The tracer is "parity unpinned" by
construction, so it is anchored here before it judges anything: (1) off, and a scene nothing can meet, is the tracer without the
list, bit for bit; (2) a wall on the front element leaves nothing, two half planes add up; (3) the C mapping is
lfo.lens_exit_to_world, and under a general pose the C decisions are those of an analytic sphere and quad in numpy -- and not
those under the transposed pose; (4) the reach: a wall behind a lamp hides nothing, one in front everything, a quad in a panel's
own plane nothing; (5) on every frame the GPU test renders, the occluders' edge band stays the exception and every partly
hidden light is partly hidden; (6) the band's two constants are what they were measured to be.

THE FRAMES of the GPU test are defined here (OCCL_FRAMES), so that (5) measures exactly what that test renders.  Occluders are
written in CAMERA coordinates (world units; the lens-space point (x, y, z) mm lies at ((x, y, z - z_ref) wpm)) and carried to the
world through POSE in float64."""
import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo
from test_area_ghosts_cpu import RECTS, AREA, geom_of
from test_geo_f64_lights_cpu import MASK, RAD, RAD2, RAD3, SUN, SUN_B, TILTED, crop, DIRECTIONAL, POINT

WPM = 0.001
RAD4 = [0.125, 0.25, 0.5]
LAMP = (POINT, [-3.0, 2.0, -300.0], RAD3, 0.03)          # the lamp 300 mm out of tests/test_gpu_near_occlusion.py
LAMP2 = (POINT, [1.5, -1.0, -90.0], RAD, 0.05)
PANEL90 = (AREA, TILTED[1], RAD4, 0.0)                   # the tilted 12 x 8 mm parallelogram at 90 mm
PANEL300 = (AREA, geom_of(RECTS[0]), RAD, 0.0)           # 40 x 24 mm, square to the axis, 300 mm out
SKY, LIGHT = lfo.REACH_SKY, lfo.REACH_LIGHT


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


# one general pose for every frame: 0.4 rad about the skew axis (1, 2, 3), away from the origin
POSE = (_rotation((1.0, 2.0, 3.0), 0.4), np.array([0.3, -1.2, 2.5]))
IDENTITY = (np.eye(3), np.zeros(3))
assert np.abs(POSE[0] - POSE[0].T).max() > 0.3          # (far from symmetric: the transposed pose is another pose)


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def z_ref_of(lens):
    """the paraxial entrance pupil's z at the reference wavelength (host arithmetic): what lf_get_lens_camera reports"""
    return float(_pkg().paraxial_entrance_pupil(lens)[0])


def cam_z(z_ref, mm_in_front):
    """camera z of the lens-space plane `mm_in_front` millimetres in front of the first vertex"""
    return (-mm_in_front - z_ref) * WPM


def quad(x0, x1, y0, y1, z):
    """two triangles (nine numbers each) over [x0, x1] x [y0, y1] of the camera plane z"""
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    return [a + b + c, a + c + d]


def icosphere(centre, radius, subdivisions=2):
    """20 x 4^subdivisions triangles inscribed in the sphere (320 at two subdivisions)"""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    tris = [[np.asarray(v[i], np.float64) / np.sqrt(1.0 + g * g) for i in t] for t in f]
    for _ in range(subdivisions):
        nxt = []
        for a, b, c in tris:
            ab, bc, ca = [(p + q) / np.linalg.norm(p + q) for p, q in ((a, b), (b, c), (c, a))]
            nxt += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        tris = nxt
    c = np.asarray(centre, np.float64)
    return [tuple(np.concatenate([c + radius * p for p in t])) for t in tris]


def to_world(pose, spheres, tris):
    """camera coordinates -> world through the pose, in float64"""
    R, pos = pose
    sp = [tuple(pos + R @ np.asarray(s[:3], np.float64)) + (float(s[3]),) for s in spheres]
    tr = [tuple(np.concatenate([pos + R @ np.asarray(t[3 * i:3 * i + 3], np.float64) for i in range(3)])) for t in tris]
    return sp, tr


def comb(lens, z_ref, mm_in_front=2.0, period=2.0, open_share=0.5):
    """slats along y, `period` mm apart and (1 - open_share) of it wide, across 2.2 clear diameters of the front element"""
    h = 2.2 * float(lens["semi_aperture"][0])
    n = int(np.ceil(h / period))
    z = cam_z(z_ref, mm_in_front)
    return [t for k in range(-n, n) for t in quad(k * period * WPM, (k + 1.0 - open_share) * period * WPM, -h * WPM, h * WPM, z)]


def _sun_sky_scene(lens, z_ref):
    # an analytic sphere 0.35 m out over part of the beam, a tessellated one (320 triangles) 0.6 m out over another part, and the
    # comb 2 mm in front of the first vertex: its edges cut right across the front element
    spheres = [(0.022, -0.008, cam_z(z_ref, 350.0), 0.016)]
    mesh = icosphere((-0.026, 0.012, cam_z(z_ref, 600.0)), 0.024)
    return spheres, mesh + comb(lens, z_ref)


def _lamp_scene(lens, z_ref):
    # a half wall (x < -1 mm) half way to the lamp, and a full wall 50 mm behind it
    return [], quad(-0.5, -0.001, -0.5, 0.5, cam_z(z_ref, 150.0)) + quad(-1.0, 1.0, -1.0, 1.0, cam_z(z_ref, 350.0))


def _mixed_scene(lens, z_ref):
    # half walls at three depths: in front of everything (40 mm: y > 0.5 mm), between the lights at 90 mm and the lamp at 300 mm
    # (150 mm: x < -2 mm), and beyond the lamp (600 mm: y < -6 mm, which only the sun's rays reach)
    return [], (quad(-0.5, 0.5, 0.0005, 0.5, cam_z(z_ref, 40.0)) + quad(-0.5, -0.002, -0.5, 0.5, cam_z(z_ref, 150.0))
                + quad(-1.0, 1.0, -1.0, -0.006, cam_z(z_ref, 600.0)))


LAST_WAVELENGTH = [[0.0] * 3, [0.0] * 3, [1.0] * 3]
# name -> (lens file, W, H, key, lights, reach, occluders in camera coordinates (lens, z_ref) -> (spheres, triangles),
#          the lights that are partly hidden, lambda_rgb or None); every frame is the 64-pixel crop of the 36 mm / 1920 sensor
OCCL_FRAMES = {
    "sun_sky": ("dgauss11.lens", 64, 48, 0x0CF1, [SUN], SKY, _sun_sky_scene, [0], None),
    "two_suns_sky": ("dgauss11.lens", 64, 48, 0x0CF2, [SUN, SUN_B], SKY, _sun_sky_scene, [0, 1], None),
    "lamp_reach": ("dgauss11.lens", 64, 48, 0x0CF3, [LAMP], LIGHT, _lamp_scene, [0], None),
    "mixed_reach": ("dgauss11.lens", 64, 48, 0x0CF4, [SUN, LAMP, LAMP2, PANEL90], LIGHT, _mixed_scene, [0, 1, 2, 3], None),
    "sun_sky_last_wavelength": ("dgauss11.lens", 64, 48, 0x0CF5, [SUN], SKY, _sun_sky_scene, [0], LAST_WAVELENGTH),
}


def frame_of(pkg, name, pose=POSE):
    """-> (lens, W, H, key, lights, occlusion, partly, lambda_rgb, (spheres, triangles) in the world) of OCCL_FRAMES[name]; occlusion =
    the keyword arguments of lfo.g64_set_occlusion under `pose`"""
    fname, W, H, key, lights, reach, scene, partly, lambda_rgb = OCCL_FRAMES[name]
    lens = crop(pkg.load_lens_file(fname), W)
    z_ref = z_ref_of(lens)
    sp, tr = to_world(pose, *scene(lens, z_ref))
    occlusion = dict(spheres=sp, triangles=tr, c2w=pose[0], pos=pose[1], world_per_mm=WPM, z_ref_mm=z_ref, reach=reach)
    return lens, W, H, key, lights, occlusion, partly, lambda_rgb, (sp, tr)


@pytest.fixture(scope="module")
def mask():
    return load_texels(MASK)


@pytest.fixture(scope="module")
def lens64():
    return crop(_pkg().load_lens_file("dgauss11.lens"), 64)


def _trace(lens, W, H, spp, key, mask, lights, occlusion=None, **kw):
    return lfo.g64_trace(lens, W, H, 0, H, spp, key, None, True, mask, [0.0, 0.0, -1.0], [0.0, 0.0, 0.0], 0.05, lights=lights,
                         occlusion=occlusion, **kw)


def _occl(lens, spheres=(), tris=(), pose=IDENTITY, reach=SKY):
    sp, tr = to_world(pose, spheres, tris)
    return dict(spheres=sp, triangles=tr, c2w=pose[0], pos=pose[1], world_per_mm=WPM, z_ref_mm=z_ref_of(lens), reach=reach)


# ---- 1. off is unchanged ------------------------------------------------------------------------------------------------------
def test_off_and_what_no_ray_can_meet_are_the_tracer_without_the_list(mask, lens64):
    lens = _pkg().load_lens_file("dgauss11.lens")
    W, H, spp, key = 32, 24, 16, 0x5117
    sun, rad, alpha = [0.03, 0.02, -1.0], [1.0, 0.9, 0.5], 0.05
    # without a light list: the parent commit's figures (tests/test_geo_f64_lights_cpu.py holds the same frame to them), before and
    # after a list of occluders has been set and cleared
    for again in (False, True):
        if again:
            lfo.g64_set_occlusion(**_occl(lens, [(0.0, 0.0, -0.1, 0.05)], quad(-1, 1, -1, 1, -0.05)))
            lfo.g64_set_occlusion()
        img, frag, c = lfo.g64_trace(lens, W, H, 0, H, spp, key, None, True, mask, sun, rad, alpha)
        assert float(img.sum()).hex() == "0x1.eb353ddc402dbp-5", float(img.sum()).hex()
        assert float(frag.sum()).hex() == "0x1.845be3a081deap-11" and (c["rays_hit_light"], c["rays_fragile"]) == (6238, 7905)
    # with a list: an empty occluder list, a wall behind the camera and a wall beside the beam change no bit and no counter
    W, H, spp, key = 64, 48, 16, 0x0CE1
    lights = [SUN, LAMP, TILTED]
    want = _trace(lens64, W, H, spp, key, mask, lights)
    pairs = lfo.g64_last_light_pairs
    assert want[0].max() > 0 and lfo.g64_last_occlusion_pairs is None
    h = 2.2 * float(lens64["semi_aperture"][0]) * WPM
    z_ref = z_ref_of(lens64)
    scenes = {"empty": ([], []), "behind": ([(0.0, 0.0, 5.0, 1.0)], quad(-9.0, 9.0, -9.0, 9.0, 0.5)),
              "beside": ([], quad(-h + 6.0 * h, h + 6.0 * h, -h, h, cam_z(z_ref, 0.1)))}
    for name, (sp, tr) in scenes.items():
        for pose in (IDENTITY, POSE):
            got = _trace(lens64, W, H, spp, key, mask, lights, _occl(lens64, sp, tr, pose, LIGHT))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], name
            assert lfo.g64_last_light_pairs == pairs
            o = lfo.g64_last_occlusion_pairs
            if name == "empty":
                assert o["tested"] == 0          # (no primitive: the list is off)
            else:
                assert o["tested"] == want[2]["rays_hit_light"] and o["blocked"] == o["edge"] == 0
                assert [p[0] for p in o["per_light"]] == [p[0] for p in pairs]
    # ... and the setting is cleared afterwards
    again = _trace(lens64, W, H, spp, key, mask, lights)
    assert np.array_equal(again[0], want[0]) and again[2] == want[2]


# ---- 2. full and half walls ---------------------------------------------------------------------------------------------------
def test_a_wall_on_the_front_element_leaves_nothing_and_half_planes_add_up(mask, lens64):
    W, H, spp, key = 64, 48, 16, 0x0CE2
    lights = [(DIRECTIONAL, [0.0, 0.0, -1.0], RAD, 0.05)]
    free, ffree, cf = _trace(lens64, W, H, spp, key, mask, lights)
    z_ref = z_ref_of(lens64)
    h = 2.2 * float(lens64["semi_aperture"][0]) * WPM
    for pose in (IDENTITY, POSE):
        img, frag, c = _trace(lens64, W, H, spp, key, mask, lights, _occl(lens64, [], quad(-h, h, -h, h, cam_z(z_ref, 0.1)), pose))
        o = lfo.g64_last_occlusion_pairs
        assert not img.any() and c["rays_hit_light"] == 0 and o["blocked"] == o["tested"] == cf["rays_hit_light"] > 0
        assert {k: v for k, v in c.items() if k != "rays_hit_light"} == {k: v for k, v in cf.items() if k != "rays_hit_light"}
    # the two half planes of tests/test_gpu_ghost_occlusion.py _halves: 1 mm in front of the lens, and 100 m away
    for where, (z, L) in dict(near=(cam_z(z_ref, 1.0), 10.0 * float(lens64["semi_aperture"][0]) * WPM), far=(-100.0, 50.0)).items():
        parts = []
        for half in (quad(-L, 0.0, -L, L, z), quad(0.0, L, -L, L, z)):
            img, frag, c = _trace(lens64, W, H, spp, key, mask, lights, _occl(lens64, [], half, POSE))
            parts.append((img, c, lfo.g64_last_occlusion_pairs))
        (ia, ca, oa), (ib, cb, ob) = parts
        edge = max(oa["edge"], ob["edge"])
        print(f"{where}: blocked {oa['blocked']} + {ob['blocked']} of {oa['tested']}, edge pairs {oa['edge']} / {ob['edge']}")
        assert oa["tested"] == ob["tested"] == cf["rays_hit_light"]
        assert abs(oa["blocked"] + ob["blocked"] - oa["tested"]) <= edge
        assert 0.2 < ia.sum() / free.sum() < 0.8
        assert np.abs(ia + ib - free).max() <= 1e-12 * free.max()          # (float64 puts every ray on one side of the seam)
        assert edge > 0 or where == "far"


# ---- 3. the pose -------------------------------------------------------------------------------------------------------------
POSE_SPHERE = (0.02, -0.01, -0.35, 0.03)                     # camera coordinates, as tests/test_gpu_ghost_occlusion.py has them
POSE_QUAD = (-0.10, 0.01, -0.02, 0.09, -0.8)


def _analytic(o, d, pose):
    """(blocked, margin) of the world rays (o, unit d) against POSE_SPHERE and POSE_QUAD standing in camera coordinates under
    `pose`, in numpy: the rays are taken BACK to the camera (its inverse), where the sphere and the quad are axis-aligned"""
    R, pos = pose
    oc_, dc_ = (o - pos) @ R, d @ R                          # R^T (o - pos), R^T d
    c, rad = np.array(POSE_SPHERE[:3]), POSE_SPHERE[3]
    oc = oc_ - c
    b = (oc * dc_).sum(1)
    disc = b * b - ((oc * oc).sum(1) - rad * rad)
    hit_s = (disc > 0) & (-b + np.sqrt(np.maximum(disc, 0)) > 0)
    m_s = np.abs(disc) / np.maximum(b * b, 1e-300)
    x0, x1, y0, y1, z = POSE_QUAD
    t = (z - oc_[:, 2]) / dc_[:, 2]
    u = (oc_[:, 0] + t * dc_[:, 0] - x0) / (x1 - x0)
    v = (oc_[:, 1] + t * dc_[:, 1] - y0) / (y1 - y0)
    hit_q = (t > 0) & (u > 0) & (u < 1) & (v > 0) & (v < 1)
    m_q = np.minimum.reduce([np.abs(u), np.abs(1 - u), np.abs(v), np.abs(1 - v), np.abs(u - v)])
    return hit_s | hit_q, np.minimum(m_s, m_q)


def test_the_mapping_is_lens_exit_to_world_and_a_general_pose_is_not_its_transpose(lens64):
    rng = np.random.default_rng(0x0CE3)
    n = 512
    h, R0 = float(lens64["semi_aperture"][0]), float(lens64["radius"][0])
    rho, phi = h * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    ang, psi = 0.1 * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    P = np.stack([rho * np.cos(phi), rho * np.sin(phi), R0 - np.sign(R0) * np.sqrt(R0 * R0 - rho * rho)], 1)
    d = np.stack([np.sin(ang) * np.cos(psi), np.sin(ang) * np.sin(psi), -np.cos(ang)], 1) * rng.uniform(0.5, 2.0, (n, 1))
    z_ref = z_ref_of(lens64)
    assert abs(z_ref) > 1.0
    x0, x1, y0, y1, z = POSE_QUAD
    answers = {}
    for name, pose in dict(general=POSE, transposed=(POSE[0].T, POSE[1])).items():
        # the occluders stand where POSE puts them; the camera maps with `pose`
        sp, tr = to_world(POSE, [POSE_SPHERE], quad(x0, x1, y0, y1, z))
        lfo.g64_set_occlusion(spheres=sp, triangles=tr, c2w=pose[0], pos=pose[1], world_per_mm=WPM, z_ref_mm=z_ref)
        try:
            blocked, edge, o, dw, reach = lfo.g64_occlusion_rays(P, d)
        finally:
            lfo.g64_set_occlusion()
        want_o, want_d = lfo.lens_exit_to_world(P, d, pose[0], pose[1], WPM, z_ref)
        assert np.abs(o - want_o).max() <= 1e-12 and np.abs(dw - want_d).max() <= 1e-12 and np.isinf(reach).all()
        hit, margin = _analytic(want_o, want_d, POSE)
        sure = margin >= 1e-9
        assert (~sure).sum() <= n // 100
        assert np.array_equal(blocked[sure], hit[sure]), name
        answers[name] = blocked
    assert 0.05 * n < answers["general"].sum() < 0.95 * n          # (both answers occur, often)
    assert (answers["general"] != answers["transposed"]).sum() > 0.05 * n


# ---- 4. the reach ------------------------------------------------------------------------------------------------------------
def test_the_reach_ends_at_the_lamp_and_just_before_the_panel(mask, lens64):
    W, H, spp, key = 64, 48, 16, 0x0CE4
    z_ref = z_ref_of(lens64)
    wall = lambda mm: quad(-1.0, 1.0, -1.0, 1.0, cam_z(z_ref, mm))          # noqa: E731
    for light in (LAMP, PANEL300):
        free, _, cf = _trace(lens64, W, H, spp, key, mask, [light])
        assert free.max() > 0
        # a wall behind the light hides nothing; under the sky's reach it would hide everything
        img, frag, c = _trace(lens64, W, H, spp, key, mask, [light], _occl(lens64, [], wall(400.0), POSE, LIGHT))
        assert np.array_equal(img, free) and c == cf and lfo.g64_last_occlusion_pairs["blocked"] == 0
        img, _, c = _trace(lens64, W, H, spp, key, mask, [light], _occl(lens64, [], wall(400.0), POSE, SKY))
        assert not img.any() and c["rays_hit_light"] == 0
        # the same wall 10 mm nearer than the light hides everything
        img, _, c = _trace(lens64, W, H, spp, key, mask, [light], _occl(lens64, [], wall(290.0), POSE, LIGHT))
        o = lfo.g64_last_occlusion_pairs
        assert not img.any() and o["blocked"] == o["tested"] == cf["rays_hit_light"]
        # (the band holds the rays across the wall's diagonal alone: neither of its two triangles blocks such a ray FIRMLY)
        assert 0 < o["edge"] <= EDGE_CAP * o["tested"]
    # ... and where it covers a cone only, everything in that cone: the half wall's frame and the other half's add up
    free, _, cf = _trace(lens64, W, H, spp, key, mask, [LAMP])
    parts = [_trace(lens64, W, H, spp, key, mask, [LAMP], _occl(lens64, [], quad(x0, x1, -1.0, 1.0, cam_z(z_ref, 290.0)), POSE, LIGHT))
             + (lfo.g64_last_occlusion_pairs,) for x0, x1 in ((-1.0, 0.0), (0.0, 1.0))]
    assert abs(parts[0][3]["blocked"] + parts[1][3]["blocked"] - cf["rays_hit_light"]) <= max(p[3]["edge"] for p in parts)
    assert all(0.1 < p[3]["blocked"] / p[3]["tested"] < 0.9 for p in parts)
    # a quad lying in the panel's own plane -- the lamp's emissive mesh -- does not hide the panel
    free, _, cf = _trace(lens64, W, H, spp, key, mask, [PANEL300])
    img, _, c = _trace(lens64, W, H, spp, key, mask, [PANEL300], _occl(lens64, [], quad(-0.1, 0.1, -0.1, 0.1, cam_z(z_ref, 300.0)), POSE, LIGHT))
    o = lfo.g64_last_occlusion_pairs
    assert np.array_equal(img, free) and c == cf and o["blocked"] == 0 and o["tested"] > 0


def test_reach_of_a_ray_is_the_definition(lens64):
    """per ray: +inf for a directional light, wpm (L - P) . unit(d) for a lamp, wpm t - (double)0.00001f for a rectangle, t from
    uv64's plane intersection written again here"""
    rng = np.random.default_rng(0x0CE5)
    n = 64
    P = np.concatenate([rng.uniform(-10, 10, (n, 2)), rng.uniform(0, 2, (n, 1))], 1)
    d = np.concatenate([rng.uniform(-0.05, 0.05, (n, 2)), -np.ones((n, 1))], 1)
    dn = d / np.linalg.norm(d, axis=1)[:, None]
    lights = [SUN, LAMP, PANEL90]
    lfo.g64_set_lights(lights)
    lfo.g64_set_occlusion(**_occl(lens64, [(0.0, 0.0, 9.0, 1.0)], [], POSE, LIGHT))
    try:
        reach = [lfo.g64_occlusion_rays(P, d, k)[4] for k in range(3)]
        sky = lfo.g64_occlusion_rays(P, d, -1)[4]
    finally:
        lfo.g64_set_occlusion()
        lfo.g64_set_lights(None)
    assert np.isinf(reach[0]).all() and np.isinf(sky).all()
    Lp = np.asarray(LAMP[1], np.float32).astype(np.float64)
    assert np.abs(reach[1] - WPM * ((Lp - P) * dn).sum(1)).max() <= 1e-15
    g = np.asarray(PANEL90[1], np.float32).astype(np.float64)
    nrm = np.cross(g[6:9], g[9:12])
    t = ((g[0:3] - P) @ nrm) / (dn @ nrm)
    assert np.abs(reach[2] - (WPM * t - float(np.float32(0.00001)))).max() <= 1e-15 and (reach[2] > 0.08).all()


# ---- 5. the caps, on the frames the GPU test renders ------------------------------------------------------------------------------
EDGE_CAP = 0.01


@pytest.mark.parametrize("name", sorted(OCCL_FRAMES))
def test_edge_band_stays_the_exception_and_partly_hidden_lights_are_partly_hidden(mask, name):
    """per light: the pairs in the occluders' band are at most 1 % of the pairs tested, and 0.1 < blocked / tested < 0.9 for
    every light the frame calls partly hidden (64 spp: the shares are those of the GPU test's 256)"""
    lens, W, H, key, lights, occlusion, partly, lambda_rgb, (sp, tr) = frame_of(_pkg(), name)
    img, frag, c = _trace(lens, W, H, 64, key, mask, lights, occlusion, lambda_rgb=lambda_rgb, n_threads=16)
    o = lfo.g64_last_occlusion_pairs
    print(f"{name}: {len(sp)} spheres, {len(tr)} triangles; {(img >= 2e-5).sum()} lit values; per light (tested, blocked, edge) {o['per_light'][:len(lights)]}")
    assert (img >= 2e-5).sum() >= 150
    assert c["rays_hit_light"] == o["tested"] - o["blocked"]
    for k in range(len(lights)):
        tested, blocked, edge = o["per_light"][k]
        assert tested > 0 and edge <= EDGE_CAP * tested, (k, tested, edge)
        if k in partly:
            assert 0.1 < blocked / tested < 0.9, (k, blocked, tested)
    if name.startswith("sun_sky"):
        assert len(tr) >= 320 + 2 and len(sp) == 1


# ---- 6. the constants ---------------------------------------------------------------------------------------------------------
def test_the_bands_constants_hold_on_the_lens_and_crop_of_every_frame(mask):
    """the occluders' band reuses eps_exit and eps_dir = 10 x the largest float32-versus-float64 deviation of the exit point / the
    unit exit direction: measured again on the one lens and crop every frame of OCCL_FRAMES uses"""
    assert {(f[0], f[1], f[2]) for f in OCCL_FRAMES.values()} == {("dgauss11.lens", 64, 48)}
    lens = crop(_pkg().load_lens_file("dgauss11.lens"), 64)
    e_pos, e_dir, n, fates = lfo.g64_exit_deviation(lens, 64, 48, 64, 0xE95, mask)
    eps_exit, eps_dir, _ = lfo.g64_light_eps()
    print(f"{n} rays compared: exit point {e_pos:.3e} mm, direction {e_dir:.3e}; eps_exit {eps_exit:.3e}, eps_dir {eps_dir:.3e}")
    assert n > 4e6 and fates == 0
    assert e_pos <= eps_exit / 10.0 and e_dir <= eps_dir / 10.0
