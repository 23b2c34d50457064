"""Lens ghosts of the scene's area lights (lf_set_lights_geom, LF_LIGHT_AREA; lens-flare_amd/csrc: lf_area_inside /
lf_area_pretest / lf_area_shadow_reach in lf_march_events.h, light_admits_at / lights_pretest / lights_epilogue<VAR & kVarArea>
in lf_march_common.h, k_cull_audit_area and the cone in lf_cull_prepass.hip, the kVarArea instantiations of k_march /
k_march_cull / k_march_items): every ray that has left the front element is tested against the rectangle itself, from ITS
OWN exit point.  The reference's ghosts know only `angle_to_sun`.

Contributions are unsigned 64-bit fixed-point integers, so the identities here are bit for bit: spp is a power of two and
`bits` 36 throughout (checked), a frame is acc 2^-36 / spp and sums of frames are exact in float64 (sums below 2^53).  The
radiances are powers of two: weight x radiance is then exact in float32, and what separates the device's pixel from the
float64 sum over the oracle's samples is the truncation to the 2^-36 grid alone (below 2^-36 per pixel and channel) -- and
the samples within EDGE of the rectangle's outline, whose weight is the tolerance (tests/test_area_ghosts_cpu.py)."""
import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo
from test_area_ghosts_cpu import RECTS, EDGE, AREA, geom_of, area_rays, inside64, uv64
from test_gpu_near_occlusion import _quad, _wall, _half, _plane_z, _z_ref_of, _map, analytic

pytestmark = pytest.mark.gpu
RAD = [1.0, 0.5, 0.25]
RAD2 = [0.5, 1.0, 0.125]
RAD3 = [0.25, 0.125, 1.0]
MASK = "pentbig500_14.png"
WPM = 0.001
DIRECTIONAL, POINT = 0, 1
LF_ERR_INVALID, LF_ERR_STATE = 1, 4
# (kind, geometry, radiance, angular radius)
SUN = (DIRECTIONAL, [0.012, 0.004, -1.0], RAD2, 0.03)
LAMP = (POINT, [1.5, -1.0, -90.0], RAD3, 0.05)
PANEL = (AREA, geom_of(RECTS[0]), RAD, 0.0)
MIXED = [SUN, LAMP, PANEL]


def _rect(k, rad=RAD, direction=(0.0, 0.0, 1.0)):
    return (AREA, geom_of(RECTS[k], direction), rad, 0.0)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="module")
def mask():
    return load_texels(MASK)


@pytest.fixture(scope="module")
def lf(pkg):
    ctx = pkg.LensFlare(0)
    yield ctx
    ctx.close()


@pytest.fixture()
def forced(pkg, lf):
    """the culled march whatever the table starts, as tests/test_gpu_multi_light.py forces it"""
    lf.test_knob("cull_force", 1)
    pkg.test_knob_default("cull_force", 1)
    yield
    lf.test_knob("cull_force", 0)
    pkg.test_knob_default("cull_force", 0)


def _crop(lens, W, pitch_of=1920):
    c = dict(lens)
    c["sensor_width_mm"] = 36.0 * W / pitch_of
    return c


def _setup(pkg, lf, lens, W, H, mask, lambda_rgb=None):
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    if lambda_rgb is not None:
        lf.set_lambda_rgb(lambda_rgb)
    lf.set_ghost_pairs(None, True)
    lf.set_band(0, H)
    lf.set_row_interleave(0, 1)
    lf.set_tile_stride(8)
    lf.set_pupil_subcells(6)
    lf.set_mask_filter(pkg.MASK_NEAREST)
    lf.set_ghost_accumulate(False)
    lf.set_camera(np.eye(3).reshape(-1), [0.0, 0.0, 0.0], 40.0, 27.0)
    lf.set_ghost_occlusion(False)
    lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_SKY)


def _install(lf, lights):
    lf.set_lights_geom([l[0] for l in lights], [l[1] for l in lights], [l[2] for l in lights], [l[3] for l in lights])


def _frame(pkg, lf, spp, key, mode):
    lf.set_march_culling(mode)
    lf.reset_counters()
    lf.trace_ghosts(spp, key)
    assert lf.march_fix_bits() == 36
    return lf.read_buffer(pkg.GHOST_BUFFER), lf.counters()


def _variant(lf):
    return lf.get_ghost_occlusion()["march_variant"]


def _primary(pkg, lf, lights, spp, key):
    """the primary path alone: {pair (0, 1), primary} minus {pair (0, 1)} under one key (the sums are integers)"""
    _install(lf, lights)
    lf.set_ghost_pairs([(0, 1)], True)
    a, ca = _frame(pkg, lf, spp, key, 0)
    lf.set_ghost_pairs([(0, 1)], False)
    b, cb = _frame(pkg, lf, spp, key, 0)
    return a - b, ca["rays_hit_light"] - cb["rays_hit_light"]


def _samples(pkg, lf, lens, W, H, spp, key, mask):
    lfo.geo_follow_device(lf)
    try:
        smp = lfo.geo_lens_samples(lens, W, H, spp, key, 1, np.arange(W * H), mask).astype(np.float64)
    finally:
        lfo.geo_follow_device(None)
    return smp.reshape(W * H * spp, 8)


# ---- 1. per ray -----------------------------------------------------------------------------------------------------------
def test_per_ray_factors_are_the_host_function_bit_for_bit(pkg, lf, mask):
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), 80)
    _setup(pkg, lf, lens, 80, 48, mask)
    lights = [_rect(0), SUN, _rect(1), LAMP, _rect(2), _rect(3)]
    _install(lf, lights)
    assert _variant(lf) == 4 | 32 | 64
    h, R = float(lens["semi_aperture"][0]), float(lens["radius"][0])
    rays = np.concatenate([area_rays(np.random.default_rng(0xA5EA + k), 4096, RECTS[k], h, R) for k in range(4)])
    got = lf.ghost_ray_light_factors(rays)
    assert got.shape == (len(rays), len(lights)) and got.dtype == np.float32
    for k, (kind, g, _, ar) in enumerate(lights):
        factor, inside, _ = pkg.light_geom_factors(kind, g, ar, rays)
        if kind == DIRECTIONAL:     # (v_sqrt_f32 on the device, a correctly rounded root on the host: tests/test_gpu_near_lights.py)
            assert np.abs(got[:, k].astype(np.float64) - factor).max() <= 4 * 2.0 ** -23, k
            continue
        assert np.array_equal(got[:, k], factor), k
        if kind == AREA:
            assert set(np.unique(got[:, k])) == {0.0, 1.0}, k
            want, sure = inside64(g, rays)
            assert np.array_equal((got[:, k] > 0)[sure], want[sure]), k


# ---- 2. the primary image -------------------------------------------------------------------------------------------------
def test_primary_image_of_a_rectangle_is_the_sum_over_the_oracles_exit_rays(pkg, lf, mask):
    W, H, spp, key = 80, 48, 64, 0xA5E2
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    lam = np.zeros((3, 3), np.float32)
    lam[1] = 1.0
    _setup(pkg, lf, lens, W, H, mask, lam)
    smp = _samples(pkg, lf, lens, W, H, spp, key, mask)
    alive = smp[:, 7] > 0
    rays = smp[:, :6].astype(np.float32)
    # rectangles small enough for their outline to cross the frame (80 pixels see 0.03 rad): 4 x 2.4 mm at 300 mm, and a tilted
    # parallelogram at 90 mm
    small = [((-1.0, 0.6, -300.0), (4.0, 0.0, 0.0), (0.0, 2.4, 0.0)), ((0.3, -0.2, -90.0), (1.2, 0.0, 0.4), (0.1, 0.8, 0.0))]
    for k in (0, 1):
        kind, g, rad, _ = light = (AREA, geom_of(small[k]), RAD, 0.0)
        got, hits = _primary(pkg, lf, [light], spp, key)
        assert _variant(lf) == 4 | 32 | 64
        inside, sure = inside64(g, rays)
        edge = alive & ~sure
        print(f"rectangle {k}: samples alive {alive.sum()} of {len(smp)}, inside {(alive & inside).sum()}, in the edge band {edge.sum()}")
        assert edge.sum() < 0.01 * alive.sum()
        rad64 = np.asarray(rad, np.float64)[None, None, :]
        want = np.where(alive & inside & sure, smp[:, 6], 0.0).reshape(H, W, spp).sum(2)[..., None] * rad64 / spp
        tol = np.where(edge, smp[:, 6], 0.0).reshape(H, W, spp).sum(2)[..., None] * rad64 / spp + 3 * 2.0 ** -36
        assert want.max() > 0 and 20 < (want[..., 0] > 0).sum() < W * H - 20          # (lit and unlit pixels: the outline is in the frame)
        err = np.abs(got - want)
        print(f"rectangle {k}: max |delta pixel| {err.max():.3e}, brightest {want.max():.3e}, lit pixels {(want[..., 0] > 0).sum()}")
        assert (err <= tol).all(), k
        assert hits >= (alive & inside & sure).sum()          # (rays_hit_light counts every wavelength's rays, the image shows one)
        # a hard outline: the point light at C is another image, and the rectangle seen from behind is black
        lamp, _ = _primary(pkg, lf, [(POINT, g[:3], rad, 0.05)], spp, key)
        assert not np.array_equal(lamp, got) and (np.abs(lamp - got) > tol).sum() > W * H          # (of 3 W H values)
        behind = (AREA, geom_of(small[k], (0.0, 0.0, -1.0)), RAD, 0.0)
        back, bhits = _primary(pkg, lf, [behind], spp, key)
        assert not back.any() and bhits == 0
        _install(lf, [behind])
        lf.set_ghost_pairs(None, True)
        black, cb = _frame(pkg, lf, spp, key, 0)
        assert not black.any() and cb["rays_hit_light"] == 0 and cb["rays_reached_scene"] > 0


# ---- 3. the whole sky -------------------------------------------------------------------------------------------------------
def test_the_whole_sky_lights_every_ray_that_leaves_the_lens(pkg, lf, mask):
    W, H, spp, key = 80, 48, 64, 0xA5E3
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    _install(lf, [_rect(3)])
    g, c = _frame(pkg, lf, spp, key, 1)
    assert c["rays_hit_light"] == c["rays_reached_scene"] > 0 and g.max() > 0
    assert lf.cull_reason() == "table_too_full" and not lf.cull_info()["culled"]


# ---- 4. the sum, in every kernel family -------------------------------------------------------------------------------------
def test_mixed_lights_are_the_sum_of_the_single_light_frames_in_every_kernel_family(pkg, lf, mask, forced):
    W, H, spp, key = 80, 48, 64, 0xA5E4
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    try:
        for name, bits, mode in (("path tree", 6, 0), ("culled", 6, 2), ("items", 0, 2)):
            lf.set_pupil_subcells(bits)
            _install(lf, MIXED)
            assert _variant(lf) == 4 | 32 | 64
            g, c = _frame(pkg, lf, spp, key, mode)
            assert lf.cull_info()["culled"] == (mode == 2), (name, lf.cull_reason())
            singles, hits = [], 0
            for light in MIXED:
                _install(lf, [light])
                assert _variant(lf) == {DIRECTIONAL: 0, POINT: 4 | 32, AREA: 4 | 32 | 64}[light[0]]
                s, cs = _frame(pkg, lf, spp, key, mode)
                assert lf.cull_info()["culled"] == (mode == 2), (name, lf.cull_reason())
                assert s.max() > 0
                singles.append(s)
                hits += cs["rays_hit_light"]
            assert np.array_equal(g, singles[0] + singles[1] + singles[2]), name
            assert c["rays_hit_light"] == hits, name
            if mode == 2:
                audit = lf.cull_audit()
                assert audit["rays"] > 0 and audit["lit"] == 0 and audit["launches_refuted"] == 0
    finally:
        lf.set_pupil_subcells(6)


# ---- 5. the cull table ------------------------------------------------------------------------------------------------------
def _moved(rect, to):
    return (tuple(to), rect[1], rect[2])


def test_culled_is_the_full_enumeration_for_rectangles_on_and_off_the_axis(pkg, mask, forced):
    W, H, spp, key = 80, 48, 64, 0xA5E5
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    ctx = pkg.LensFlare(0)
    try:
        _setup(pkg, ctx, lens, W, H, mask)
        for k in range(3):
            dist = -RECTS[k][0][2]
            for rect in (RECTS[k], _moved(RECTS[k], (0.0, 0.0, -dist))):
                _install(ctx, [(AREA, geom_of(rect), RAD, 0.0)])
                g2, c2 = _frame(pkg, ctx, spp, key, 2)
                assert ctx.cull_info()["culled"] and ctx.cull_reason() == "applied", (rect, ctx.cull_reason())
                audit = ctx.cull_audit()
                assert audit["rays"] > 0 and audit["lit"] == 0 and audit["launches_refuted"] == 0, (rect, audit)
                g0, c0 = _frame(pkg, ctx, spp, key, 0)
                assert not ctx.cull_info()["culled"]
                print(f"rectangle at {rect[0]}: started {ctx.cull_started_fraction():.4f}, hits {c0['rays_hit_light']}")
                assert np.array_equal(g2, g0) and c2["rays_hit_light"] == c0["rays_hit_light"] > 0, rect
    finally:
        ctx.close()


def test_a_rectangles_table_contains_its_centres_and_the_widening_is_needed(pkg, mask, forced):
    W, H, spp, key = 80, 48, 64, 0xA5E6
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    ctx = pkg.LensFlare(0)
    try:
        _setup(pkg, ctx, lens, W, H, mask)
        u = np.array([0.012, -0.007, -1.0])
        rect = _moved(RECTS[1], 90.0 * u / np.linalg.norm(u))          # the 90 mm rectangle, off the axis
        g = geom_of(rect)
        tables = {}
        for name, light in (("panel", (AREA, g, RAD, 0.0)), ("lamp", (POINT, g[:3], RAD, 0.03))):
            _install(ctx, [light])
            _frame(pkg, ctx, spp, key, 2)
            assert ctx.cull_info()["culled"], (name, ctx.cull_reason())
            tables[name] = ctx.cull_table()
        assert not (tables["lamp"] & ~tables["panel"]).any()
        assert (tables["panel"] & ~tables["lamp"]).any()
        _install(ctx, [(AREA, g, RAD, 0.0)])
        full, c0 = _frame(pkg, ctx, spp, key, 0)
        ctx.test_knob("cull_no_widening", 1)
        try:
            ctx.set_cull_audit(4)
            got, c = _frame(pkg, ctx, spp, key, 2)
            audit = ctx.cull_audit()
            print(f"not widened: audit {audit}, reason {ctx.cull_reason()}")
            assert audit["lit"] > 0 and ctx.cull_reason() == "audit_refuted" and not ctx.cull_info()["culled"]
            assert np.array_equal(got, full)              # (the refuted table is not used)
        finally:
            ctx.test_knob("cull_no_widening", 0)
            ctx.set_cull_audit(1)
        got, c = _frame(pkg, ctx, spp, key, 2)
        assert ctx.cull_info()["culled"] and np.array_equal(got, full) and ctx.cull_audit()["lit"] == 0
        # a table built without one of the lights is refuted too (cull_ignore_light)
        _install(ctx, [SUN, (AREA, g, RAD, 0.0)])
        both, _ = _frame(pkg, ctx, spp, key, 0)
        ctx.test_knob("cull_ignore_light", 1)
        try:
            ctx.set_cull_audit(4)
            got, _ = _frame(pkg, ctx, spp, key, 2)
            assert ctx.cull_audit()["lit"] > 0 and ctx.cull_reason() == "audit_refuted" and np.array_equal(got, both)
        finally:
            ctx.test_knob("cull_ignore_light", -1)
            ctx.set_cull_audit(1)
    finally:
        ctx.close()


# ---- 6. tiling --------------------------------------------------------------------------------------------------------------
def test_a_rectangle_is_its_two_halves(pkg, lf, mask):
    W, H, spp, key = 80, 48, 64, 0xA5E7
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    lam = np.zeros((3, 3), np.float32)
    lam[1] = 1.0
    _setup(pkg, lf, lens, W, H, mask, lam)
    C, e1, e2 = (np.asarray(x, np.float64) for x in RECTS[0])
    halves = [(AREA, geom_of((C + s * e1 / 4, e1 / 2, e2)), RAD, 0.0) for s in (-1, 1)]
    whole, hw = _primary(pkg, lf, [_rect(0)], spp, key)
    two, h2 = _primary(pkg, lf, halves, spp, key)
    smp = _samples(pkg, lf, lens, W, H, spp, key, mask)
    u, v, t, cd = uv64(geom_of(RECTS[0]), smp[:, :6].astype(np.float32))
    seam = (smp[:, 7] > 0) & (np.abs(u) < EDGE) & (np.abs(v) <= 0.5 + EDGE)
    tol = np.where(seam, smp[:, 6], 0.0).reshape(H, W, spp).sum(2)[..., None] * np.asarray(RAD)[None, None, :] / spp + 3 * 2.0 ** -36
    print(f"samples within {EDGE} of the seam: {seam.sum()}; hits {hw} and {h2}; pixels that differ {(whole != two).any(2).sum()}")
    assert whole.max() > 0 and (np.abs(whole - two) <= tol).all()
    lf.set_ghost_pairs(None, True)


# ---- 7. occlusion -------------------------------------------------------------------------------------------------------------
def test_occlusion_ends_the_shadow_ray_just_before_the_rectangle(pkg, lf, mask):
    W, H, spp, key = 80, 48, 64, 0xA5E8
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    z_ref = _z_ref_of(pkg, lens)
    _install(lf, [PANEL])
    free, cf = _frame(pkg, lf, spp, key, 0)
    assert free.max() > 0
    lf.set_scene([], _wall(z_ref, 200.0), [])
    lf.set_ghost_occlusion(True, WPM)
    try:
        with pytest.raises(pkg.LensFlareError) as e:          # the sky's reach: refused, as with a point light
            lf.trace_ghosts(spp, key)
        assert e.value.status == LF_ERR_STATE and "lf_set_ghost_occlusion_reach" in str(e.value)
        lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_LIGHT)
        assert _variant(lf) == 4 | 16 | 32 | 64
        g, c = _frame(pkg, lf, spp, key, 0)                    # a wall in front
        s = lf.ghost_occlusion_stats()
        assert not g.any() and c["rays_hit_light"] == 0 and s["tested"] == s["blocked"] == cf["rays_hit_light"]
        lf.set_scene([], _wall(z_ref, 400.0), [])              # a wall behind
        g, c = _frame(pkg, lf, spp, key, 0)
        assert np.array_equal(g, free) and c == cf and lf.ghost_occlusion_stats()["blocked"] == 0
        # a quad lying in the light's own plane -- the lamp's emissive mesh -- does not hide it
        lf.set_scene([], _quad(-0.1, 0.1, -0.1, 0.1, _plane_z(z_ref, 300.0)), [])
        g, c = _frame(pkg, lf, spp, key, 0)
        assert np.array_equal(g, free) and c == cf and lf.ghost_occlusion_stats()["blocked"] == 0
        # a half wall clips: the two halves of the wall share the rays between them
        parts, hits = [], 0
        for side in (0, 1):
            lf.set_scene([], _half(z_ref, 200.0, side), [])
            g, c = _frame(pkg, lf, spp, key, 0)
            assert 0 < c["rays_hit_light"] < cf["rays_hit_light"]
            parts.append(g)
            hits += c["rays_hit_light"]
        assert np.array_equal(parts[0] + parts[1], free) and hits == cf["rays_hit_light"]
        # mixed kinds under occlusion stay the sum
        lf.set_scene([], _half(z_ref, 60.0, 0), [])
        _install(lf, MIXED)
        g, c = _frame(pkg, lf, spp, key, 0)
        total = 0
        for light in MIXED:
            _install(lf, [light])
            total = total + _frame(pkg, lf, spp, key, 0)[0]
        assert np.array_equal(g, total) and g.max() > 0
    finally:
        lf.set_ghost_occlusion(False)
        lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_SKY)


def test_per_ray_light_visibility_is_the_float64_any_hit_over_the_reach(pkg, lf, mask):
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), 80)
    _setup(pkg, lf, lens, 80, 48, mask)
    z_ref = _z_ref_of(pkg, lens)
    spheres = [(0.034, -0.0072, _plane_z(z_ref, 600.0), 0.028), (-0.004, 0.003, _plane_z(z_ref, 60.0), 0.006)]
    quads = [(-0.2, 0.001, -0.2, 0.2, _plane_z(z_ref, 200.0))]
    lf.set_scene([s + ("d", 0.5, 0.5, 0.5) for s in spheres], [t for q in quads for t in _quad(*q)], [])
    lights = [_rect(0), _rect(2), SUN, LAMP]
    _install(lf, lights)
    lf.set_ghost_occlusion(True, WPM)
    lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_LIGHT)
    try:
        h, R = float(lens["semi_aperture"][0]), float(lens["radius"][0])
        rays = np.concatenate([area_rays(np.random.default_rng(0xA5E9 + k), 1024, RECTS[k], h, R) for k in (0, 2)])
        o, d = _map(rays, z_ref)
        vis = lf.ghost_ray_light_visibility(rays)
        assert vis.shape == (len(rays), 4)
        for k, (kind, g, _, _) in enumerate(lights):
            reach = pkg.ghost_shadow_reach_geom(kind, g, rays, WPM)
            blocked, sure = analytic(o, d, spheres, quads, reach)
            assert (~sure).sum() <= len(rays) // 100
            assert np.array_equal(vis[sure, k], ~blocked[sure]), k
            assert 0.05 * len(rays) <= vis[:, k].sum() <= 0.95 * len(rays), k
        assert (vis[:, 0] != vis[:, 1]).sum() > 0.02 * len(rays)       # (the sphere between the two rectangles)
    finally:
        lf.set_ghost_occlusion(False)
        lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_SKY)


# ---- 8. coated, stacked and filtered variants -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,bits", [("coated", 1), ("stacked", 1 | 8), ("bilinear", 2)])
def test_coated_stacked_and_filtered_variants(pkg, lf, mask, forced, variant, bits):
    W, H, spp, key = 64, 48, 64, 0xA5EA
    name = {"coated": "dgauss11_coated.lens", "stacked": "dgauss11_multicoated.lens", "bilinear": "dgauss11.lens"}[variant]
    lens = _crop(pkg.load_lens_file(name), W)
    _setup(pkg, lf, lens, W, H, mask)
    if variant == "bilinear":
        lf.set_mask_filter(pkg.MASK_BILINEAR)
    try:
        _install(lf, [PANEL, SUN])
        assert _variant(lf) == 4 | 32 | 64 | bits
        g2, c2 = _frame(pkg, lf, spp, key, 2)
        assert lf.cull_info()["culled"], lf.cull_reason()
        assert lf.cull_audit()["lit"] == 0
        g0, c0 = _frame(pkg, lf, spp, key, 0)
        assert np.array_equal(g2, g0) and c2["rays_hit_light"] == c0["rays_hit_light"] > 0
        _install(lf, [PANEL])
        panel, _ = _frame(pkg, lf, spp, key, 0)
        _install(lf, [SUN])
        sun, _ = _frame(pkg, lf, spp, key, 0)
        assert np.array_equal(g0, panel + sun) and panel.max() > 0 and sun.max() > 0
    finally:
        lf.set_mask_filter(pkg.MASK_NEAREST)
        lf.set_lens_coatings(None)
        lf.set_lens_coating_stacks(None)


# ---- 9. two contexts under the block deal -----------------------------------------------------------------------------------
def test_two_contexts_under_the_block_deal(pkg, mask, forced):
    W, H, spp, key = 130, 70, 16, 0xA5EB
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)

    def render(rank, n):
        ctx = pkg.LensFlare(0)
        try:
            _setup(pkg, ctx, lens, W, H, mask)
            _install(ctx, [PANEL, SUN])
            if n > 1:
                ctx.set_block_deal(rank, n)
            g, c = _frame(pkg, ctx, spp, key, 2)
            assert ctx.cull_info()["culled"], ctx.cull_reason()
            assert ctx.cull_audit()["lit"] == 0
            return g, c
        finally:
            ctx.close()

    want, wc = render(0, 1)
    bx = (W + 63) // 64
    yy, xx = np.mgrid[0:H, 0:W]
    owner = ((yy // 64) * bx + xx // 64) % 2
    got, hits = np.zeros_like(want), 0
    for r in range(2):
        g, c = render(r, 2)
        got[owner == r] = g[owner == r]
        hits += c["rays_hit_light"]
    assert np.array_equal(got, want) and want.max() > 0 and hits == wc["rays_hit_light"]


# ---- 10. from the scene -----------------------------------------------------------------------------------------------------
def test_lights_from_the_scene(pkg, mask):
    W, H = 80, 48
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    ctx = pkg.LensFlare(0)
    try:
        _setup(pkg, ctx, lens, W, H, mask)
        th = 0.3
        c2w = np.array([[np.cos(th), 0.0, np.sin(th)], [0.0, 1.0, 0.0], [-np.sin(th), 0.0, np.cos(th)]])
        pos = np.array([0.4, -0.2, 1.5])
        ctx.set_camera(c2w.reshape(-1), pos, 40.0, 27.0)
        ctx.set_lens_camera(1, WPM, 1.0)
        z_ref = ctx.lens_camera()["entrance_pupil_z_mm"]
        ctx.set_lens_camera(0)
        # camera space, world units: a lamp, a panel in front (centre, direction, dim_x, dim_y) and one behind the camera
        lamp_cam = np.array([0.02, 0.01, -0.5])
        panel_cam = np.array([[-0.05, 0.03, -2.0], [0.0, -0.6, 0.8], [0.5, 0.0, 0.0], [0.0, 0.3, 0.1]])
        behind_cam = panel_cam * np.array([[1, 1, -1], [1, 1, 1], [1, 1, 1], [1, 1, 1]])
        to_world = lambda v: v @ c2w.T          # noqa: E731
        panel_w = np.concatenate([pos + to_world(panel_cam[0]), to_world(panel_cam[1]), to_world(panel_cam[2]), to_world(panel_cam[3])])
        behind_w = np.concatenate([pos + to_world(behind_cam[0]), to_world(behind_cam[1]), to_world(behind_cam[2]), to_world(behind_cam[3])])
        lamp_w = pos + to_world(lamp_cam)
        to_sun = c2w @ np.array([0.5, 0.3, -10.0])
        rgb = [(1.0, 0.8, 0.6), (0.2, 0.9, 0.4), (0.3, 0.3, 1.0)]
        ctx.set_scene([(0.0, 0.0, -50.0, 1.0, "d", 0.5, 0.5, 0.5)], [], [(0, *to_sun, 1.0, 1.0, 1.0)])
        ctx.set_scene_lights([[0, 1.0, 1.0, 1.0, *to_sun, 0, 0, 0, 0, 0, 0, 0, 0, 0], [1, *rgb[0], *lamp_w, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                              [3, *rgb[1], *panel_w], [3, *rgb[2], *behind_w]])
        ctx.find_sun_pos([[*to_sun, 2.0, 1.5, 1.0]])
        assert ctx.set_lights_from_scene(0.0, 0.04, WPM) == (1, 1)
        old = ctx.lights_geom()
        assert list(old[0]) == [DIRECTIONAL, POINT] and not old[1][:, 3:].any()
        nd, npt, na = ctx.set_lights_from_scene_ex(0.0, 0.04, WPM)
        assert (nd, npt, na) == (1, 1, 1)                       # (the panel behind the camera is skipped)
        kinds, geoms, rads, ars = ctx.lights_geom()
        assert list(kinds) == [DIRECTIONAL, POINT, AREA] and list(ars) == [np.float32(0.04), np.float32(0.04), 0.0]
        assert all(np.array_equal(a[:2], b) for a, b in zip((kinds, geoms, rads, ars), old))
        # the forward mapping: c2w^T (p - pos) / wpm + (0, 0, z_ref); c2w^T v; c2w^T v / wpm -- summed in the library's order
        back = lambda w: np.array([(c2w[0, c] * w[0] + c2w[1, c] * w[1]) + c2w[2, c] * w[2] for c in range(3)])      # noqa: E731
        want = np.concatenate([back(panel_w[:3] - pos) / WPM + [0, 0, z_ref], back(panel_w[3:6]), back(panel_w[6:9]) / WPM, back(panel_w[9:]) / WPM])
        assert np.allclose(want[:3], panel_cam[0] / WPM + [0, 0, z_ref], rtol=0, atol=1e-9)
        assert np.allclose(want[6:], np.concatenate([panel_cam[2], panel_cam[3]]) / WPM, rtol=0, atol=1e-9)
        n = want[3:6] / np.linalg.norm(want[3:6])
        assert np.array_equal(geoms[2, :3], want[:3].astype(np.float32)) and np.array_equal(geoms[2, 6:], want[6:].astype(np.float32))
        assert np.abs(geoms[2, 3:6] - n).max() <= 1e-7
        assert np.array_equal(rads[2], np.asarray(rgb[1], np.float32))
        # lf_get_lights_ex: kind 2 with its centre; lf_get_lights: the unit vector from the front vertex to the centre
        k3, v3, _, a3 = ctx.lights_ex()
        assert list(k3) == [DIRECTIONAL, POINT, AREA] and np.array_equal(v3[2], geoms[2, :3]) and a3[2] == 0.0
        assert np.abs(ctx.lights()[0][2] - want[:3] / np.linalg.norm(want[:3])).max() <= 1e-7
        # the getter round-trips through the setter
        ctx.set_lights_geom(kinds, geoms, rads, ars)
        assert all(np.array_equal(a, b) for a, b in zip(ctx.lights_geom(), (kinds, geoms, rads, ars)))
        # too many lights: refused, nothing installed
        ctx.set_scene_lights([[3, *rgb[1], *panel_w]] * 8)
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.set_lights_from_scene_ex(0.0, 0.04, WPM)
        assert e.value.status == LF_ERR_INVALID and "LF_MAX_LIGHTS" in str(e.value)
        assert np.array_equal(ctx.lights_geom()[1], geoms)
    finally:
        ctx.close()


# ---- 11. lifecycle and refusals -------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals(pkg, mask):
    W, H, spp, key = 80, 48, 64, 0xA5EC
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    ctx = pkg.LensFlare(0)
    try:
        ctx.set_frame(W, H)
        with pytest.raises(pkg.LensFlareError) as e:          # (before a lens: the limits are the lens's)
            _install(ctx, [PANEL])
        assert e.value.status == LF_ERR_STATE
        _setup(pkg, ctx, lens, W, H, mask)
        _install(ctx, [PANEL, SUN])
        before = ctx.lights_geom()
        ctx.set_frame(W, H)
        assert all(np.array_equal(x, y) for x, y in zip(before, ctx.lights_geom())) and _variant(ctx) == 4 | 32 | 64
        # refusals leave the lights installed; the three-float call knows no kind 2
        close = geom_of(_moved(RECTS[0], (0.0, 0.0, -20.0)))
        flat = geom_of((RECTS[0][0], RECTS[0][1], RECTS[0][1]))
        for bad in ([(AREA, close, RAD, 0.0)], [(AREA, flat, RAD, 0.0)], [(3, PANEL[1], RAD, 0.0)], [PANEL] * 9,
                    [SUN, (AREA, PANEL[1], [-1.0, 0.0, 0.0], 0.0)]):
            with pytest.raises(pkg.LensFlareError) as e:
                _install(ctx, bad)
            assert e.value.status == LF_ERR_INVALID
            assert all(np.array_equal(x, y) for x, y in zip(before, ctx.lights_geom()))
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.set_lights_ex([AREA], [[0.0, 0.0, -300.0]], [RAD], [0.03])
        assert e.value.status == LF_ERR_INVALID and "LF_LIGHT_POINT (1)" in str(e.value)
        assert all(np.array_equal(x, y) for x, y in zip(before, ctx.lights_geom()))
        # lf_set_lights clears the area light
        ctx.set_lights([SUN[1]], [SUN[2]], [SUN[3]])
        assert list(ctx.lights_geom()[0]) == [DIRECTIONAL] and _variant(ctx) == 0
        # a lens whose front element comes too close: lf_set_lens keeps the lights, the launch refuses until they fit again
        h0, R0 = float(lens["semi_aperture"][0]), abs(float(lens["radius"][0]))
        r_f = float(np.hypot(h0, R0 - np.sqrt(R0 * R0 - h0 * h0)))
        near = geom_of(((0.0, 0.0, -4.6 * r_f), (10.0, 0.0, 0.0), (0.0, 10.0, 0.0)))
        _install(ctx, [(AREA, near, RAD, 0.0)])
        ctx.trace_ghosts(spp, key)
        big = dict(lens)
        big["semi_aperture"] = np.array(lens["semi_aperture"], np.float32)
        big["semi_aperture"][0] = 1.3 * lens["semi_aperture"][0]
        ctx.set_lens(big)
        assert list(ctx.lights_geom()[0]) == [AREA]
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.trace_ghosts(spp, key)
        assert e.value.status == LF_ERR_STATE and "r_f" in str(e.value)
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.ghost_ray_light_factors(np.array([[0, 0, 0, 0, 0, -1]], np.float32))
        assert e.value.status == LF_ERR_STATE
        ctx.set_lens(lens)
        ctx.trace_ghosts(spp, key)
    finally:
        ctx.close()


def test_a_context_without_an_area_light_is_the_parents(pkg, lf, mask, forced):
    """lf_set_lights_geom with kinds 0 and 1 IS lf_set_lights_ex: the same stored state, the same march_variant, the same
    launches per kernel family (lf_timing_get) and the same frames, bit for bit -- and one directional light's frame is the
    CPU oracle's, as the parent commit's is."""
    W, H, spp, key = 80, 48, 64, 0xA5ED
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    names = ("march", "cull_prepass", "cull_audit")          # (the cached tree of the pre-pass is light-independent: built once)
    lf.timing_enable(True)
    try:
        for lights, variant in (([SUN], 0), ([SUN, LAMP], 4 | 32), ([SUN, (DIRECTIONAL, [0.0, 0.01, -1.0], RAD, 0.02)], 4)):
            out = []
            for geom in (False, True):
                if geom:
                    _install(lf, lights)
                else:
                    lf.set_lights_ex([l[0] for l in lights], [l[1] for l in lights], [l[2] for l in lights], [l[3] for l in lights])
                assert _variant(lf) == variant
                stored = lf.lights_geom()
                lf.timing_reset()
                g0, c0 = _frame(pkg, lf, spp, key, 0)
                g2, c2 = _frame(pkg, lf, spp, key, 2)
                assert np.array_equal(g0, g2)
                out.append((stored, g0, c0, c2, [lf.timing_get(n)[0] for n in names]))
            a, b = out
            assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and not a[0][1][:, 3:].any()
            assert np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] and a[4] == b[4] and a[1].max() > 0
        _install(lf, [SUN])
        g0, _ = _frame(pkg, lf, spp, key, 0)
        lfo.geo_follow_device(lf)
        try:
            want = lfo.geo_trace(lens, W, H, 0, H, spp, key, None, True, mask, SUN[1], SUN[2], SUN[3], cull=None)[0]
        finally:
            lfo.geo_follow_device(None)
        assert np.array_equal(g0, want)
    finally:
        lf.timing_enable(False)
