"""Ghost occlusion (lf_set_ghost_occlusion; lens-flare_amd/csrc: ghost_ray_visible / lights_epilogue<VAR & kVarOccl> in
lf_march_common.h, the walk of lf_scene_walk.h, k_ghost_ray_visibility in lf_march.hip): a lit ghost ray adds what it added
only if the scene does not block its shadow ray -- its own exit point on the front element along its own exit direction,
mapped to the world as the lens camera maps its primary rays.  The reference's ghosts know no occluder.

Contributions are unsigned 64-bit fixed-point integers, so every identity here is bit for bit: spp is a power of two and
`bits` 36 throughout (checked), a frame is acc 2^-36 / spp and sums of frames are exact in float64 (sums below 2^53)."""
import numpy as np
import pytest

from goldenlib import load_texels

pytestmark = pytest.mark.gpu
RAD = [1.0, 0.9, 0.5]
RAD2 = [0.5, 1.0, 0.8]
MASK = "pentbig500_14.png"
WPM = 0.001
LF_ERR_INVALID, LF_ERR_STATE = 1, 4
TWO = [([0.012, 0.004, -1.0], RAD, 0.03), ([-0.014, -0.006, -1.0], RAD2, 0.05)]
AXIS = [([0.0, 0.0, -1.0], RAD, 0.05)]


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


def _install(lf, lights):
    lf.set_lights([l[0] for l in lights], [l[1] for l in lights], [l[2] for l in lights])


def _frame(pkg, lf, spp, key, mode):
    lf.set_march_culling(mode)
    lf.reset_counters()
    lf.trace_ghosts(spp, key)
    assert lf.march_fix_bits() == 36
    return lf.read_buffer(pkg.GHOST_BUFFER), lf.counters(), lf.ghost_occlusion_stats()


def _z_ref(lf):
    """the paraxial entrance pupil's z, as lf_get_lens_camera reports it"""
    lf.set_lens_camera(1, WPM, 1.0)
    try:
        return lf.lens_camera()["entrance_pupil_z_mm"]
    finally:
        lf.set_lens_camera(0)


def _quad(x0, x1, y0, y1, z):
    """two triangles over [x0, x1] x [y0, y1] of the world plane z, as set_scene's rows"""
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    n = (0.0, 0.0, 1.0)
    row = lambda p, q, r: tuple(p + q + r + n + n + n) + ("d", 0.5, 0.5, 0.5)      # noqa: E731
    return [row(a, b, c), row(a, c, d)]


def _plane_z(lf, mm_in_front):
    """world z of the lens-space plane `mm_in_front` millimetres in front of the first vertex (identity pose at the origin)"""
    return (-mm_in_front - _z_ref(lf)) * WPM


# ---- per ray ------------------------------------------------------------------------------------------------------------
def _map(rays, z_ref, wpm=WPM, flip=(1.0, 1.0), drop_zref=False):
    """the contract's mapping in float64 for the identity pose at the origin: world origins and unit directions"""
    r = np.asarray(rays, np.float32).astype(np.float64)
    o = np.stack([flip[0] * r[:, 0] * wpm, flip[1] * r[:, 1] * wpm, (r[:, 2] - (0.0 if drop_zref else z_ref)) * wpm], 1)
    d = r[:, 3:] * np.array([flip[0], flip[1], 1.0])
    return o, d / np.sqrt((d * d).sum(1))[:, None]


SPHERE = (0.02, -0.01, -0.35, 0.03)
QUAD = (-0.10, 0.01, -0.02, 0.09, -0.8)


def _analytic(o, d):
    """(hit, margin) of the world rays against SPHERE and QUAD in float64; margin = the smallest distance to a silhouette in
    discriminant (relative to b^2) / barycentric terms"""
    c, R = np.array(SPHERE[:3]), SPHERE[3]
    oc = o - c
    b = (oc * d).sum(1)
    disc = b * b - ((oc * oc).sum(1) - R * R)
    hit_s = (disc > 0) & (-b + np.sqrt(np.maximum(disc, 0)) > 0)
    m_s = np.abs(disc) / np.maximum(b * b, 1e-300)
    x0, x1, y0, y1, z = QUAD
    t = (z - o[:, 2]) / d[:, 2]
    u = (o[:, 0] + t * d[:, 0] - x0) / (x1 - x0)
    v = (o[:, 1] + t * d[:, 1] - y0) / (y1 - y0)
    hit_q = (t > 0) & (u > 0) & (u < 1) & (v > 0) & (v < 1)
    m_q = np.minimum.reduce([np.abs(u), np.abs(1 - u), np.abs(v), np.abs(1 - v), np.abs(u - v)])      # (u = v: the shared diagonal)
    return hit_s | hit_q, np.minimum(m_s, m_q)


def test_per_ray_visibility_is_the_scene_trace_and_the_analytic_test(pkg, lf, mask):
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), 80)
    _setup(pkg, lf, lens, 80, 48, mask)
    x0, x1, y0, y1, z = QUAD
    lf.set_scene([SPHERE + ("d", 0.5, 0.5, 0.5)], _quad(x0, x1, y0, y1, z), [])
    lf.set_ghost_occlusion(True, WPM)
    z_ref = _z_ref(lf)
    assert abs(z_ref) > 1.0          # (the double Gauss: ~ +20 mm; a mapping without it is another mapping)
    rng = np.random.default_rng(0x0CC1)
    n = 2048
    h = float(lens["semi_aperture"][0])
    rho, phi = h * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    ang, psi = 0.1 * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    rays = np.stack([rho * np.cos(phi), rho * np.sin(phi), np.zeros(n),
                     np.sin(ang) * np.cos(psi), np.sin(ang) * np.sin(psi), -np.cos(ang)], 1).astype(np.float32)
    vis = lf.ghost_ray_visibility(rays)
    o, d = _map(rays, z_ref)
    hit, margin = _analytic(o, d)
    sure = margin >= 1e-9
    assert (~sure).sum() <= n // 100
    assert 0.05 * n < hit.sum() < 0.95 * n          # (both answers occur, often)
    assert np.array_equal(vis[sure], ~hit[sure])
    traced = np.array([lf.scene_trace_ray(o[i], d[i])["hit"] for i in range(n)])
    assert np.array_equal(vis, ~traced)
    # a wrong mapping is another answer: x or y flipped, z_ref dropped, wpm squared
    for kw in (dict(flip=(-1.0, 1.0)), dict(flip=(1.0, -1.0)), dict(drop_zref=True), dict(wpm=WPM * WPM)):
        ho, hd = _map(rays, z_ref, **kw)
        wrong, wm = _analytic(ho, hd)
        ok = sure & (wm >= 1e-9)
        assert not np.array_equal(vis[ok], ~wrong[ok]), kw


# ---- frames ---------------------------------------------------------------------------------------------------------------
def _blocker(lf, lens, shift_widths=0.0):
    """a quad 2.2 x the front element's clear diameter wide, 0.1 mm in front of the first vertex"""
    half = 2.2 * float(lens["semi_aperture"][0]) * WPM
    dx = shift_widths * 2.0 * half
    return _quad(-half + dx, half + dx, -half, half, _plane_z(lf, 0.1))


def test_a_wall_on_the_front_element_blocks_everything(pkg, lf, mask):
    W, H, spp, key = 80, 48, 64, 0x0C01
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    _install(lf, AXIS)
    g0, c0, s0 = _frame(pkg, lf, spp, key, 0)
    assert g0.max() > 0 and c0["rays_hit_light"] > 0 and s0 == dict(tested=0, blocked=0)
    lf.set_scene([], _blocker(lf, lens), [])
    lf.set_ghost_occlusion(True, WPM)
    g, c, s = _frame(pkg, lf, spp, key, 0)
    assert not g.any() and c["rays_hit_light"] == 0
    assert s["tested"] == s["blocked"] == c0["rays_hit_light"]
    assert {k: v for k, v in c.items() if k != "rays_hit_light"} == {k: v for k, v in c0.items() if k != "rays_hit_light"}


@pytest.mark.parametrize("scene", ["beside", "behind"])
def test_what_the_rays_cannot_meet_blocks_nothing(pkg, mask, forced, scene):
    W, H, spp, key = 96, 64, 64, 0x0C02
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    ctx = pkg.LensFlare(0)
    try:
        _setup(pkg, ctx, lens, W, H, mask)
        _install(ctx, [([0.012, 0.004, -1.0], RAD, 0.02)])
        g0, c0, _ = _frame(pkg, ctx, spp, key, 2)
        assert ctx.cull_info()["culled"], ctx.cull_reason()
        t0, a0, e0 = ctx.cull_table(), ctx.cull_audit(), ctx.executed_events() if hasattr(ctx, "executed_events") else None
        if scene == "beside":
            ctx.set_scene([], _blocker(ctx, lens, shift_widths=3.0), [])
        else:
            ctx.set_scene([(0.0, 0.0, 5.0, 1.0, "d", 0.5, 0.5, 0.5)], _quad(-9.0, 9.0, -9.0, 9.0, 0.5), [])
        ctx.set_ghost_occlusion(True, WPM)
        assert ctx.get_ghost_occlusion()["march_variant"] & 16
        g, c, s = _frame(pkg, ctx, spp, key, 2)
        assert ctx.cull_info()["culled"]
        assert np.array_equal(g, g0) and c == c0 and g0.max() > 0
        assert s["blocked"] == 0 and s["tested"] == c0["rays_hit_light"] > 0
        assert np.array_equal(ctx.cull_table(), t0) and ctx.cull_audit() == a0
        if e0 is not None:
            assert ctx.executed_events() == e0
    finally:
        ctx.close()


def test_a_sphere_in_front_of_one_light_leaves_the_other_lights_frame(pkg, lf, mask):
    W, H, spp, key = 80, 48, 64, 0x0C03
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    lights = [([0.10, 0.05, -1.0], RAD, 0.02), ([-0.10, 0.05, -1.0], RAD2, 0.02)]
    singles = []
    for l in lights:
        _install(lf, [l])
        singles.append(_frame(pkg, lf, spp, key, 0)[0])
    print("single-light sums:", [float(s.sum()) for s in singles])
    assert singles[0].max() > 0 and singles[1].max() > 0 and not np.array_equal(singles[0], singles[1])
    _install(lf, lights)
    lf.set_ghost_occlusion(True, WPM)
    dist = 10.0
    R = dist * 0.05 + float(lens["semi_aperture"][0]) * WPM
    for hidden in (0, 1):
        v = np.array(lights[hidden][0])
        c = dist * v / np.sqrt((v * v).sum())
        lf.set_scene([(c[0], c[1], c[2], R, "d", 0.5, 0.5, 0.5)], [], [])
        g, _, s = _frame(pkg, lf, spp, key, 0)
        assert np.array_equal(g, singles[1 - hidden]), hidden
        assert 0 < s["blocked"] < s["tested"]
    # (a flipped axis puts the sphere over the other light: the frames above would be swapped)


def _halves(lf, lens, where):
    """the half planes x < 0 and x > 0, sharing the edge x = 0: 1 mm in front of the lens, or 100 m away"""
    if where == "near":
        z, L = _plane_z(lf, 1.0), 10.0 * float(lens["semi_aperture"][0]) * WPM
    else:
        z, L = -100.0, 50.0
    return _quad(-L, 0.0, -L, L, z), _quad(0.0, L, -L, L, z)


def _complement(pkg, lf, lens, spp, key, mode, where):
    lf.set_ghost_occlusion(False)
    g0, c0, _ = _frame(pkg, lf, spp, key, mode)
    assert g0.max() > 0
    lf.set_ghost_occlusion(True, WPM)
    parts = []
    for half in _halves(lf, lens, where):
        lf.set_scene([], half, [])
        parts.append(_frame(pkg, lf, spp, key, mode))
    (ga, ca, sa), (gb, cb, sb) = parts
    assert np.array_equal(ga + gb, g0)
    for g in (ga, gb):
        frac = g.sum() / g0.sum()
        print(where, "fraction of the unoccluded sum:", float(frac))
        assert 0.2 < frac < 0.8
    assert sa["tested"] == sb["tested"] == c0["rays_hit_light"]
    assert sa["blocked"] + sb["blocked"] == sa["tested"]
    assert ca["rays_hit_light"] + cb["rays_hit_light"] == c0["rays_hit_light"]
    return g0, c0


@pytest.mark.parametrize("where", ["near", "far"])
def test_two_half_planes_add_up_to_the_unoccluded_frame(pkg, lf, mask, where):
    W, H, spp, key = 80, 48, 64, 0x0C04
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    _install(lf, AXIS)
    _complement(pkg, lf, lens, spp, key, 0, where)


def test_a_far_occluder_off_the_axis_clips_by_the_rays_own_direction(pkg, lf, mask):
    """100 m away everything x > 1 m is covered: a ray of the on-axis light's lobe (0.05 rad) is blocked iff ITS direction
    leans more than 0.01 to +x -- a shadow ray along the light's direction would start within the front element's 3 cm of
    the axis and never get there"""
    W, H, spp, key = 80, 48, 64, 0x0C0A
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    _install(lf, AXIS)
    g0, c0, _ = _frame(pkg, lf, spp, key, 0)
    lf.set_ghost_occlusion(True, WPM)
    lf.set_scene([], _quad(1.0, 50.0, -50.0, 50.0, -100.0), [])
    ga, _, sa = _frame(pkg, lf, spp, key, 0)
    lf.set_scene([], _quad(-50.0, 1.0, -50.0, 50.0, -100.0), [])
    gb, _, sb = _frame(pkg, lf, spp, key, 0)
    assert np.array_equal(ga + gb, g0) and sa["blocked"] + sb["blocked"] == sa["tested"] == c0["rays_hit_light"]
    print("blocked of tested, x > 1 m at 100 m:", sa["blocked"], sa["tested"])
    assert 0.02 * sa["tested"] < sa["blocked"] < 0.5 * sa["tested"]
    assert 0 < ga.sum() < g0.sum() and 0 < gb.sum() < ga.sum()


def test_one_wavelength_of_three_is_the_single_wavelength_lens(pkg, lf, mask):
    """the shadow ray starts where THIS wavelength's re-marched ray left the lens: the frame of the three-wavelength lens with
    only its middle wavelength weighted is, under the same occluder, the frame of the lens that has that wavelength alone
    (which has no other wavelength's ray to start from)"""
    W, H, spp, key = 80, 48, 64, 0x0C0B
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    assert lens["ior"].shape[0] == 3
    alone = dict(lens)
    alone["ior"] = np.ascontiguousarray(lens["ior"][1:2])
    frames = []
    for l, w in ((alone, [[1.0, 1.0, 1.0]]), (lens, [[0.0] * 3, [1.0] * 3, [0.0] * 3])):
        _setup(pkg, lf, l, W, H, mask, w)
        _install(lf, AXIS)
        lf.set_scene([], _halves(lf, lens, "near")[0], [])
        row = [_frame(pkg, lf, spp, key, 0)[0]]
        lf.set_ghost_occlusion(True, WPM)
        g, _, s = _frame(pkg, lf, spp, key, 0)
        assert 0 < s["blocked"] < s["tested"]
        frames.append(row + [g])
    assert np.array_equal(frames[0][0], frames[1][0]) and frames[0][0].max() > 0      # (the premise, without occlusion)
    assert np.array_equal(frames[0][1], frames[1][1]) and 0 < frames[0][1].sum() < frames[0][0].sum()


def test_every_kernel_family_under_occlusion(pkg, lf, mask, forced):
    W, H, spp, key = 96, 64, 64, 0x0C05
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    _install(lf, TWO)
    lf.set_scene([], _halves(lf, lens, "near")[0], [])
    lf.set_ghost_occlusion(True, WPM)
    g0, c0, s0 = _frame(pkg, lf, spp, key, 0)
    assert g0.max() > 0 and 0 < s0["blocked"] < s0["tested"]
    try:
        for bits in (6, 0):      # 0: independent pixels, the compacted march (k_march_items)
            lf.set_pupil_subcells(bits)
            full, cf, sf = _frame(pkg, lf, spp, key, 0)
            assert not lf.cull_info()["culled"]
            g, c, s = _frame(pkg, lf, spp, key, 2)
            assert lf.cull_info()["culled"], lf.cull_reason()
            assert np.array_equal(g, full) and c["rays_hit_light"] == cf["rays_hit_light"] > 0 and s == sf, bits
            if bits == 6:
                assert np.array_equal(full, g0)
        lf.set_pupil_subcells(6)
        for knob in ("cull_no_prefix", "cull_weights_first"):
            lf.test_knob(knob, 1)
            try:
                g, c, s = _frame(pkg, lf, spp, key, 2)
            finally:
                lf.test_knob(knob, 0)
            assert lf.cull_info()["culled"]
            assert np.array_equal(g, g0) and c["rays_hit_light"] == c0["rays_hit_light"] and s == s0, knob
        # the K-light frame is the sum of the single-light frames under the same occlusion
        singles = []
        for l in TWO:
            _install(lf, [l])
            assert lf.get_ghost_occlusion()["march_variant"] & 20 == 20      # one light: the lights epilogue, a list of one
            singles.append(_frame(pkg, lf, spp, key, 2))
        assert np.array_equal(g0, singles[0][0] + singles[1][0]) and min(s[0].max() for s in singles) > 0
        assert s0["tested"] == sum(s[2]["tested"] for s in singles) and s0["blocked"] == sum(s[2]["blocked"] for s in singles)
    finally:
        lf.set_pupil_subcells(6)


def test_two_contexts_under_the_block_deal(pkg, mask, forced):
    W, H, spp, key = 130, 70, 16, 0x0C06
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    lights = [([0.02, 0.003, -1.0], RAD, 0.02), ([-0.02, -0.004, -1.0], RAD2, 0.03)]

    def render(rank, n):
        ctx = pkg.LensFlare(0)
        try:
            _setup(pkg, ctx, lens, W, H, mask)
            _install(ctx, lights)
            ctx.set_scene([], _halves(ctx, lens, "near")[0], [])
            ctx.set_ghost_occlusion(True, WPM)
            if n > 1:
                ctx.set_block_deal(rank, n)
            g, c, s = _frame(pkg, ctx, spp, key, 2)
            assert ctx.cull_info()["culled"], ctx.cull_reason()
            return g, c, s
        finally:
            ctx.close()

    want, wc, ws = render(0, 1)
    bx = (W + 63) // 64
    yy, xx = np.mgrid[0:H, 0:W]
    owner = ((yy // 64) * bx + xx // 64) % 2
    got, hits, tested, blocked = np.zeros_like(want), 0, 0, 0
    for r in range(2):
        g, c, s = render(r, 2)
        got[owner == r] = g[owner == r]
        hits += c["rays_hit_light"]; tested += s["tested"]; blocked += s["blocked"]
    assert np.array_equal(got, want) and want.max() > 0 and hits == wc["rays_hit_light"]
    assert (tested, blocked) == (ws["tested"], ws["blocked"]) and 0 < blocked < tested


@pytest.mark.parametrize("variant", ["coated", "stacked", "bilinear", "eight"])
def test_variants_combine_with_occlusion(pkg, lf, mask, forced, variant):
    W, H, spp, key = 96, 64, 64, 0x0C07
    name = dict(coated="dgauss11_coated.lens", stacked="dgauss11_multicoated.lens", eight="dgauss11_8lambda.lens").get(variant, "dgauss11.lens")
    lens = _crop(pkg.load_lens_file(name), W)
    lam = pkg.spectral_weights(lens["lambda_nm"])[0] if variant == "eight" else None
    _setup(pkg, lf, lens, W, H, mask, lam)
    if variant == "bilinear":
        lf.set_mask_filter(pkg.MASK_BILINEAR)
    try:
        _install(lf, AXIS)
        want = dict(coated=1, stacked=9, bilinear=2, eight=0)[variant]
        lf.set_ghost_occlusion(True, WPM)
        assert lf.get_ghost_occlusion()["march_variant"] == 20 | want
        g0, c0 = _complement(pkg, lf, lens, spp, key, 2, "near")
        assert lf.cull_info()["culled"]
        # ... and an occluder no ray can meet changes nothing
        lf.set_scene([], _blocker(lf, lens, shift_widths=3.0), [])
        g, c, s = _frame(pkg, lf, spp, key, 2)
        assert np.array_equal(g, g0) and c == c0 and s["blocked"] == 0 and s["tested"] == c0["rays_hit_light"]
    finally:
        lf.set_mask_filter(pkg.MASK_NEAREST)
        lf.set_lens_coatings(None)
        lf.set_lens_coating_stacks(None)
        lf.set_ghost_occlusion(False)


def test_lifecycle_and_refusals(pkg, mask):
    W, H, spp, key = 80, 48, 64, 0x0C08
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    ctx = pkg.LensFlare(0)
    try:
        assert ctx.get_ghost_occlusion() == dict(on=False, world_per_mm=0.001, march_variant=0)
        ctx.set_frame(W, H)
        ctx.set_aperture(pkg.APERTURE_STARBURST, mask)
        ctx.set_lens(lens)
        _install(ctx, AXIS)
        # refusals of the setter (through the library, not the wrapper's own check): the previous state stays
        ctx.set_ghost_occlusion(True, 0.002)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            import ctypes as C
            assert ctx.lib.lf_set_ghost_occlusion(ctx.ctx, 1, C.c_double(bad)) == LF_ERR_INVALID
            with pytest.raises(ValueError):
                ctx.set_ghost_occlusion(True, bad)
            assert ctx.get_ghost_occlusion()["on"] and ctx.get_ghost_occlusion()["world_per_mm"] == 0.002
        ctx.set_ghost_occlusion(True, WPM)
        # no camera, no scene: LF_ERR_STATE, and the message names what is missing
        for call in (lambda: ctx.trace_ghosts(spp, key), lambda: ctx.ghost_ray_visibility(np.array([[0, 0, 0, 0, 0, -1.0]]))):
            with pytest.raises(pkg.LensFlareError) as e:
                call()
            assert e.value.status == LF_ERR_STATE and "lf_set_camera" in str(e.value) and "lf_set_scene" in str(e.value)
        ctx.set_camera(np.eye(3).reshape(-1), [0.0, 0.0, 0.0], 40.0, 27.0)
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.trace_ghosts(spp, key)
        assert e.value.status == LF_ERR_STATE and "lf_set_camera" not in str(e.value) and "lf_set_scene" in str(e.value)
        # off: the launch needs neither
        ctx.set_ghost_occlusion(False)
        g0, c0, _ = _frame(pkg, ctx, spp, key, 0)
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.ghost_ray_visibility(np.array([[0, 0, 0, 0, 0, -1.0]]))
        assert e.value.status == LF_ERR_STATE
        # on, off and on again; the scene replaced and the camera moved between launches
        left, right = _halves(ctx, lens, "near")
        ctx.set_scene([], left, [])
        ctx.set_ghost_occlusion(True, WPM)
        ga, _, sa = _frame(pkg, ctx, spp, key, 0)
        ctx.set_ghost_occlusion(False)
        g, c, s = _frame(pkg, ctx, spp, key, 0)
        assert np.array_equal(g, g0) and c == c0 and s == dict(tested=0, blocked=0)
        ctx.set_ghost_occlusion(True, WPM)
        assert np.array_equal(_frame(pkg, ctx, spp, key, 0)[0], ga)
        ctx.set_scene([], right, [])
        gb, _, sb = _frame(pkg, ctx, spp, key, 0)
        assert np.array_equal(ga + gb, g0) and sa["blocked"] + sb["blocked"] == sa["tested"] and 0 < sa["blocked"] < sa["tested"]
        # the camera turned half round about y: the right half plane now stands where the left one stood
        ctx.set_camera(np.diag([-1.0, 1.0, -1.0]).reshape(-1), [0.0, 0.0, 0.0], 40.0, 27.0)
        zc = _plane_z(ctx, 1.0)
        L = 10.0 * float(lens["semi_aperture"][0]) * WPM
        ctx.set_scene([], _quad(0.0, L, -L, L, -zc), [])
        assert np.array_equal(_frame(pkg, ctx, spp, key, 0)[0], ga)
        ctx.set_camera(np.eye(3).reshape(-1), [0.0, 0.0, 0.0], 40.0, 27.0)
        ctx.set_scene([], left, [])
        # the setting survives set_lens, set_lights and set_frame
        ctx.set_lens(lens)
        _install(ctx, AXIS)
        ctx.set_frame(W, H)
        ctx.set_aperture(pkg.APERTURE_STARBURST, mask)
        assert ctx.get_ghost_occlusion() == dict(on=True, world_per_mm=WPM, march_variant=20)
        assert np.array_equal(_frame(pkg, ctx, spp, key, 0)[0], ga)
    finally:
        ctx.close()


def test_a_wall_in_front_of_the_sun_through_the_host_mirror(pkg, mask, tmp_path):
    """shim_demo geowall: lfamd::PathTracer::use_ghost_occlusion -> lf_frame_plan::ghost_occlusion -> lf_run_frame"""
    import os
    import re
    import subprocess
    demo = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lens-flare_amd", "host", "shim_demo")
    assert os.path.exists(demo), "run __graft_entry__.build() first"
    W, H, spp = 80, 48, 64
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    n, nl = lens["n"], lens["ior"].shape[0]
    with open(tmp_path / "lens.txt", "w") as f:
        f.write(f"{n} {lens['stop']} {nl} {lens['sensor_width_mm']!r}\n")
        for k in range(n):
            row = [lens["radius"][k], lens["thickness"][k], lens["semi_aperture"][k]] + [lens["ior"][l, k] for l in range(nl)]
            f.write(" ".join(repr(float(v)) for v in row) + "\n")
    mask.tofile(tmp_path / "mask.f32")
    frames, stats = [], []
    for wall in (0, 1, 2):
        out = str(tmp_path / f"w{wall}")
        run = subprocess.run([demo, "geowall", str(tmp_path / "lens.txt"), str(tmp_path / "mask.f32"), str(mask.shape[1]), str(mask.shape[0]),
                              str(W), str(H), str(spp), "0.01", "0.005", "-1.0", "0.02", out, str(wall)], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        frames.append(np.fromfile(out + ".ghost.f64", np.float64).reshape(H, W, 3))
        stats.append(tuple(map(int, re.search(r"shadow tests (\d+) blocked (\d+)", run.stdout).groups())))
    assert frames[0].max() > 0 and stats[0] == (0, 0)
    assert not frames[1].any() and stats[1][0] == stats[1][1] > 0
    assert 0 < stats[2][1] < stats[2][0] == stats[1][0]
    assert 0.2 < frames[2].sum() / frames[0].sum() < 0.8 and (frames[2] <= frames[0]).all()


def test_off_is_the_parent(pkg, mask, forced):
    """with a scene installed and occlusion off the launch is the one of a context that never saw a scene, through the
    kernels it always took: the variant carries neither the occlusion bit nor, with one light, the lights bit"""
    W, H, spp, key = 96, 64, 64, 0x0C09
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    out = []
    for with_scene in (False, True):
        ctx = pkg.LensFlare(0)
        try:
            _setup(pkg, ctx, lens, W, H, mask)
            if with_scene:
                ctx.set_scene([], _halves(ctx, lens, "near")[0], [])
                ctx.set_ghost_occlusion(True, WPM)
                ctx.set_ghost_occlusion(False)
            res = []
            for lights in (AXIS, TWO):
                _install(ctx, lights)
                assert ctx.get_ghost_occlusion()["march_variant"] == (4 if len(lights) > 1 else 0)
                for mode in (0, 2):
                    res.append(_frame(pkg, ctx, spp, key, mode))
                    assert ctx.cull_info()["culled"] == (mode == 2)
            out.append(res)
        finally:
            ctx.close()
    for (g, c, s), (g1, c1, s1) in zip(*out):
        assert np.array_equal(g, g1) and c == c1 and s == s1 == dict(tested=0, blocked=0) and g.max() > 0
