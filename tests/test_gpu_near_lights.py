"""Lens ghosts for lights at a finite distance (lf_set_lights_ex, LF_LIGHT_POINT; lens-flare_amd/csrc: lf_point_lobe_q /
lf_point_pretest in lf_march_events.h, light_admits_at / lights_pretest / lights_epilogue<VAR & kVarNear> in
lf_march_common.h, k_cull_audit_near and the widened radius in lf_cull_prepass.hip, k_ghost_ray_light_factors in
lf_march.hip): every ray that has left the front element is tested against the direction from ITS OWN exit point to the
light.  The reference's ghosts know only `angle_to_sun`.

Contributions are unsigned 64-bit fixed-point integers, so the identities here are bit for bit: spp is a power of two and
`bits` 36 throughout (checked), a frame is acc 2^-36 / spp and sums of frames are exact in float64 (sums below 2^53).
The bar on |delta (1 - q)^2| is tests/test_near_lights_cpu.py's, derived there: 8e-7 / alpha + 1.9e-6."""
import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo
from test_near_lights_cpu import bar_of, q64, stored_direction, EDGE, DELTA_THETA

pytestmark = pytest.mark.gpu
RAD = [1.0, 0.9, 0.5]
RAD2 = [0.5, 1.0, 0.8]
RAD3 = [0.7, 0.4, 1.0]
MASK = "pentbig500_14.png"
WPM = 0.001
DIRECTIONAL, POINT = 0, 1
LF_ERR_INVALID, LF_ERR_STATE = 1, 4
# (kind, vector, radiance, angular radius)
SUN = (DIRECTIONAL, [0.012, 0.004, -1.0], RAD, 0.03)
LAMP = (POINT, [-3.0, 2.0, -300.0], RAD2, 0.03)
LAMP2 = (POINT, [1.5, -1.0, -90.0], RAD3, 0.05)
MIXED = [SUN, LAMP, LAMP2]


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


def _r_f(lens):
    h, R = float(lens["semi_aperture"][0]), abs(float(lens["radius"][0]))
    sag = 0.0 if R == 0 else (R - np.sqrt(R * R - h * h) if h < R else R)
    return float(np.sqrt(h * h + sag * sag))


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
    lf.set_lights_ex([l[0] for l in lights], [l[1] for l in lights], [l[2] for l in lights], [l[3] for l in lights])


def _frame(pkg, lf, spp, key, mode):
    lf.set_march_culling(mode)
    lf.reset_counters()
    lf.trace_ghosts(spp, key)
    assert lf.march_fix_bits() == 36
    return lf.read_buffer(pkg.GHOST_BUFFER), lf.counters()


def _variant(lf):
    return lf.get_ghost_occlusion()["march_variant"]


# ---- 1. per ray ---------------------------------------------------------------------------------------------------------
def test_per_ray_factors_are_the_host_function_and_the_float64_expression(pkg, lf, mask):
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), 80)
    _setup(pkg, lf, lens, 80, 48, mask)
    lights = [LAMP, LAMP2, (POINT, [20.0, -12.0, -1000.0], RAD, 0.1), SUN]
    _install(lf, lights)
    assert _variant(lf) == 4 | 32
    rng = np.random.default_rng(0x9EA1)
    n = 2048
    h, R = float(lens["semi_aperture"][0]), float(lens["radius"][0])
    rho, phi = h * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    P = np.stack([rho * np.cos(phi), rho * np.sin(phi), R - np.sqrt(R * R - rho * rho)], 1)
    # each ray looks at one of the lights (from its own exit point) within 1.6 lobe radii
    which = rng.integers(0, len(lights), n)
    s = np.zeros((n, 3))
    alpha = np.zeros(n)
    for k, (kind, vec, _, ar) in enumerate(lights):
        m = which == k
        s[m] = (np.asarray(vec, np.float64)[None, :] - P[m]) if kind == POINT else np.asarray(vec, np.float64)[None, :]
        alpha[m] = ar
    s /= np.linalg.norm(s, axis=1)[:, None]
    a = np.cross(s, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a, axis=1)[:, None]
    b = np.cross(s, a)
    ang, psi = 1.6 * alpha * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    d = np.cos(ang)[:, None] * s + np.sin(ang)[:, None] * (np.cos(psi)[:, None] * a + np.sin(psi)[:, None] * b)
    rays = np.concatenate([P, d], 1).astype(np.float32)
    got = lf.ghost_ray_light_factors(rays)
    assert got.shape == (n, len(lights)) and got.dtype == np.float32
    for k, (kind, vec, _, ar) in enumerate(lights):
        q, inside = pkg.light_lobe_factors(kind, vec, ar, rays)
        host = np.where(inside, (np.float32(1.0) - q) * (np.float32(1.0) - q), np.float32(0.0)).astype(np.float32)
        if kind == POINT:
            # the same definition: bit for bit
            assert np.array_equal(got[:, k], host), k
        else:
            # a directional light's root is v_sqrt_f32 on the device (1 ulp), correctly rounded on the host: q to 2 ulp,
            # (1 - q)^2 to 2 * 2 ulp(1) absolutely -- and the same rays inside, away from the edge
            assert np.abs(got[:, k].astype(np.float64) - host).max() <= 4 * 2.0 ** -23, k
        v32 = np.asarray(vec, np.float32) if kind == POINT else stored_direction(vec)
        want, _ = q64(kind, v32, ar, rays)
        sure = np.abs(want - 1.0) >= EDGE
        assert (~sure).sum() <= n // 100
        assert np.array_equal((got[:, k] > 0)[sure], (want < 1.0)[sure]), k
        err = np.abs(got[:, k] - np.where(want < 1.0, (1.0 - want) ** 2, 0.0))[sure]
        print(f"light {k}: inside {(want < 1.0).sum()} of {n}, max |delta (1 - q)^2| {err.max():.3e} (bar {bar_of(ar):.3e})")
        assert err.max() <= bar_of(ar), (k, err.max())
        assert 0.02 * n < (want < 1.0).sum() < 0.9 * n
    # a wrong mapping is another answer on the rays the float64 expression is sure about (light 1: 90 mm away)
    kind, vec, _, ar = lights[1]
    right, _ = q64(kind, np.asarray(vec, np.float32), ar, rays)
    front_zv_dropped = rays * np.array([1, 1, 0, 1, 1, 1], np.float32)       # (z = front_zv + hz: without it hz's sag is lost too)
    for name, mr in (("exit point dropped", rays * np.array([0, 0, 0, 1, 1, 1], np.float32)), ("z dropped", front_zv_dropped),
                     ("x flipped", rays * np.array([-1, 1, 1, 1, 1, 1], np.float32)),
                     ("y flipped", rays * np.array([1, -1, 1, 1, 1, 1], np.float32))):
        wrong, _ = q64(kind, np.asarray(vec, np.float32), ar, mr)
        ok = (np.abs(right - 1.0) >= EDGE) & (np.abs(wrong - 1.0) >= EDGE)
        assert not np.array_equal((got[:, 1] > 0)[ok], (wrong < 1.0)[ok]), name


# ---- 2. the primary path of a whole small frame, independent of the march -------------------------------------------------
def test_primary_image_of_a_lamp_is_the_sum_over_the_oracles_exit_rays(pkg, lf, mask):
    """The primary path alone is the difference of two launches under one key (the sums are integers): {pair (0, 1), primary}
    minus {pair (0, 1)}.  One wavelength: lambda_rgb zero but for wavelength 1.  lfo.geo_lens_samples gives every sample's
    exit ray and weight as the march computes them; weight x (1 - q)^2 x radiance, summed in float64 numpy with the float64
    textbook q, must be the device's pixel within bar(alpha) x the pixel's mean weight x radiance (+ the fixed-point grid)."""
    W, H, spp, key = 80, 48, 64, 0x9EA2
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    lam = np.zeros((3, 3), np.float32)
    lam[1] = 1.0
    _setup(pkg, lf, lens, W, H, mask, lam)
    kind, vec, rad, ar = LAMP
    _install(lf, [LAMP])
    lf.set_ghost_pairs([(0, 1)], True)
    with_primary, _ = _frame(pkg, lf, spp, key, 0)
    lf.set_ghost_pairs([(0, 1)], False)
    without, _ = _frame(pkg, lf, spp, key, 0)
    got = with_primary - without
    lfo.geo_follow_device(lf)
    try:
        smp = lfo.geo_lens_samples(lens, W, H, spp, key, 1, np.arange(W * H), mask).astype(np.float64)
    finally:
        lfo.geo_follow_device(None)
    smp = smp.reshape(W * H * spp, 8)
    alive = smp[:, 7] > 0
    q, _ = q64(POINT, np.asarray(vec, np.float32), ar, smp[:, :6].astype(np.float32))
    edge = alive & (np.abs(q - 1.0) < EDGE)
    print(f"samples alive {alive.sum()} of {len(smp)}, within {EDGE} of the lobe's edge {edge.sum()}")
    assert edge.sum() < 0.01 * alive.sum()
    f = np.where(alive & (q < 1.0), smp[:, 6] * (1.0 - q) ** 2, 0.0).reshape(H, W, spp)
    want = f.sum(2)[..., None] * np.asarray(rad, np.float32).astype(np.float64)[None, None, :] / spp
    mean_w = np.where(alive, smp[:, 6], 0.0).reshape(H, W, spp).sum(2) / spp
    # (an edge sample adds at most EDGE^2 of its weight; each contribution is truncated to the 2^-36 grid)
    tol = (bar_of(ar) + EDGE * EDGE) * mean_w[..., None] * max(rad) + 3 * 2.0 ** -36
    assert want.max() > 0
    py, px = np.unravel_index(np.argmax(want[..., 0]), (H, W))
    y0, x0 = min(max(py - 8, 0), H - 16), min(max(px - 8, 0), W - 16)
    win = (slice(y0, y0 + 16), slice(x0, x0 + 16))
    err = np.abs(got - want)
    print(f"window at ({x0}, {y0}): max err {err[win].max():.3e}, tol there {tol[win].min():.3e}; frame max err / tol {(err / tol).max():.3f}")
    assert (err[win] <= tol[win]).all() and want[win].min() > 0
    assert (err <= tol).all()
    # ... and it is not the directional light of the same direction: at 300 mm the two images differ by far more than the bar
    _install(lf, [(DIRECTIONAL, vec, rad, ar)])
    lf.set_ghost_pairs([(0, 1)], True)
    a, _ = _frame(pkg, lf, spp, key, 0)
    lf.set_ghost_pairs([(0, 1)], False)
    b, _ = _frame(pkg, lf, spp, key, 0)
    assert (np.abs((a - b) - want) > 100 * tol).any()


# ---- 3. focus ------------------------------------------------------------------------------------------------------------
def _moments(g):
    img = g[..., 0]
    ys, xs = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    t = img.sum()
    cx, cy = (img * xs).sum() / t, (img * ys).sum() / t
    return cx, cy, (img * ((xs - cx) ** 2 + (ys - cy) ** 2)).sum() / t


def test_a_lamp_is_sharpest_when_the_lens_is_focused_on_it(pkg, mask):
    """thinlens.lens stopped down to a semi-aperture a = 3 mm, a lamp on the axis D = 300 mm in front, alpha = 8 mrad.
    Paraxially, with m the image scale (lf_paraxial_image_scale: mm on the sensor per radian) at each sensor position: a
    pixel's rays leave towards ONE object point when the lens is focused at D and in ONE direction when at infinity, so
      lamp, focused at D:   the lobe alone, radius m_D alpha           second moment (m_D alpha)^2 / 4   [(1 - q)^2 profile]
      lamp, at infinity:    the lobe spread by the pupil's parallax a / D:  m_0^2 (alpha^2 / 4 + (a / D)^2 / 2)
      sun,  at infinity:    (m_0 alpha)^2 / 4  -- SMALLER than the focused lamp's by (m_0 / m_D)^2: the image scale grows
      sun,  focused at D:   m_D^2 (alpha^2 / 4 + (a / D)^2 / 2)
    The ordering and, within 15 % (an f/8 singlet's spherical aberration, the pupil's cos^4 weighting and the pixel grid are
    per cent each), the values are asserted; the centroid is the frame's centre to one pixel."""
    W, H, spp, key = 80, 48, 64, 0x9EA3
    D, a, alpha = 300.0, 3.0, 0.008
    lens = _crop(pkg.load_lens_file("thinlens.lens"), W, pitch_of=720)      # (a 4 mm x 2.4 mm sensor)
    lens["semi_aperture"] = np.array([a, a], np.float32)
    pitch = lens["sensor_width_mm"] / W
    ctx = pkg.LensFlare(0)
    try:
        _setup(pkg, ctx, lens, W, H, np.ones((8, 8), np.float32))
        ctx.set_ghost_pairs([(0, 1)], True)
        got, scale = {}, {}
        for focus in (D, 0.0):
            t_last = ctx.focus_lens(focus)
            moved = dict(lens)
            moved["thickness"] = np.array([lens["thickness"][0], t_last], np.float32)
            scale[focus] = pkg.paraxial_image_scale(moved)
            for name, light in (("lamp", (POINT, [0.0, 0.0, -D], RAD, alpha)), ("sun", (DIRECTIONAL, [0.0, 0.0, -1.0], RAD, alpha))):
                _install(ctx, [light])
                ctx.set_ghost_pairs([(0, 1)], True)
                with_primary, _ = _frame(pkg, ctx, spp, key, 0)
                ctx.set_ghost_pairs([(0, 1)], False)
                without, _ = _frame(pkg, ctx, spp, key, 0)
                got[name, focus] = _moments(with_primary - without)
        lobe, spread = alpha ** 2 / 4.0, (a / D) ** 2 / 2.0
        want = {("lamp", D): scale[D] ** 2 * lobe, ("lamp", 0.0): scale[0.0] ** 2 * (lobe + spread),
                ("sun", 0.0): scale[0.0] ** 2 * lobe, ("sun", D): scale[D] ** 2 * (lobe + spread)}
        for k in want:
            cx, cy, m2 = got[k]
            print(f"{k}: centroid ({cx:.2f}, {cy:.2f}) second moment {m2 * pitch * pitch:.4f} mm^2, paraxial {want[k]:.4f} mm^2")
        for k in want:
            cx, cy, m2 = got[k]
            assert abs(cx - (W - 1) / 2) <= 1.0 and abs(cy - (H - 1) / 2) <= 1.0, k
            assert abs(m2 * pitch * pitch / want[k] - 1.0) <= 0.15, (k, m2 * pitch * pitch, want[k])
        assert scale[D] > scale[0.0] > 0
        assert got["lamp", D][2] < got["lamp", 0.0][2]
        assert got["lamp", D][2] < got["sun", D][2]
        assert got["sun", 0.0][2] < got["lamp", D][2]          # (the paraxial model says otherwise: the image scale)
    finally:
        ctx.close()


# ---- 4. the sum, in every kernel family -------------------------------------------------------------------------------------
def test_mixed_lights_are_the_sum_of_the_single_light_frames_in_every_kernel_family(pkg, lf, mask, forced):
    W, H, spp, key = 80, 48, 64, 0x9EA4
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    try:
        for name, bits, mode in (("path tree", 6, 0), ("culled", 6, 2), ("items", 0, 2)):
            lf.set_pupil_subcells(bits)
            _install(lf, MIXED)
            assert _variant(lf) == 4 | 32
            g, c = _frame(pkg, lf, spp, key, mode)
            assert lf.cull_info()["culled"] == (mode == 2), (name, lf.cull_reason())
            singles, hits = [], 0
            for light in MIXED:
                _install(lf, [light])
                assert _variant(lf) == (4 | 32 if light[0] == POINT else 0)
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


# ---- 5. the far limit ---------------------------------------------------------------------------------------------------------
def test_a_lamp_ten_kilometres_away_is_the_sun(pkg, lf, mask):
    """|L| = 1e7 mm.  Per sample the factor differs from the directional light's by the two evaluations' float error (the bar)
    and by the parallax r_f / (|L| - r_f) = 1.3e-6 rad of the exit point, which enters as delta_theta does (tests/
    test_near_lights_cpu.py): |delta pixel| <= bar(alpha; delta_theta + parallax) x the most a pixel can weigh.  Ghost pairs
    and the primary path, every pixel."""
    W, H, spp, key = 80, 48, 64, 0x9EA5
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    kind, d, rad, ar = SUN
    u = stored_direction(d).astype(np.float64)
    _install(lf, [SUN])
    sun, cs = _frame(pkg, lf, spp, key, 0)
    _install(lf, [(POINT, (1e7 * u).astype(np.float32), rad, ar)])
    lamp, cl = _frame(pkg, lf, spp, key, 0)
    parallax = _r_f(lens) / (1e7 - _r_f(lens))
    bar = bar_of(ar, DELTA_THETA + parallax)
    # A pixel channel is (1 / spp) sum over its samples, the 46 paths and the wavelengths of weight x factor x radiance x
    # lambda_rgb (the default weights: wavelength c carries channel c alone).  |delta factor| <= bar per contribution and a
    # weight is at most geom_norm, the start weight (the range contract's bound: Fresnel and the mask only lower it):
    #     |delta pixel| <= bar x geom_norm x paths x max radiance.
    h, zs = float(lens["semi_aperture"][-1]), float(lens["thickness"][-1])
    geom_norm = np.pi * h * h / (zs * zs)
    per_pixel = bar * geom_norm * 46 * max(rad)
    err = np.abs(sun - lamp).max()
    print(f"max |delta pixel| {err:.3e} (bound {per_pixel:.3e}, brightest pixel {sun.max():.3e}), hits {cs['rays_hit_light']} {cl['rays_hit_light']}")
    assert sun.max() > per_pixel                # (a bound over ALL paths: loose on a pixel few paths reach, but below the image)
    assert err <= per_pixel
    # the rays whose answer the parallax can turn lie within it of the lobe's edge: 2 parallax / alpha of the lit ones, were
    # they spread evenly over the lobe -- ten times that is allowed
    assert abs(cl["rays_hit_light"] - cs["rays_hit_light"]) <= 10 * (2 * parallax / ar) * cs["rays_hit_light"] + 10
    assert {k: v for k, v in cl.items() if k != "rays_hit_light"} == {k: v for k, v in cs.items() if k != "rays_hit_light"}


# ---- 6. the cull table ----------------------------------------------------------------------------------------------------------
def _positions(lens):
    r = _r_f(lens)
    out = []
    for dist in (4.5 * r, 20.0 * r, 1000.0):
        out.append((0.0, 0.0, -dist))
        u = np.array([0.012, -0.007, -1.0])
        out.append(tuple(dist * u / np.linalg.norm(u)))
    return out


def test_culled_is_the_full_enumeration_for_lamps_near_and_far(pkg, mask, forced):
    W, H, spp, key = 80, 48, 64, 0x9EA6
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    ctx = pkg.LensFlare(0)
    try:
        _setup(pkg, ctx, lens, W, H, mask)
        for pos in _positions(lens):
            _install(ctx, [(POINT, pos, RAD, 0.03)])
            g2, c2 = _frame(pkg, ctx, spp, key, 2)
            assert ctx.cull_info()["culled"] and ctx.cull_reason() == "applied", (pos, ctx.cull_reason())
            audit = ctx.cull_audit()
            assert audit["rays"] > 0 and audit["lit"] == 0 and audit["launches_refuted"] == 0, (pos, audit)
            g0, c0 = _frame(pkg, ctx, spp, key, 0)
            assert not ctx.cull_info()["culled"]
            print(f"lamp at {np.round(pos, 1)}: started {ctx.cull_started_fraction():.4f}, hits {c0['rays_hit_light']}")
            assert np.array_equal(g2, g0) and c2["rays_hit_light"] == c0["rays_hit_light"] > 0, pos
    finally:
        ctx.close()


def test_a_lamps_table_contains_the_suns_and_the_widening_is_needed(pkg, mask, forced):
    """The table of a lamp is the table of the sun unit(L) with a wider radius: it contains it and differs from it.  Without the
    widening (lf_test_knob cull_no_widening: a table wrong by construction) a lamp 4.5 r_f in front of the lens loses light:
    the audit finds lit rays in dropped boxes and refutes the table -- the launch marches everything."""
    W, H, spp, key = 80, 48, 64, 0x9EA7
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    r = _r_f(lens)
    ctx = pkg.LensFlare(0)
    try:
        _setup(pkg, ctx, lens, W, H, mask)
        u = np.array([0.012, -0.007, -1.0])
        pos = 4.5 * r * u / np.linalg.norm(u)
        tables = {}
        for name, light in (("lamp", (POINT, pos, RAD, 0.03)), ("sun", (DIRECTIONAL, pos, RAD, 0.03))):
            _install(ctx, [light])
            _frame(pkg, ctx, spp, key, 2)
            assert ctx.cull_info()["culled"], (name, ctx.cull_reason())
            tables[name] = ctx.cull_table()
        assert not (tables["sun"] & ~tables["lamp"]).any()
        assert (tables["lamp"] & ~tables["sun"]).any()
        _install(ctx, [(POINT, pos, RAD, 0.03)])
        full, c0 = _frame(pkg, ctx, spp, key, 0)
        ctx.test_knob("cull_no_widening", 1)
        try:
            ctx.set_cull_audit(4)
            g, c = _frame(pkg, ctx, spp, key, 2)
            audit = ctx.cull_audit()
            print(f"not widened: audit {audit}, reason {ctx.cull_reason()}")
            assert audit["lit"] > 0 and ctx.cull_reason() == "audit_refuted" and not ctx.cull_info()["culled"]
            assert np.array_equal(g, full)              # (the refuted table is not used)
        finally:
            ctx.test_knob("cull_no_widening", 0)
            ctx.set_cull_audit(1)
        g, c = _frame(pkg, ctx, spp, key, 2)
        assert ctx.cull_info()["culled"] and np.array_equal(g, full) and ctx.cull_audit()["lit"] == 0
    finally:
        ctx.close()


# ---- 7. occlusion -------------------------------------------------------------------------------------------------------------
def test_occlusion_with_a_point_light_is_refused(pkg, lf, mask):
    """kVarNear | kVarOccl (a closest-hit walk against the light's distance) is not built: the launch says so, and names the way
    out; directional lights under occlusion, and point lights without it, launch as ever"""
    W, H, spp, key = 80, 48, 64, 0x9EA8
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    lf.set_scene([(0.0, 0.0, -5.0, 0.01, "d", 0.5, 0.5, 0.5)], [], [])
    _install(lf, [LAMP])
    free, _ = _frame(pkg, lf, spp, key, 0)
    lf.set_ghost_occlusion(True, WPM)
    try:
        with pytest.raises(pkg.LensFlareError) as e:
            lf.trace_ghosts(spp, key)
        assert e.value.status == LF_ERR_STATE and "point light" in str(e.value) and "lf_set_ghost_occlusion" in str(e.value)
        _install(lf, [SUN])
        assert _variant(lf) == 4 | 16
        lf.trace_ghosts(spp, key)
    finally:
        lf.set_ghost_occlusion(False)
    _install(lf, [LAMP])
    again, _ = _frame(pkg, lf, spp, key, 0)
    assert np.array_equal(again, free) and free.max() > 0


# ---- 8. coated, stacked and filtered variants -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,bits", [("coated", 1), ("stacked", 1 | 8), ("bilinear", 2)])
def test_coated_stacked_and_filtered_variants(pkg, lf, mask, forced, variant, bits):
    W, H, spp, key = 64, 48, 64, 0x9EA9
    name = {"coated": "dgauss11_coated.lens", "stacked": "dgauss11_multicoated.lens", "bilinear": "dgauss11.lens"}[variant]
    lens = _crop(pkg.load_lens_file(name), W)
    _setup(pkg, lf, lens, W, H, mask)
    if variant == "bilinear":
        lf.set_mask_filter(pkg.MASK_BILINEAR)
    try:
        _install(lf, [LAMP, SUN])
        assert _variant(lf) == 4 | 32 | bits
        g2, c2 = _frame(pkg, lf, spp, key, 2)
        assert lf.cull_info()["culled"], lf.cull_reason()
        assert lf.cull_audit()["lit"] == 0
        g0, c0 = _frame(pkg, lf, spp, key, 0)
        assert np.array_equal(g2, g0) and c2["rays_hit_light"] == c0["rays_hit_light"] > 0
        _install(lf, [LAMP])
        lamp, _ = _frame(pkg, lf, spp, key, 0)
        _install(lf, [SUN])
        sun, _ = _frame(pkg, lf, spp, key, 0)
        assert np.array_equal(g0, lamp + sun) and lamp.max() > 0 and sun.max() > 0
    finally:
        lf.set_mask_filter(pkg.MASK_NEAREST)
        lf.set_lens_coatings(None)
        lf.set_lens_coating_stacks(None)


# ---- 9. two contexts under the block deal -----------------------------------------------------------------------------------
def test_two_contexts_under_the_block_deal(pkg, mask, forced):
    W, H, spp, key = 130, 70, 16, 0x9EAA
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)

    def render(rank, n):
        ctx = pkg.LensFlare(0)
        try:
            _setup(pkg, ctx, lens, W, H, mask)
            _install(ctx, [LAMP, SUN])
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
        lamps_cam = np.array([[0.02, 0.01, -0.5], [-0.05, 0.03, -2.0], [0.0, 0.0, 0.4]])      # (camera space, world units; the last: behind)
        world = pos[None, :] + lamps_cam @ c2w.T
        to_sun = c2w @ np.array([0.5, 0.3, -10.0])        # (dirToLight of a directional light the camera looks at)
        rgb = [(1.0, 0.8, 0.6), (0.2, 0.9, 0.4), (1.0, 1.0, 1.0)]
        ctx.set_scene([(0.0, 0.0, -50.0, 1.0, "d", 0.5, 0.5, 0.5)], [],
                      [(0, *to_sun, 1.0, 1.0, 1.0)] + [(1, *world[i], *rgb[i]) for i in range(3)])
        ctx.find_sun_pos([[*to_sun, 2.0, 1.5, 1.0]])
        n_flares = ctx.set_lights_from_flares(0.0, 0.04)
        d_flares, r_flares, _ = ctx.lights()
        nd, npt = ctx.set_lights_from_scene(0.0, 0.04, WPM)
        assert (nd, npt) == (n_flares, 2) and nd == 1
        kinds, vecs, rads, ars = ctx.lights_ex()
        assert list(kinds) == [DIRECTIONAL, POINT, POINT] and np.allclose(ars, 0.04)
        assert np.array_equal(vecs[0], d_flares[0]) and np.array_equal(rads[0], r_flares[0])
        w = world[:2] - pos[None, :]                       # c2w^T (p - pos) / wpm + (0, 0, z_ref), summed in the library's order
        want = np.stack([((c2w[0, c] * w[:, 0] + c2w[1, c] * w[:, 1]) + c2w[2, c] * w[:, 2]) / WPM for c in range(3)], 1)
        want[:, 2] += z_ref
        assert np.allclose(want, lamps_cam[:2] / WPM + [0, 0, z_ref], rtol=0, atol=1e-9)
        assert np.array_equal(vecs[1:], want.astype(np.float32))
        assert np.array_equal(rads[1:], np.asarray(rgb[:2], np.float32))
        # lf_get_lights: a point light as the unit vector from the front vertex
        d, r, a = ctx.lights()
        un = want / np.linalg.norm(want, axis=1)[:, None]
        assert np.abs(d[1:] - un).max() <= 1e-7
        # the getter round-trips through the setter
        ctx.set_lights_ex(kinds, vecs, rads, ars)
        k2, v2, r2, a2 = ctx.lights_ex()
        assert np.array_equal(k2, kinds) and np.array_equal(v2, vecs) and np.array_equal(r2, rads) and np.array_equal(a2, ars)
        # too many lights: refused, nothing installed
        ctx.set_scene_lights([[1, *rgb[0], *world[0], 0, 0, 0, 0, 0, 0, 0, 0, 0]] * 8)
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.set_lights_from_scene(0.0, 0.04, WPM)
        assert e.value.status == LF_ERR_INVALID and "LF_MAX_LIGHTS" in str(e.value)
        assert np.array_equal(ctx.lights_ex()[1], vecs)
    finally:
        ctx.close()


# ---- 11. lifecycle and refusals -------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals(pkg, mask):
    W, H, spp, key = 80, 48, 64, 0x9EAB
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    ctx = pkg.LensFlare(0)
    try:
        ctx.set_frame(W, H)
        with pytest.raises(pkg.LensFlareError) as e:          # (before a lens: the limits are the lens's)
            _install(ctx, [LAMP])
        assert e.value.status == LF_ERR_STATE
        _setup(pkg, ctx, lens, W, H, mask)
        _install(ctx, [LAMP, SUN])
        before = ctx.lights_ex()
        ctx.set_frame(W, H)                                    # the lights survive lf_set_frame
        after = ctx.lights_ex()
        assert all(np.array_equal(x, y) for x, y in zip(before, after)) and _variant(ctx) == 4 | 32
        # refusals leave the lights installed
        r = _r_f(lens)
        for bad in ([(POINT, [0.0, 0.0, -3.9 * r], RAD, 0.03)], [(POINT, [0.0, 0.0, 100.0], RAD, 0.03)], [(2, [0.0, 0.0, -300.0], RAD, 0.03)],
                    [(POINT, [np.nan, 0.0, -300.0], RAD, 0.03)], [LAMP] * 9, [(POINT, [0.0, 0.0, -300.0], RAD, 0.0)],
                    [SUN, (POINT, [0.0, 0.0, -300.0], [-1.0, 0.0, 0.0], 0.03)]):
            with pytest.raises(pkg.LensFlareError) as e:
                _install(ctx, bad)
            assert e.value.status == LF_ERR_INVALID
            assert all(np.array_equal(x, y) for x, y in zip(before, ctx.lights_ex()))
        with pytest.raises(pkg.LensFlareError) as e:
            _install(ctx, [(POINT, [0.0, 0.0, -3.9 * r], RAD, 0.03)])
        assert "r_f" in str(e.value) and "4 r_f" in str(e.value)
        lib = ctx.lib
        z3, z1 = (np.zeros(3, np.float32), np.zeros(1, np.float32))
        fp = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)        # noqa: E731
        ki = np.zeros(1, np.int32)
        assert lib.lf_set_lights_ex(ctx.ctx, 1, None, fp(z3), fp(z3), fp(z1)) == LF_ERR_INVALID
        assert lib.lf_set_lights_ex(ctx.ctx, 1, fp(ki), None, fp(z3), fp(z1)) == LF_ERR_INVALID
        assert lib.lf_set_lights_ex(ctx.ctx, 1, fp(ki), fp(z3), None, fp(z1)) == LF_ERR_INVALID
        assert lib.lf_set_lights_ex(ctx.ctx, 1, fp(ki), fp(z3), fp(z3), None) == LF_ERR_INVALID
        assert lib.lf_ghost_ray_light_factors(ctx.ctx, 4, None, None) == LF_ERR_INVALID
        # lf_set_lights clears the point lights
        ctx.set_lights([SUN[1]], [SUN[2]], [SUN[3]])
        assert list(ctx.lights_ex()[0]) == [DIRECTIONAL] and _variant(ctx) == 0
        # a lens whose front element comes too close: lf_set_lens keeps the lights, the launch refuses until they fit again
        _install(ctx, [(POINT, [0.0, 0.0, -4.5 * r], RAD, 0.03)])
        ctx.trace_ghosts(spp, key)
        big = dict(lens)
        big["semi_aperture"] = np.array(lens["semi_aperture"], np.float32)
        big["semi_aperture"][0] = 1.3 * lens["semi_aperture"][0]
        ctx.set_lens(big)
        assert list(ctx.lights_ex()[0]) == [POINT]
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


# ---- 12. off is the parent ----------------------------------------------------------------------------------------------------
def test_a_context_without_point_lights_is_the_parents(pkg, lf, mask, forced):
    """The variants a context without point lights reports are the ones it reported before (0 for one light, 4 for several,
    | 16 under occlusion), lf_set_lights_ex with every kind 0 IS lf_set_lights, and the frames of 1 and 3 directional lights
    are the parent commit's, by the multi-light identities (the oracle's single-light frames, summed) -- the kernels launched are
    the parent's, instruction for instruction (profiles/near_light_resources.txt)."""
    W, H, spp, key = 80, 48, 64, 0x9EAC
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    three = [([0.012, 0.004, -1.0], RAD, 0.03), ([-0.014, -0.006, -1.0], RAD2, 0.05), ([0.0, 0.01, -1.0], RAD3, 0.02)]
    lfo.geo_follow_device(lf)
    try:
        for lights in (three[:1], three):
            lf.set_lights([l[0] for l in lights], [l[1] for l in lights], [l[2] for l in lights])
            assert _variant(lf) == (0 if len(lights) == 1 else 4)
            stored = lf.lights()
            g0, c0 = _frame(pkg, lf, spp, key, 0)
            g2, c2 = _frame(pkg, lf, spp, key, 2)
            assert lf.cull_info()["culled"]
            _install(lf, [(DIRECTIONAL,) + l for l in lights])
            assert _variant(lf) == (0 if len(lights) == 1 else 4)
            assert all(np.array_equal(x, y) for x, y in zip(stored, lf.lights()))
            e0, ce = _frame(pkg, lf, spp, key, 0)
            assert np.array_equal(e0, g0) and np.array_equal(g2, g0) and ce == c0
            want = sum(lfo.geo_trace(lens, W, H, 0, H, spp, key, None, True, mask, l[0], l[1], l[2], cull=None)[0] for l in lights)
            assert np.array_equal(g0, want) and want.max() > 0
    finally:
        lfo.geo_follow_device(None)
