"""Single-layer anti-reflection coatings on the device (lf_set_lens_coatings): transmission known-answer tests through
lf_generate_lens_rays against float64 closed forms, ghost ratios through lf_trace_ghosts, geometry untouched by a film
(counters, events, cull table, audit bit for bit), invariance, kernel agreement and the coatings' lifecycle.  The float32
CPU oracle does not follow coated frames: these tests pin them instead."""
import math
import os

import numpy as np
import pytest

from goldenlib import load_texels
from test_coatings_cpu import airy64

pytestmark = pytest.mark.gpu
LAMBDAS = (656.3, 587.6, 486.1)
MGF2 = 1.38
SUN_NS = (0.521445, 0.517156)     # bench.py: where the c3 frame's sun lands


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="module")
def lf(pkg):
    ctx = pkg.LensFlare(0)
    ctx.set_frame(64, 64)
    ctx.set_aperture(pkg.APERTURE_STARBURST, np.ones((4, 4), np.float32))
    yield ctx
    ctx.close()


def _plate(n, h=500.0, t=(5.0, 20.0), stop=False):
    """a flat glass plate of index n in air (interfaces air -> glass, glass -> air), sensor in air; stop=True puts an open
    stop in front of it (interface 0)"""
    radius = np.zeros(3 if stop else 2, np.float32)
    th = np.array(([2.0] if stop else []) + list(t), np.float32)
    ior = np.array([([1.0] if stop else []) + [n, 1.0]] * 3, np.float32)
    return dict(n=len(radius), stop=0 if stop else -1, radius=radius, thickness=th, ior=ior,
                semi_aperture=np.full(len(radius), h, np.float32), sensor_width_mm=36.0)


def _slab(n, t=20.0, h=500.0):
    """ONE flat interface: air on the scene side, glass of index n from the interface to the sensor."""
    return dict(n=1, stop=-1, radius=np.zeros(1, np.float32), thickness=np.array([t], np.float32),
                ior=np.array([[n]] * 3, np.float32), semi_aperture=np.array([h], np.float32), sensor_width_mm=36.0)


def _weight(lf, lam, uv=(0.0, 0.0)):
    out = lf.generate_lens_rays(lam, [[0.0, 0.0]], [list(uv)])[0]
    assert out[7] == 1.0
    return float(out[6])


def _coat(lf, n_surf, films, m=MGF2):
    """films: {interface: thickness_nm}"""
    d = np.zeros(n_surf, np.float32)
    for k, t in films.items():
        d[k] = t
    lf.set_lens_coatings(LAMBDAS, d, np.full((3, n_surf), m, np.float32))


@pytest.mark.parametrize("n", [1.5, 1.67, 1.9])
def test_slabs_at_normal_incidence_quarter_and_half_wave(pkg, lf, n):
    for lens, films in ((_slab(n), (0,)), (_plate(n), (0, 1))):
        lf.set_lens(lens)
        bare = [_weight(lf, lam) for lam in range(3)]
        for lam, L in enumerate(LAMBDAS):
            rb = ((n - 1.0) / (n + 1.0)) ** 2
            qw = ((n - MGF2 ** 2) / (n + MGF2 ** 2)) ** 2
            for thick, R in ((L / (4 * MGF2), qw), (L / (2 * MGF2), rb)):
                _coat(lf, lens["n"], {k: thick for k in films})
                got = _weight(lf, lam) / bare[lam]
                want = ((1 - R) / (1 - rb)) ** len(films)
                assert got == pytest.approx(want, rel=2e-6), (n, L, thick)
        lf.set_lens_coatings(None)


@pytest.mark.parametrize("direction", ["glass_to_air", "air_to_glass"])
def test_angle_sweep_against_float64_airy(pkg, lf, direction):
    n, t, h = 1.67, 20.0, 500.0
    if direction == "glass_to_air":     # the primary path leaves the glass through interface 0 of a slab
        lens, k, n_in, n_out, crit = _slab(n, t, h), 0, n, 1.0, math.asin(1.0 / n)
    else:                               # ... enters the plate's glass through its rear interface 1 from the air
        lens, k, n_in, n_out, crit = _plate(n, h, (5.0, t)), 1, 1.0, n, math.pi / 2
    lf.set_lens(lens)
    for lam, L in enumerate(LAMBDAS):
        for d in (L / (4 * MGF2), 0.37 * L, 1.1 * L):
            for frac in np.linspace(0.0, 0.9, 10):
                u = math.tan(frac * crit) * t / h          # pupil point h u at distance t: incidence angle frac * crit
                lf.set_lens_coatings(None)
                wb = _weight(lf, lam, (u, 0.0))
                _coat(lf, lens["n"], {k: d})
                wc = _weight(lf, lam, (u, 0.0))
                c = math.cos(math.atan2(float(np.float32(h) * np.float32(u)), t))
                rc = airy64(n_in, MGF2, n_out, float(np.float32(d)), float(np.float32(L)), c)
                rb = airy64(n_in, n_in, n_out, 0.0, 500.0, c)
                assert wc / wb == pytest.approx((1 - rc) / (1 - rb), rel=2e-5), (lam, d, frac)
    lf.set_lens_coatings(None)


def test_axial_ray_through_the_coated_double_gauss(pkg, lf):
    lens = pkg.load_lens_file("dgauss11_coated.lens")
    lf.set_lens(lens)
    c = lens["coatings"]
    norm = math.pi * float(lens["semi_aperture"][-1]) ** 2 / float(lens["thickness"][-1]) ** 2
    for lam in range(3):
        T, nb = 1.0, 1.0
        for k in range(lens["n"]):
            if k == lens["stop"]:
                continue
            na = float(lens["ior"][lam, k])
            d = float(c["thickness_nm"][k])
            m = float(c["index"][lam, k]) if d > 0 else nb
            T *= 1.0 - airy64(na, m, nb, d, float(c["lambda_nm"][lam]), 1.0)   # the primary path travels -z
            nb = na
        assert _weight(lf, lam) / norm == pytest.approx(T, rel=5e-6)
        assert T > 0.9            # against 0.5 .. 0.9 uncoated (test_gpu_lens_kat.py)


# ---- ghosts through lf_trace_ghosts ---------------------------------------------------------------------------------

def _plate_frame(pkg, lf, pairs, primary):
    # a 1.5 mm sensor: the lobe's footprint on the 0.5 mm pupil (0.2 mm) is a sizeable part of it, the lit disc 60 pixels wide
    lens = _plate(1.67, h=0.5, t=(5.0, 20.0), stop=True)
    lens["sensor_width_mm"] = 1.5
    lf.set_frame(64, 64)
    lf.set_aperture(pkg.APERTURE_STARBURST, np.ones((8, 8), np.float32))
    lf.set_lens(lens)
    lf.set_sun([0.0, 0.0, -1.0], [1000.0, 1000.0, 1000.0], 0.01)
    lf.set_ghost_pairs(pairs, primary)
    lf.set_band(0, 64)
    return lens


@pytest.mark.parametrize("cull,bits", [(0, 6), (2, 6), (0, 0), (2, 0)])
def test_ghost_and_primary_ratios_on_a_coated_plate(pkg, lf, cull, bits):
    """pair (1, 2) of a plate behind an open stop and the primary path, launched apart: coated / bare of every lit
    value is that path's closed-form ratio at normal incidence (the sun is axial and 0.01 rad wide)"""
    lf.test_knob("cull_force", 1)
    try:
        for pairs, primary in (([[1, 2]], False), ([[-1, -1]], False)):
            lens = _plate_frame(pkg, lf, pairs, primary)
            lf.set_pupil_subcells(bits)
            lf.set_march_culling(cull)
            frames = []
            for coat in (False, True):
                if coat:
                    _coat(lf, lens["n"], {1: 99.638, 2: 99.638})
                else:
                    lf.set_lens_coatings(None)
                lf.trace_ghosts(64, 11)
                frames.append(lf.read_buffer(pkg.GHOST_BUFFER).copy())
            if cull == 0:
                assert not lf.cull_info()["culled"]
            bare, coated = frames
            lit_b, lit_c = bare > 0, coated > 0
            assert lit_b.sum() > 100
            assert not np.any(lit_c & ~lit_b)
            big = bare > 1e-4 * bare.max()
            assert np.all(lit_c[big])
            for ch, L in enumerate(LAMBDAS):
                rb = airy64(1.0, 1.0, 1.67, 0.0, L, 1.0)
                rc = airy64(1.0, MGF2, 1.67, 99.638, L, 1.0)
                ratio = ((1 - rc) / (1 - rb)) ** 2 * ((rc / rb) ** 2 if pairs[0][0] >= 0 else 1.0)
                sel = big[..., ch]
                got = coated[..., ch][sel] / bare[..., ch][sel]
                assert np.allclose(got, ratio, rtol=1e-3), (pairs, ch, got.min(), got.max(), ratio)
    finally:
        lf.test_knob("cull_force", 0)
        lf.set_march_culling(1)
        lf.set_pupil_subcells(6)
        lf.set_lens_coatings(None)


# ---- the double Gauss: geometry, invariance, kernels, lifecycle ----------------------------------------------------

def _c3_band(pkg, lf, lens, spp=64, cull=2, y0=512, y1=576):
    W, H = 1920, 1080
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, load_texels("pentbig500_14.png"))
    lf.set_lens(lens)
    efl = pkg.paraxial_efl(lens)
    sw = lens["sensor_width_mm"]
    lf.set_sun([(SUN_NS[0] - 0.5) * sw / efl, (SUN_NS[1] - 0.5) * sw * H / W / efl, -1.0], [1.0, 0.9, 0.5], 0.05)
    lf.set_ghost_pairs(None, True)
    lf.set_band(y0, y1)
    lf.set_march_culling(cull)
    lf.reset_counters()
    lf.trace_ghosts(spp, 0x1e45f1a4e)
    return dict(ghost=lf.read_buffer(pkg.GHOST_BUFFER).copy(), counters=lf.counters(), executed=lf.executed_events(),
                stats=lf.march_stats(), fix=lf.march_fix_bits(), table=lf.cull_table(), audit=lf.cull_audit(),
                culled=lf.cull_info()["culled"])


def test_coatings_never_touch_geometry(pkg, lf):
    a = _c3_band(pkg, lf, pkg.load_lens_file("dgauss11.lens"))
    b = _c3_band(pkg, lf, pkg.load_lens_file("dgauss11_coated.lens"))
    assert lf.lens_coatings()["n_coated"] == 8
    assert a["culled"] and b["culled"]
    for k in ("counters", "executed", "stats", "fix", "audit"):
        assert a[k] == b[k], k
    assert np.array_equal(a["table"], b["table"])
    # the same rays light the same pixels; a lit value of the coated frame can only vanish where all of its (far dimmer)
    # contributions fall below the fixed-point grid of the sums, 2^-36
    lit_a, lit_b = a["ghost"] > 0, b["ghost"] > 0
    assert not np.any(lit_b & ~lit_a)
    assert lit_b.sum() > 0.99 * lit_a.sum()
    assert not np.any(lit_a & ~lit_b) or a["ghost"][lit_a & ~lit_b].max() < 1e5 * 2.0 ** -36
    assert not np.array_equal(a["ghost"], b["ghost"])
    lf.set_band(0, 1080)


@pytest.mark.parametrize("film", ["m_is_air", "zero_thickness"])
def test_neutral_films_reproduce_the_bare_frame(pkg, lf, film):
    lens = pkg.load_lens_file("dgauss11.lens")
    a = _c3_band(pkg, lf, lens, spp=16)
    coated = dict(lens)
    glass_air = [0, 1, 2, 4, 6, 8, 9, 10]
    d = np.zeros(11, np.float32)
    d[glass_air] = 0.0 if film == "zero_thickness" else 123.0
    coated["coatings"] = dict(lambda_nm=np.array(LAMBDAS, np.float32), thickness_nm=d,
                              index=np.ones((3, 11), np.float32))
    b = _c3_band(pkg, lf, coated, spp=16)
    assert lf.lens_coatings()["n_coated"] == (0 if film == "zero_thickness" else 8)
    assert np.array_equal(a["ghost"] > 0, b["ghost"] > 0)
    lit = a["ghost"] > 0
    # 1e-5 relative, and a few steps of the 2^-36 grid every contribution is truncated to (a value of 1e-9 is 70 steps)
    assert np.allclose(b["ghost"][lit], a["ghost"][lit], rtol=1e-5, atol=64 * 2.0 ** -36)
    assert a["counters"] == b["counters"]
    lf.set_band(0, 1080)


def test_kernels_agree_bit_for_bit_on_the_coated_lens(pkg, lf):
    lens = pkg.load_lens_file("dgauss11_coated.lens")
    lf.test_knob("cull_force", 1)
    try:
        full = _c3_band(pkg, lf, lens, spp=16, cull=0)
        culled = _c3_band(pkg, lf, lens, spp=16, cull=2)
        assert culled["culled"] and not full["culled"]
        assert np.array_equal(full["ghost"], culled["ghost"])
        assert full["counters"]["rays_hit_light"] == culled["counters"]["rays_hit_light"]
        lf.test_knob("cull_weights_first", 1)
        try:
            wf = _c3_band(pkg, lf, lens, spp=16, cull=2)
        finally:
            lf.test_knob("cull_weights_first", 0)
        assert np.array_equal(wf["ghost"], culled["ghost"])
        # the independent-pixel item kernel against the path tree, one sampling specification
        lf.set_pupil_subcells(0)
        tree = _c3_band(pkg, lf, lens, spp=16, cull=0)
        items = _c3_band(pkg, lf, lens, spp=16, cull=2)
        assert items["culled"]
        assert np.array_equal(tree["ghost"], items["ghost"])
        assert tree["ghost"].sum() > 0
    finally:
        lf.test_knob("cull_force", 0)
        lf.set_pupil_subcells(6)
        lf.set_march_culling(1)
        lf.set_band(0, 1080)


def test_lifecycle(pkg, lf):
    bare_lens, coated_lens = pkg.load_lens_file("dgauss11.lens"), pkg.load_lens_file("dgauss11_coated.lens")
    never = _c3_band(pkg, lf, bare_lens, spp=16)
    # set, then clear: the frame of a context that never had coatings
    c = coated_lens["coatings"]
    lf.set_lens_coatings(c["lambda_nm"], c["thickness_nm"], c["index"])
    lf.trace_ghosts(16, 0x1e45f1a4e)
    assert not np.array_equal(lf.read_buffer(pkg.GHOST_BUFFER), never["ghost"])
    lf.set_lens_coatings(None)
    assert lf.lens_coatings()["n_coated"] == 0
    lf.reset_counters()
    lf.trace_ghosts(16, 0x1e45f1a4e)
    assert np.array_equal(lf.read_buffer(pkg.GHOST_BUFFER), never["ghost"])
    # lf_set_lens clears them
    coated = _c3_band(pkg, lf, coated_lens, spp=16)
    assert not np.array_equal(coated["ghost"], never["ghost"])
    again = _c3_band(pkg, lf, bare_lens, spp=16)
    assert lf.lens_coatings()["n_coated"] == 0 and np.array_equal(again["ghost"], never["ghost"])
    # the C loader of the coated file = set_lens + set_lens_coatings with the same numbers
    lf.load_lens_file(os.path.join(pkg.DATA, "dgauss11_coated.lens"))
    got = lf.lens_coatings()
    assert got["n_coated"] == 8 and np.array_equal(got["thickness_nm"], c["thickness_nm"])
    assert np.array_equal(got["index"], c["index"]) and np.array_equal(got["lambda_nm"], c["lambda_nm"])
    lf.reset_counters()
    lf.trace_ghosts(16, 0x1e45f1a4e)
    assert np.array_equal(lf.read_buffer(pkg.GHOST_BUFFER), coated["ghost"])
    # focusing keeps them
    lf.focus_lens(2000.0)
    assert lf.lens_coatings()["n_coated"] == 8
    # the lens camera's calibration follows the films: more light through the lens, a smaller exposure
    lf.set_frame(64, 64)
    lf.set_aperture(pkg.APERTURE_STARBURST, np.ones((8, 8), np.float32))
    lf.set_lens(bare_lens)
    lf.set_lens_camera(1, 0.001, 0.0)
    e_bare = lf.lens_camera()["exposure"]
    lf.set_lens_coatings(c["lambda_nm"], c["thickness_nm"], c["index"])
    e_coat = lf.lens_camera()["exposure"]
    assert e_coat < 0.8 * e_bare
    lf.set_lens_coatings(None)
    assert lf.lens_camera()["exposure"] == e_bare
    lf.set_lens_camera(0, 0.001, 0.0)


def test_refusals_through_the_context(pkg):
    ctx = pkg.LensFlare(0)
    try:
        ctx.set_frame(32, 32)
        with pytest.raises(pkg.LensFlareError, match="LF_ERR_STATE"):
            ctx.set_lens_coatings(LAMBDAS, np.zeros(11, np.float32), np.ones((3, 11), np.float32))
        ctx.set_lens(pkg.load_lens_file("dgauss11.lens"))
        good_d = np.zeros(11, np.float32)
        good_d[0] = 100.0
        ones = np.full((3, 11), MGF2, np.float32)
        ctx.set_lens_coatings(LAMBDAS, good_d, ones)
        bad = []
        d = good_d.copy(); d[5] = 100.0; bad.append((LAMBDAS, d, ones))                      # the stop
        d = good_d.copy(); d[0] = -1.0; bad.append((LAMBDAS, d, ones))
        d = good_d.copy(); d[0] = 20000.0; bad.append((LAMBDAS, d, ones))
        d = good_d.copy(); d[0] = np.nan; bad.append((LAMBDAS, d, ones))
        bad.append(((656.3, 0.0, 486.1), good_d, ones))
        bad.append(((656.3, np.inf, 486.1), good_d, ones))
        bad.append((LAMBDAS, np.zeros(10, np.float32), np.ones((3, 10), np.float32)))      # sizes of another lens
        bad.append((LAMBDAS[:2], good_d, ones[:2]))
        low = ones.copy(); low[1, 0] = 0.99; bad.append((LAMBDAS, good_d, low))            # below air
        nan = ones.copy(); nan[2, 0] = np.nan; bad.append((LAMBDAS, good_d, nan))
        for args in bad:
            with pytest.raises(pkg.LensFlareError, match="LF_ERR_INVALID"):
                ctx.set_lens_coatings(*args)
        got = ctx.lens_coatings()                  # a refused call changes nothing
        assert got["n_coated"] == 1 and got["thickness_nm"][0] == np.float32(100.0)
        # a film on a cemented interface must not go below the smaller of its two glasses
        low = ones.copy(); low[:, 3] = 1.6
        d = np.zeros(11, np.float32); d[3] = 100.0
        with pytest.raises(pkg.LensFlareError, match="LF_ERR_INVALID"):
            ctx.set_lens_coatings(LAMBDAS, d, low)
        ok = ones.copy(); ok[:, 3] = 1.7
        ctx.set_lens_coatings(LAMBDAS, d, ok)
    finally:
        ctx.close()
