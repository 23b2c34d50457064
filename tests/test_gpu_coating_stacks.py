"""Multi-layer anti-reflection stacks on the device (lf_set_lens_coating_stacks, the kVarStack kernels): per-ray
transmission through lf_generate_lens_rays against the float64 characteristic-matrix formula of
tests/test_coating_stacks_cpu.py (asymmetric stacks, both directions of travel: a wrong layer order fails), ghost ratios
through lf_trace_ghosts, the curved lens against the float64 tracer through a stack that must equal a single film,
geometry untouched, kernel agreement, routing of one-layer stacks to the film kernels, combinations with the bilinear mask
and several lights, and the stacks' lifecycle and refusals."""
import math
import os

import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo
from test_coating_stacks_cpu import matrix64
from test_geo_rays_vs_f64 import DIR_TOL, POS_TOL_MM, W_TOL
from test_gpu_coatings import LAMBDAS, _c3_band, _plate, _plate_frame, _slab, _weight
from test_gpu_lens_camera import look_at, setup_scene_frame
from test_gpu_march_f64 import _check_against_f64

pytestmark = pytest.mark.gpu
GLASS = 1.67
AIR_GLASS = [0, 1, 2, 4, 6, 8, 9, 10]
# asymmetric stacks, listed scene side first: (index, thickness nm)
STACK2 = [(1.38, 110.0), (2.05, 61.0)]
STACK3 = [(1.38, 99.6), (2.05, 134.1), (1.63, 84.4)]
STACK6 = [(1.38, 90.0), (2.3, 25.0), (1.46, 140.0), (2.05, 70.0), (1.63, 211.0), (1.9, 33.0)]


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


def _arrays(n_surf, stacks, n_lambda=3, rows=6):
    """stacks: {interface: [(index, thickness_nm), ...]} scene side first -> n_layers, thickness (rows x n), index"""
    cnt = np.zeros(n_surf, np.int32)
    d = np.zeros((rows, n_surf), np.float32)
    m = np.ones((rows, n_lambda, n_surf), np.float32)
    for k, layers in stacks.items():
        cnt[k] = len(layers)
        for j, (mj, dj) in enumerate(layers):
            d[j, k] = dj
            m[j, :, k] = mj
    return cnt, d, m


def _stack(lf, n_surf, stacks, lambdas=LAMBDAS):
    lf.set_lens_coating_stacks(lambdas, *_arrays(n_surf, stacks, len(lambdas)))


def _R(n_in, ray_order, n_out, lam, cos_in=1.0):
    """the matrix formula with every number as the device receives it"""
    f = lambda v: float(np.float32(v))
    return matrix64(f(n_in), [f(m) for m, _ in ray_order], [f(d) for _, d in ray_order], f(n_out), f(lam), cos_in)


# ---- 1. per ray, flat glass -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", ["glass_to_air", "air_to_glass"])
def test_angle_sweep_against_the_float64_matrix_formula(pkg, lf, direction):
    """coated / bare transmission of one flat interface of n = 1.67 under asymmetric stacks of 2, 3 and 6 layers, the three
    wavelengths, ten angles to 0.9 of the critical angle (of grazing incidence from the air).  The primary path travels
    towards the scene: it meets the layers in the REVERSE of their listed order.  Bar: the single film's rel = 2e-5."""
    n, t, h = GLASS, 20.0, 500.0
    if direction == "glass_to_air":     # the primary path leaves the glass through interface 0 of a slab
        lens, k, n_in, n_out, crit = _slab(n, t, h), 0, n, 1.0, math.asin(1.0 / n)
    else:                               # ... enters the plate's glass through its rear interface 1 from the air
        lens, k, n_in, n_out, crit = _plate(n, h, (5.0, t)), 1, 1.0, n, math.pi / 2
    lf.set_lens(lens)
    us = [math.tan(frac * crit) * t / h for frac in np.linspace(0.0, 0.9, 10)]
    bare = {(lam, i): _weight(lf, lam, (u, 0.0)) for lam in range(3) for i, u in enumerate(us)}
    worst = 0.0
    for layers in (STACK2, STACK3, STACK6):
        wrong = 0.0
        _stack(lf, lens["n"], {k: layers})
        assert lf.get_lens_coating_stacks()["n_stacked"] == 1
        for lam, L in enumerate(LAMBDAS):
            for i, u in enumerate(us):
                wc = _weight(lf, lam, (u, 0.0))
                c = math.cos(math.atan2(float(np.float32(h) * np.float32(u)), t))
                rc = _R(n_in, layers[::-1], n_out, L, c)
                rb = _R(n_in, [], n_out, L, c)
                want = (1 - rc) / (1 - rb)
                dev = abs(wc / bare[lam, i] / want - 1.0)
                worst = max(worst, dev)
                assert dev <= 2e-5, (len(layers), lam, i, wc / bare[lam, i], want)
                wrong = max(wrong, abs((1 - _R(n_in, layers, n_out, L, c)) / (1 - rb) / want - 1.0))
        # the listed order is NOT the order of travel: the other order is another number, far outside the bar
        assert wrong > 1e-3, (len(layers), wrong)
    print(f"{direction}: worst relative deviation of coated / bare from the matrix formula {worst:.2e}")
    lf.set_lens_coating_stacks(None)


# ---- 2., 3. ghosts through lf_trace_ghosts ---------------------------------------------------------------------------

def _pair_and_primary_ratios(stack1, stack2):
    """closed-form coated / bare of pair (1, 2) and of the primary path of the plate behind an open stop, per channel:
    the ray crosses 2 and reflects at 1 travelling -z (layers reversed), reflects at 2 travelling +z (as listed)"""
    out = []
    for L in LAMBDAS:
        rb = _R(1.0, [], GLASS, L)
        t2 = 1 - _R(1.0, stack2[::-1], GLASS, L)          # air -> glass through 2, -z
        t1 = 1 - _R(GLASS, stack1[::-1], 1.0, L)          # glass -> air through 1, -z
        r1 = _R(GLASS, stack1[::-1], 1.0, L)              # mirror at 1, arriving -z from the glass
        r2 = _R(GLASS, stack2, 1.0, L)                    # mirror at 2, arriving +z from the glass
        tt = t1 * t2 / (1 - rb) ** 2
        out.append((tt * r1 * r2 / rb ** 2, tt))
    return out


def _plate_ratio(pkg, lf, pairs, stacks, cull=0, bits=6):
    lens = _plate_frame(pkg, lf, pairs, False)
    lf.set_pupil_subcells(bits)
    lf.set_march_culling(cull)
    frames = []
    for coat in (False, True):
        if coat:
            _stack(lf, lens["n"], stacks)
        else:
            lf.set_lens_coating_stacks(None)
        lf.trace_ghosts(64, 11)
        frames.append(lf.read_buffer(pkg.GHOST_BUFFER).copy())
    if cull == 0:
        assert not lf.cull_info()["culled"]
    bare, coated = frames
    assert (bare > 0).sum() > 100 and not np.any((coated > 0) & ~(bare > 0))
    return bare, coated, bare > 1e-4 * bare.max()


def test_the_v_coat_has_no_ghost_at_its_design_wavelength(pkg, lf):
    """two quarter-wave layers at the d line with m2 = m1 sqrt(n): the ghost of pair (1, 2) vanishes in that channel
    (ratio < 1e-4), the other channels follow the closed form"""
    m1 = 1.38
    m2 = m1 * math.sqrt(GLASS)
    L = LAMBDAS[1]
    front = [(m1, L / (4 * m1)), (m2, L / (4 * m2))]            # interface 1: the air is on the scene side
    try:
        bare, coated, big = _plate_ratio(pkg, lf, [[1, 2]], {1: front, 2: front[::-1]})
        want = _pair_and_primary_ratios(front, front[::-1])
        for ch in range(3):
            got = coated[..., ch][big[..., ch]] / bare[..., ch][big[..., ch]]
            if ch == 1:
                assert got.max() < 1e-4, got.max()
            else:
                print(f"V-coat, channel {ch}: coated / bare in [{got.min():.4e}, {got.max():.4e}], closed form {want[ch][0]:.4e}")
                assert np.allclose(got, want[ch][0], rtol=1e-3), (ch, got.min(), got.max(), want[ch][0])
    finally:
        lf.set_march_culling(1)
        lf.set_lens_coating_stacks(None)


@pytest.mark.parametrize("cull,bits", [(0, 6), (2, 6), (0, 0), (2, 0)])
def test_ghost_and_primary_ratios_on_a_stacked_plate(pkg, lf, cull, bits):
    """pair (1, 2) and the primary path of a plate whose two faces carry the SAME listed three-layer stack: the two
    mirror events see it from opposite sides in opposite orders"""
    lf.test_knob("cull_force", 1)
    try:
        want = _pair_and_primary_ratios(STACK3, STACK3)
        for pairs, col in (([[1, 2]], 0), ([[-1, -1]], 1)):
            bare, coated, big = _plate_ratio(pkg, lf, pairs, {1: STACK3, 2: STACK3}, cull, bits)
            assert np.all((coated > 0)[big])
            for ch in range(3):
                got = coated[..., ch][big[..., ch]] / bare[..., ch][big[..., ch]]
                assert np.allclose(got, want[ch][col], rtol=1e-3), (pairs, ch, got.min(), got.max(), want[ch][col])
    finally:
        lf.test_knob("cull_force", 0)
        lf.set_march_culling(1)
        lf.set_pupil_subcells(6)
        lf.set_lens_coating_stacks(None)


def test_a_film_and_a_stack_on_one_lens(pkg, lf):
    """face 1 of the plate carries ONE layer -- a single film: an LfCoatK record, bit 0 of its offset clear -- and face 2 a
    real stack, so the film is evaluated inside the kVarStack kernels (StackRec::get, StackPrimary with coated = 1): pair
    (1, 2) and the primary path against the closed form, the path tree and the culled kernels"""
    film = [(1.38, 99.638)]
    lf.test_knob("cull_force", 1)
    try:
        want = _pair_and_primary_ratios(film, STACK3)
        for cull in (0, 2):
            for pairs, col in (([[1, 2]], 0), ([[-1, -1]], 1)):
                bare, coated, big = _plate_ratio(pkg, lf, pairs, {1: film, 2: STACK3}, cull)
                info = lf.get_lens_coating_stacks()
                assert info["n_stacked"] == 1 and list(info["n_layers"]) == [0, 1, 3]
                for ch in range(3):
                    got = coated[..., ch][big[..., ch]] / bare[..., ch][big[..., ch]]
                    assert np.allclose(got, want[ch][col], rtol=1e-3), (cull, pairs, ch, got.min(), got.max(), want[ch][col])
        # ... and per ray: the primary table's film row beside its stack row
        lens = _plate(GLASS, 500.0, (5.0, 20.0))
        lf.set_lens(lens)
        bare_w = [_weight(lf, lam) for lam in range(3)]
        _stack(lf, 2, {0: film, 1: STACK3})
        for lam, L in enumerate(LAMBDAS):
            rb = _R(1.0, [], GLASS, L)
            T = (1 - _R(1.0, STACK3[::-1], GLASS, L)) * (1 - _R(GLASS, film, 1.0, L)) / (1 - rb) ** 2
            assert _weight(lf, lam) / bare_w[lam] == pytest.approx(T, rel=2e-5)
    finally:
        lf.test_knob("cull_force", 0)
        lf.set_march_culling(1)
        lf.set_lens_coating_stacks(None)


# ---- 4. the axial ray --------------------------------------------------------------------------------------------------

def test_axial_ray_through_the_multicoated_double_gauss(pkg, lf):
    lens = pkg.load_lens_file("dgauss11_multicoated.lens")
    lf.set_frame(64, 64)
    lf.set_aperture(pkg.APERTURE_STARBURST, np.ones((4, 4), np.float32))
    lf.set_lens(lens)
    c = lens["coating_stacks"]
    assert lf.get_lens_coating_stacks()["n_stacked"] == 8
    norm = math.pi * float(lens["semi_aperture"][-1]) ** 2 / float(lens["thickness"][-1]) ** 2
    for lam in range(3):
        T, nb = 1.0, 1.0
        for k in range(lens["n"]):
            if k == lens["stop"]:
                continue
            na = float(lens["ior"][lam, k])
            layers = [(float(c["index"][j, lam, k]), float(c["thickness_nm"][j, k])) for j in range(c["n_layers"][k])]
            T *= 1.0 - _R(na, layers[::-1], nb, float(c["lambda_nm"][lam]))     # the primary path travels -z
            nb = na
        assert _weight(lf, lam) / norm == pytest.approx(T, rel=5e-6)
        assert T > 0.95           # against > 0.9 under single films
    lf.set_lens_coating_stacks(None)


# ---- 5. the curved lens against the float64 tracer -------------------------------------------------------------------

def _split_film_lens(pkg):
    """dgauss11_coated.lens with every 99.638 nm film split into two layers of its index, 40 + 59.638 nm: the stack
    kernels run, and the frames must be the single films' (which the float64 tracer follows)"""
    lens = pkg.load_lens_file("dgauss11_coated.lens")
    films = lens.pop("coatings")
    cnt, d, m = _arrays(lens["n"], {k: [(1.38, 40.0), (1.38, 59.638)] for k in AIR_GLASS})
    lens["coating_stacks"] = dict(lambda_nm=films["lambda_nm"], n_layers=cnt, thickness_nm=d, index=m)
    return lens, films


def test_split_films_on_the_double_gauss_against_the_float64_tracer(pkg, lf):
    lens, films = _split_film_lens(pkg)
    mask = load_texels("pentbig500_14.png")
    Wg, Hg, spp, key = 64, 48, 256, 0xBEEF
    sun, rad, alpha = [0.03, 0.02, -1.0], [1.0, 0.9, 0.5], 0.05
    lf.set_frame(Wg, Hg)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    assert lf.get_lens_coating_stacks()["n_stacked"] == 8
    lf.set_sun(sun, rad, alpha)
    lf.set_ghost_pairs(None, True)
    lf.set_band(0, Hg)
    lf.set_march_culling(0)
    lf.reset_counters()
    lf.trace_ghosts(spp, key)
    img, cnt = lf.read_buffer(pkg.GHOST_BUFFER), lf.counters()
    g = (np.arange(24) + 0.5) / 12.0 - 1.0
    uv = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2).astype(np.float32)
    try:
        lfo.g64_set_films(films)
        ref, frag, c64 = lfo.g64_trace(lens, Wg, Hg, 0, Hg, spp, key, None, True, mask, sun, rad, alpha, n_threads=16)
        rel = _check_against_f64(img, cnt, ref, frag, c64, min_lit=150)
        print(f"ghost frame through the split films: {rel.size} converged values, max rel {rel.max():.2e}, median {np.median(rel):.2e}")
        # k_lens_rays: the primary table's stack records, every interface crossed obliquely
        n_alive, worst = 0, 0.0
        for xy0 in ((0.0, 0.0), (3.0, -2.0)):
            xy = np.tile(np.float32(xy0), (len(uv), 1))
            for lam in range(3):
                got = lf.generate_lens_rays(lam, xy, uv).astype(np.float64)
                r64 = lfo.g64_lens_rays(lens, lam, xy, uv, mask)
                firm = r64[:, 8] == 0
                assert np.array_equal(got[firm, 7] == 1.0, r64[firm, 9] == 0), (xy0, lam)
                a = firm & (r64[:, 9] == 0)
                n_alive += int(a.sum())
                dd = got[a, 3:6] / np.linalg.norm(got[a, 3:6], axis=1)[:, None]
                assert (np.abs(got[a, 0:3] - r64[a, 0:3]).max(axis=1) <= POS_TOL_MM).all()
                assert (np.abs(dd - r64[a, 3:6]).max(axis=1) <= DIR_TOL).all()
                e_w = np.abs(got[a, 6] - r64[a, 6]) / r64[a, 6]
                worst = max(worst, e_w.max())
                assert (e_w <= W_TOL).all(), (xy0, lam, e_w.max())
        print(f"k_lens_rays through the split films: {n_alive} rays, worst relative weight deviation {worst:.2e}")
        assert n_alive >= 100
    finally:
        lfo.g64_set_films(None)
        lf.set_march_culling(1)


# ---- 6. - 9. the double Gauss: geometry, kernels, routing, combinations ----------------------------------------------

@pytest.fixture(scope="module")
def bands(pkg, lf):
    """the c3 band (64 rows, 64 spp, culled) under the bare, the single-coated and the multicoated lens, once"""
    out = {name: _c3_band(pkg, lf, pkg.load_lens_file(name + ".lens")) for name in ("dgauss11", "dgauss11_coated", "dgauss11_multicoated")}
    lf.set_band(0, 1080)
    return out


def test_stacks_never_touch_geometry(pkg, lf, bands):
    a, b = bands["dgauss11"], bands["dgauss11_multicoated"]
    assert a["culled"] and b["culled"]
    for k in ("counters", "executed", "stats", "fix", "audit"):
        assert a[k] == b[k], k
    assert np.array_equal(a["table"], b["table"])
    lit_a, lit_b = a["ghost"] > 0, b["ghost"] > 0
    assert not np.any(lit_b & ~lit_a)
    assert lit_b.sum() > 0.9 * lit_a.sum()


def test_the_multicoated_frame_is_its_own_and_dimmer(pkg, lf, bands):
    bare, single, multi = (bands[k]["ghost"] for k in ("dgauss11", "dgauss11_coated", "dgauss11_multicoated"))
    assert not np.array_equal(multi, single) and not np.array_equal(multi, bare)
    # the ghosts: everything but the primary path's image of the sun
    sums = {}
    for name in ("dgauss11", "dgauss11_coated", "dgauss11_multicoated"):
        _c3_band(pkg, lf, pkg.load_lens_file(name + ".lens"), spp=16)
        lf.set_ghost_pairs(None, False)
        lf.trace_ghosts(16, 0x1e45f1a4e)
        sums[name] = lf.read_buffer(pkg.GHOST_BUFFER).sum(axis=(0, 1))
    lf.set_ghost_pairs(None, True)
    lf.set_band(0, 1080)
    assert np.all(sums["dgauss11"] > 0)
    assert np.all(sums["dgauss11_multicoated"] < sums["dgauss11"])
    # (not below the single films' in every channel: a quarter wave of MgF2 on these glasses reflects 0.4 .. 0.6 % near its
    # design wavelength, the broadband stack 0.3 .. 0.8 % at the d line -- it wins at the C and F lines, by factors)
    assert sums["dgauss11_multicoated"][0] < sums["dgauss11_coated"][0] and sums["dgauss11_multicoated"][2] < sums["dgauss11_coated"][2]


def test_one_layer_stacks_are_the_single_films_bit_for_bit(pkg, lf, bands):
    lens = pkg.load_lens_file("dgauss11_coated.lens")
    films = lens.pop("coatings")
    one = dict(lens)
    cnt, d, m = _arrays(11, {k: [(1.38, float(films["thickness_nm"][k]))] for k in AIR_GLASS})
    one["coating_stacks"] = dict(lambda_nm=films["lambda_nm"], n_layers=cnt, thickness_nm=d, index=m)
    got = _c3_band(pkg, lf, one)
    info = lf.get_lens_coating_stacks()
    assert info["n_stacked"] == 0 and list(info["n_layers"][AIR_GLASS]) == [1] * 8
    assert lf.lens_coatings()["n_coated"] == 8          # ... and the single films' getter reads them
    assert np.array_equal(got["ghost"], bands["dgauss11_coated"]["ghost"])
    # a layer of thickness 0 somewhere in a real stack: the stack's frame
    multi = pkg.load_lens_file("dgauss11_multicoated.lens")
    c = multi["coating_stacks"]
    cnt, d, m = c["n_layers"].copy(), c["thickness_nm"].copy(), c["index"].copy()
    for k in AIR_GLASS:        # insert a zero layer in the middle
        d[2:4, k] = d[1:3, k]; m[2:4, :, k] = m[1:3, :, k]
        d[1, k] = 0.0; m[1, :, k] = 0.5                  # (its index is never read)
        cnt[k] = 4
    multi["coating_stacks"] = dict(lambda_nm=c["lambda_nm"], n_layers=cnt, thickness_nm=d, index=m)
    got = _c3_band(pkg, lf, multi)
    assert list(lf.get_lens_coating_stacks()["n_layers"][AIR_GLASS]) == [3] * 8
    assert np.array_equal(got["ghost"], bands["dgauss11_multicoated"]["ghost"])
    lf.set_band(0, 1080)


def test_kernels_agree_bit_for_bit_on_the_stacked_lens(pkg, lf):
    lens = pkg.load_lens_file("dgauss11_multicoated.lens")
    lf.test_knob("cull_force", 1)
    try:
        full = _c3_band(pkg, lf, lens, spp=16, cull=0)
        culled = _c3_band(pkg, lf, lens, spp=16, cull=2)
        assert culled["culled"] and not full["culled"]
        assert np.array_equal(full["ghost"], culled["ghost"]) and full["ghost"].sum() > 0
        assert full["counters"]["rays_hit_light"] == culled["counters"]["rays_hit_light"]
        lf.test_knob("cull_weights_first", 1)
        try:
            wf = _c3_band(pkg, lf, lens, spp=16, cull=2)
        finally:
            lf.test_knob("cull_weights_first", 0)
        assert np.array_equal(wf["ghost"], culled["ghost"])
        # the independent-pixel item kernel against the path tree, the other sampling specification
        lf.set_pupil_subcells(0)
        tree = _c3_band(pkg, lf, lens, spp=16, cull=0)
        items = _c3_band(pkg, lf, lens, spp=16, cull=2)
        assert items["culled"]
        assert np.array_equal(tree["ghost"], items["ghost"]) and tree["ghost"].sum() > 0
    finally:
        lf.test_knob("cull_force", 0)
        lf.set_pupil_subcells(6)
        lf.set_march_culling(1)
        lf.set_band(0, 1080)


def test_compacted_and_per_lane_lens_camera_agree_on_the_stacked_lens(pkg, lf):
    """k_scene_lens<.., STACK> against k_scene_term<.., true, .., STACK>, one ray per wavelength: frames and counters bit
    for bit, and not the single-coated lens' frame"""
    Wd, Hd, ns = 96, 64, 16
    pos = [0.2, 0.1, 0.8]
    mask = load_texels("pentbig500_14.png")
    frames = {}
    try:
        for name in ("dgauss11_multicoated", "dgauss11_coated"):
            setup_scene_frame(pkg, lf, pkg.load_lens_file(name + ".lens"), mask, Wd, Hd, ns, look_at(pos, [0.0, -0.2, -5.5]), pos)
            lf.set_lens_camera(2, 0.003, 0.0)
            for compact in ((1, 0) if name == "dgauss11_multicoated" else (1,)):
                lf.test_knob("scene_compact", compact)
                lf.set_scene_term(np.zeros((Hd, Wd, 3)))
                lf.reset_scene_counters()
                lf.render_scene_term()
                frames[name, compact] = (lf.read_buffer(pkg.SCENE_BUFFER), lf.scene_counters())
    finally:
        lf.test_knob("scene_compact", -1)
        lf.set_lens_camera(0, 0.003, 0.0)
    a, b, single = frames["dgauss11_multicoated", 1], frames["dgauss11_multicoated", 0], frames["dgauss11_coated", 1]
    assert (a[0].max(axis=-1) > 1e-3).mean() > 0.1
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert not np.array_equal(a[0], single[0]) and a[1] == single[1]        # a stack never changes a ray's fate


def test_bilinear_mask_plus_stack(pkg, lf):
    lens = pkg.load_lens_file("dgauss11_multicoated.lens")
    lf.test_knob("cull_force", 1)
    try:
        lf.set_mask_filter(pkg.MASK_BILINEAR)
        full = _c3_band(pkg, lf, lens, spp=16, cull=0)
        culled = _c3_band(pkg, lf, lens, spp=16, cull=2)
        assert culled["culled"] and not full["culled"]
        assert np.array_equal(full["ghost"], culled["ghost"]) and full["ghost"].sum() > 0
        lf.set_mask_filter(pkg.MASK_NEAREST)
        assert not np.array_equal(_c3_band(pkg, lf, lens, spp=16, cull=2)["ghost"], culled["ghost"])
    finally:
        lf.set_mask_filter(pkg.MASK_NEAREST)
        lf.test_knob("cull_force", 0)
        lf.set_march_culling(1)
        lf.set_band(0, 1080)


def test_two_lights_plus_stack(pkg, lf):
    lens = pkg.load_lens_file("dgauss11_multicoated.lens")
    one = _c3_band(pkg, lf, lens, spp=16)
    efl, sw = pkg.paraxial_efl(lens), lens["sensor_width_mm"]
    dirs = [[(0.521445 - 0.5) * sw / efl, (0.517156 - 0.5) * sw * 1080 / 1920 / efl, -1.0],
            [(0.30 - 0.5) * sw / efl, (0.45 - 0.5) * sw * 1080 / 1920 / efl, -1.0]]
    rad = [1.0, 0.9, 0.5]
    try:
        lf.set_lights(dirs, [rad, rad], [0.05, 0.05])
        lf.reset_counters()
        lf.trace_ghosts(16, 0x1e45f1a4e)
        both = lf.read_buffer(pkg.GHOST_BUFFER).copy()
        for k, d in enumerate(dirs):
            lf.set_sun(d, rad, 0.05)
            lf.set_ghost_accumulate(k > 0)
            lf.trace_ghosts(16, 0x1e45f1a4e)
        total = lf.read_buffer(pkg.GHOST_BUFFER).copy()
    finally:
        lf.set_ghost_accumulate(False)
        lf.set_sun(dirs[0], rad, 0.05)
        lf.set_band(0, 1080)
    assert np.array_equal(both, total)
    assert both.sum() > one["ghost"].sum()


def test_eight_wavelengths_plus_stack(pkg, lf):
    lens = pkg.load_lens_file("dgauss11_8lambda.lens")
    lam = np.asarray(lens["lambda_nm"], np.float32)
    cnt, d, m = _arrays(11, {k: (STACK3 if k in (0, 2, 6, 9) else STACK3[::-1]) for k in AIR_GLASS}, n_lambda=8)
    m[1] *= np.linspace(0.99, 1.02, 8, dtype=np.float32)[:, None]      # a dispersive middle layer
    lens["coating_stacks"] = dict(lambda_nm=lam, n_layers=cnt, thickness_nm=d, index=m)
    lf.test_knob("cull_force", 1)
    try:
        full = _c3_band(pkg, lf, lens, spp=16, cull=0)
        assert lf.get_lens_coating_stacks()["n_stacked"] == 8
        culled = _c3_band(pkg, lf, lens, spp=16, cull=2)
        assert culled["culled"] and not full["culled"]
        assert np.array_equal(full["ghost"], culled["ghost"]) and full["ghost"].sum() > 0
    finally:
        lf.test_knob("cull_force", 0)
        lf.set_march_culling(1)
        lf.set_band(0, 1080)


# ---- 10. lifecycle and refusals --------------------------------------------------------------------------------------

def test_lifecycle(pkg, lf, bands, tmp_path):
    bare_lens, multi_lens = pkg.load_lens_file("dgauss11.lens"), pkg.load_lens_file("dgauss11_multicoated.lens")
    c = multi_lens["coating_stacks"]
    args = (c["lambda_nm"], c["n_layers"], c["thickness_nm"], c["index"])
    never = _c3_band(pkg, lf, bare_lens)
    assert np.array_equal(never["ghost"], bands["dgauss11"]["ghost"])

    def frame():
        lf.reset_counters()
        lf.trace_ghosts(64, 0x1e45f1a4e)
        return lf.read_buffer(pkg.GHOST_BUFFER)
    # set / get round trip; clear: the frame of a context that never had stacks
    lf.set_lens_coating_stacks(*args)
    got = lf.get_lens_coating_stacks()
    assert got["n_stacked"] == 8 and np.array_equal(got["n_layers"], c["n_layers"])
    assert np.array_equal(got["thickness_nm"], c["thickness_nm"]) and np.array_equal(got["lambda_nm"], c["lambda_nm"])
    for k in AIR_GLASS:
        assert np.array_equal(got["index"][:3, :, k], c["index"][:3, :, k])
    assert np.array_equal(frame(), bands["dgauss11_multicoated"]["ghost"])
    with pytest.raises(pkg.LensFlareError, match="LF_ERR_STATE"):
        lf.lens_coatings()
    lf.set_lens_coating_stacks(None)
    assert lf.get_lens_coating_stacks()["n_stacked"] == 0 and lf.lens_coatings()["n_coated"] == 0
    assert np.array_equal(frame(), never["ghost"])
    # the two setters replace each other's state
    films = pkg.load_lens_file("dgauss11_coated.lens")["coatings"]
    lf.set_lens_coating_stacks(*args)
    lf.set_lens_coatings(films["lambda_nm"], films["thickness_nm"], films["index"])
    got = lf.get_lens_coating_stacks()
    assert got["n_stacked"] == 0 and list(got["n_layers"][AIR_GLASS]) == [1] * 8 and lf.lens_coatings()["n_coated"] == 8
    assert np.array_equal(frame(), bands["dgauss11_coated"]["ghost"])
    lf.set_lens_coating_stacks(*args)
    assert lf.get_lens_coating_stacks()["n_stacked"] == 8
    assert np.array_equal(frame(), bands["dgauss11_multicoated"]["ghost"])
    # focusing keeps them, lf_set_lens clears them
    lf.focus_lens(2000.0)
    assert lf.get_lens_coating_stacks()["n_stacked"] == 8
    lf.set_lens(bare_lens)
    assert lf.get_lens_coating_stacks()["n_stacked"] == 0 and lf.get_lens_coating_stacks()["n_layers"].sum() == 0
    assert np.array_equal(frame(), never["ghost"])
    # the C loader of the multicoated file = set_lens + set_lens_coating_stacks with the same numbers
    lf.load_lens_file(os.path.join(pkg.DATA, "dgauss11_multicoated.lens"))
    got = lf.get_lens_coating_stacks()
    assert got["n_stacked"] == 8 and np.array_equal(got["thickness_nm"], c["thickness_nm"])
    assert np.array_equal(frame(), bands["dgauss11_multicoated"]["ghost"])
    # ... and refuses what the Python parser refuses: `layer` lines beside a `coating` line, whatever that line's thickness
    src = open(os.path.join(pkg.DATA, "dgauss11.lens")).read()
    for coating in ("coating 2 99.638 1.38", "coating 2 0 1.38"):
        bad = tmp_path / "bad.lens"
        bad.write_text("lambda_nm 656.3 587.6 486.1\n" + src + "layer 2 50 1.46\n" + coating + "\n")
        with pytest.raises(pkg.LensFlareError, match="LF_ERR_INVALID"):
            lf.load_lens_file(str(bad))
    lf.set_lens(bare_lens)
    lf.set_lens_coating_stacks(None)
    lf.set_band(0, 1080)


def test_refusals_through_the_context(pkg):
    ctx = pkg.LensFlare(0)
    try:
        ctx.set_frame(32, 32)
        cnt, d, m = _arrays(11, {0: STACK3})
        with pytest.raises(pkg.LensFlareError, match="LF_ERR_STATE"):
            ctx.set_lens_coating_stacks(LAMBDAS, cnt, d, m)
        ctx.set_lens(pkg.load_lens_file("dgauss11.lens"))
        ctx.set_lens_coating_stacks(LAMBDAS, cnt, d, m)
        bad = []
        bad.append((LAMBDAS,) + _arrays(10, {0: STACK3}))                                    # n_surfaces of another lens
        bad.append((LAMBDAS[:2],) + _arrays(11, {0: STACK3}, n_lambda=2))                    # n_lambda of another lens
        bad.append((LAMBDAS,) + _arrays(11, {0: [(1.38, 50.0)] * 7}, rows=7))                # more than 6 layers
        bad.append((LAMBDAS,) + _arrays(11, {5: STACK2}))                                    # a layer on the stop
        c2, d2, m2 = _arrays(11, {0: STACK3}); m2[1, 2, 0] = 0.99; bad.append((LAMBDAS, c2, d2, m2))    # below air at one wavelength only
        c2, d2, m2 = _arrays(11, {3: [(1.7, 80.0), (1.75, 60.0), (1.8, 50.0)]}); m2[2, 1, 3] = 1.6; bad.append((LAMBDAS, c2, d2, m2))     # cemented: below both glasses
        for v in (-1.0, 10001.0, np.nan, np.inf):
            c2, d2, m2 = _arrays(11, {0: STACK3}); d2[1, 0] = v; bad.append((LAMBDAS, c2, d2, m2))
        c2, d2, m2 = _arrays(11, {0: STACK3}); m2[0, 0, 0] = np.nan; bad.append((LAMBDAS, c2, d2, m2))
        bad.append(((656.3, 0.0, 486.1),) + _arrays(11, {0: STACK3}))
        for args in bad:
            with pytest.raises(pkg.LensFlareError, match="LF_ERR_INVALID"):
                ctx.set_lens_coating_stacks(*args)
        got = ctx.get_lens_coating_stacks()          # a refused call changes nothing
        assert got["n_stacked"] == 1 and got["n_layers"][0] == 3
        ok = _arrays(11, {3: [(1.7, 80.0), (1.75, 60.0)]})
        ctx.set_lens_coating_stacks(LAMBDAS, *ok)
    finally:
        ctx.close()
