"""The ghosts of point lights, area lights and several lights on the GPU against the INDEPENDENT float64 tracer
(oracle/lf_geo_f64.c under a light list: lfo.g64_trace(lights=...), anchored by tests/test_geo_f64_lights_cpu.py), at the bar
tests/test_gpu_march_f64.py holds the directional sun to: every lit value within 1e-4 relative, the fragile rays' weight the only
allowance.  What the identities of tests/test_gpu_area_ghosts.py / test_gpu_near_lights.py / test_gpu_multi_light.py cannot see --
every kernel family shares light_admits_at / lights_epilogue (lf_march_common.h) -- is seen here: the lit value of a ray that is
tested at its OWN exit point (px, py, front vertex + hz) after two mirrors and the weighted re-march, against a tracer that
shares no expression with the device.  The tracer is fed from ctx.lights_geom(): the values the device stores.

A rectangle's outline is a hard edge: the (ray, light) pairs whose hit point lies in its edge band (lf_geo_f64.c area_lit) are
counted in light_edge_pairs, their weight is in `frag`, and they must stay below 1 % of that light's lit pairs.  Each test prints
the lit values, those needing the allowance, the largest raw deviation, the median, and the edge pairs with their share
(record: profiles/lights_f64_parity.txt).  Occluded frames are held to the same bar in tests/test_gpu_occlusion_f64.py (the tracer's
occluder list); coating stacks stay out: the tracer does not know them."""
import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo
from test_geo_f64_lights_cpu import MASK, AREA, frame_of
from test_gpu_area_ghosts import _setup, _install, _frame
from test_gpu_march_f64 import _check_against_f64, TOL, FLOOR

pytestmark = pytest.mark.gpu
EDGE_CAP = 0.01


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
    """the culled march whatever the table starts, as tests/test_gpu_area_ghosts.py forces it"""
    lf.test_knob("cull_force", 1)
    pkg.test_knob_default("cull_force", 1)
    yield
    lf.test_knob("cull_force", 0)
    pkg.test_knob_default("cull_force", 0)


def _against_f64(pkg, lf, mask, name, spp, mode=0, bits=6, label=None, min_lit=150):
    """render FRAMES[name] on the device (already _setup) and in float64 from the lights the device stores; the full helper"""
    lens, W, H, key, lights = frame_of(pkg, name)
    lf.set_pupil_subcells(bits)
    _install(lf, lights)
    img, cnt = _frame(pkg, lf, spp, key, mode)
    culled = lf.cull_info()["culled"]
    stored = lfo.lights_of(lf)
    assert [l[0] for l in stored] == [l[0] for l in lights]
    ref, frag, c64 = lfo.g64_trace(lens, W, H, 0, H, spp, key, None, True, mask, [0.0, 0.0, -1.0], [0.0, 0.0, 0.0], 0.05,
                                   n_threads=16, sub_bits=bits, cull=lf.cull_table_and_block(), lights=stored)
    pairs = lfo.g64_last_light_pairs
    lit = ref >= FLOOR
    dev = np.abs(img - ref)
    rel = dev[lit] / ref[lit]
    over = int((dev[lit] > TOL * ref[lit]).sum())
    shares = [e / h for (h, e), l in zip(pairs, stored) if l[0] == AREA and h]
    print(f"{label or name}: {int(lit.sum())} lit values, {over} need the allowance, largest raw deviation {rel.max() if rel.size else 0:.2e}, "
          f"median {np.median(rel) if rel.size else 0:.2e}; rays_hit_light {cnt['rays_hit_light']} (float64 {c64['rays_hit_light']}), "
          f"light_edge_pairs {c64['light_edge_pairs']}, share of its light's lit pairs {max(shares) if shares else 0:.3%}; "
          f"fragile rays {c64['rays_fragile']} of {c64['rays_launched']}")
    assert all(s <= EDGE_CAP for s in shares), shares
    _check_against_f64(img, cnt, ref, frag, c64, min_lit=min_lit, culled=culled, hit_light_slack=c64["light_edge_pairs"])
    return img, cnt, ref, c64


def _prepare(pkg, lf, mask, name):
    lens, W, H, _, _ = frame_of(pkg, name)
    _setup(pkg, lf, lens, W, H, mask)


# ---- 1. point lights ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lamp_near", "lamp_off_axis"])
def test_point_light_ghosts_within_1e4(pkg, lf, mask, name):
    """LAMP 90 mm in front of the lens -- where hz and the exit point matter most -- and a lamp 4.6 r_f away, off the axis; the path
    tree, 256 spp, counters included"""
    _prepare(pkg, lf, mask, name)
    _against_f64(pkg, lf, mask, name, 256)


# ---- 2. area lights ----------------------------------------------------------------------------------------------------------
def test_area_light_ghosts_within_1e4(pkg, lf, mask):
    """the tilted 12 x 8 mm parallelogram at 90 mm: its outline crosses the rays of the frame"""
    _prepare(pkg, lf, mask, "tilted")
    img, cnt, ref, c64 = _against_f64(pkg, lf, mask, "tilted", 256)
    assert c64["light_edge_pairs"] > 0 and 0.05 * cnt["rays_reached_scene"] < cnt["rays_hit_light"] < 0.95 * cnt["rays_reached_scene"]


def test_a_rectangle_seen_from_behind_is_black_on_both_sides(pkg, lf, mask):
    lens, W, H, key, lights = frame_of(pkg, "behind")
    _setup(pkg, lf, lens, W, H, mask)
    _install(lf, lights)
    img, cnt = _frame(pkg, lf, 256, key, 0)
    ref, frag, c64 = lfo.g64_trace(lens, W, H, 0, H, 256, key, None, True, mask, [0.0, 0.0, -1.0], [0.0, 0.0, 0.0], 0.05,
                                   n_threads=16, cull=lf.cull_table_and_block(), lights=lfo.lights_of(lf))
    assert not img.any() and not ref.any()
    assert cnt["rays_hit_light"] == 0 == c64["rays_hit_light"] and c64["light_edge_pairs"] == 0
    assert cnt["rays_launched"] == c64["rays_launched"] and cnt["rays_reached_scene"] > 0
    assert abs(cnt["rays_reached_scene"] - c64["rays_reached_scene"]) <= c64["rays_fragile"]


# ---- 3. mixed kinds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "two_suns"])
def test_several_lights_ghosts_within_1e4(pkg, lf, mask, name):
    """[SUN, LAMP, PANEL] under three different power-of-two radiance triples -- a wrong light's channel factors are another image --
    and two directional lights whose lobes overlap: several lights against a reference that is not a sum of device frames"""
    _prepare(pkg, lf, mask, name)
    img, cnt, ref, c64 = _against_f64(pkg, lf, mask, name, 256)
    assert all(h > 0 for h, _ in lfo.g64_last_light_pairs)          # (every light of the list lights rays of the frame)


# ---- 4. every kernel family -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,bits", [("culled", 6), ("items", 0)])
def test_mixed_lights_within_1e4_in_the_culled_march_and_the_item_kernel(pkg, lf, mask, forced, family, bits):
    _prepare(pkg, lf, mask, "mixed")
    try:
        _against_f64(pkg, lf, mask, "mixed", 64, mode=2, bits=bits, label=f"mixed, {family}")
        assert lf.cull_info()["culled"], lf.cull_reason()
        audit = lf.cull_audit()
        assert audit["rays"] > 0 and audit["lit"] == 0
    finally:
        lf.set_pupil_subcells(6)


# ---- 5. variants -------------------------------------------------------------------------------------------------------------
def test_coated_lens_under_a_panel_and_a_sun_within_1e4(pkg, lf, mask):
    lens, W, H, _, _ = frame_of(pkg, "coated")
    _setup(pkg, lf, lens, W, H, mask)
    lfo.g64_set_films(lens["coatings"])
    try:
        _against_f64(pkg, lf, mask, "coated", 256)
        assert lf.get_ghost_occlusion()["march_variant"] == 4 | 32 | 64 | 1
    finally:
        lfo.g64_set_films(None)
        lf.set_lens_coatings(None)


def test_bilinear_stop_under_a_lamp_within_1e4(pkg, lf, mask):
    _prepare(pkg, lf, mask, "bilinear")
    lf.set_mask_filter(pkg.MASK_BILINEAR)
    lfo.g64_set_mask_filter(1)
    try:
        _against_f64(pkg, lf, mask, "bilinear", 256)
        assert lf.get_ghost_occlusion()["march_variant"] == 4 | 32 | 2
    finally:
        lfo.g64_set_mask_filter(0)
        lf.set_mask_filter(pkg.MASK_NEAREST)
